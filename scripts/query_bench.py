"""Throughput of the device-resident ray queries (cr_intersect_device) on the sponza stand-in.

    python scripts/query_bench.py [--n 21] [--reps 7] [--chunk 22] [--sweep] [--out profiles/query_bench.json]

Three ray sets of 2^n rays (default 2^21), all with unit directions:
  pinhole  coherent pinhole rays of the config's camera, row-major over a 2:1 pixel grid
  ao       ambient-occlusion rays from the pinhole rays' hit points, offset 0.001 along the geometric normal
           (turned against the ray), cosine-distributed directions
  random   uniformly random in-box origins and uniformly random directions
Mray/s per set under "query_route" 0 / 1 / 2 and "query_sort" 0 / 1: torch events around the call on torch's
current stream, warm buffers (two untimed calls first), the median (and the least and the most) of --reps
repetitions.  The baseline is
"query_route" 1: the per-thread kernel cr_intersect runs, on the same device arrays.
--sweep: n = 2^8 .. 2^22 on the ao set, the per-thread kernel against the trace path ("query_trace_min" 0)
in append order and sorted -- where the crossover lies.
Not part of bench.py; prints one JSON object (and writes it to --out).
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "chiaroscuro-raytracer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import chiaroscuro_amd as ca  # noqa: E402
from chiaroscuro_amd import scenes  # noqa: E402


def unit(v):
    return v / v.norm(dim=1, keepdim=True)


def timed(dev, o, d, reps):
    """(median, min, max) ms of cr_intersect_device over the rays (o, d); the hit count as a check value."""
    n = o.shape[0]
    hit = torch.zeros(n, dtype=torch.int32, device=o.device)
    tri = torch.zeros(n, dtype=torch.int32, device=o.device)
    bary = torch.zeros((n, 2), dtype=torch.float32, device=o.device)
    dist = torch.zeros(n, dtype=torch.float32, device=o.device)
    st = torch.cuda.current_stream().cuda_stream

    def call():
        dev.intersect_device(n, o.data_ptr(), d.data_ptr(), hit.data_ptr(), tri.data_ptr(), bary.data_ptr(),
                             dist.data_ptr(), st)

    for _ in range(2):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return (statistics.median(ms), min(ms), max(ms)), int(hit.sum().item()), {"hit": hit, "tri": tri, "dist": dist}


def cell(ms, n):
    med, lo, hi = ms
    return {"ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "mray_s": round(n / med / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=21, help="log2 of the rays per set")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--chunk", type=int, default=0, help="log2 of option \"query_chunk\" (0: the default)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    N = 1 << a.n
    NMAX = max(N, 1 << 22) if a.sweep else N
    gpu = torch.device("cuda:0")
    gen = torch.Generator(device=gpu)
    gen.manual_seed(20)

    scene = ca.Scene(scenes.config_rtc("sponza"))
    model = ca.Model(scene)
    kd = ca.KDTree(model, scene)
    dev = ca.Device(0)
    desc = kd.describe()
    dev.upload(desc)
    info = scene.info
    box = kd.export()["box"]
    lo, hi = torch.tensor(box[:3], device=gpu), torch.tensor(box[3:], device=gpu)

    # pinhole: twice the rays needed, so that the ao set has enough hit points
    yres = 1 << ((NMAX.bit_length()) // 2)
    xres = 2 * NMAX // yres
    cam = ca.camera(info["VP"], info["LA"], info["UP"], info["yview"], xres, yres).as_array()
    eye, lu, dx, dy = (torch.tensor(cam[3 * i: 3 * i + 3], device=gpu) for i in range(4))
    ys, xs = torch.meshgrid(torch.arange(yres, device=gpu), torch.arange(xres, device=gpu), indexing="ij")
    sx, sy = xs.reshape(-1, 1).float() + 0.5, ys.reshape(-1, 1).float() + 0.5
    pd = unit(lu + dx * sx + dy * sy).contiguous()
    po = eye.expand_as(pd).contiguous()

    # the ao set from the pinhole rays' hits (route 1: the per-thread kernel)
    dev.set_option("query_route", 1)
    _, _, r = timed(dev, po, pd, 1)
    h = r["hit"] == 1
    P = torch.tensor(model.triangles()["pos"], device=gpu).reshape(-1, 3, 3)
    t = r["tri"][h].long()
    nrm = unit(torch.cross(P[t, 1] - P[t, 0], P[t, 2] - P[t, 0], dim=1))
    din = pd[h]
    nrm = torch.where((nrm * din).sum(dim=1, keepdim=True) > 0, -nrm, nrm)
    ao_o = (po[h] + r["dist"][h, None] * din + 0.001 * nrm).contiguous()
    u1 = torch.rand(ao_o.shape[0], generator=gen, device=gpu)
    u2 = torch.rand(ao_o.shape[0], generator=gen, device=gpu) * (2 * np.pi)
    rad = u1.sqrt()
    helper = torch.where(nrm[:, :1].abs() > 0.9, torch.tensor([0.0, 1.0, 0.0], device=gpu),
                         torch.tensor([1.0, 0.0, 0.0], device=gpu))
    tx = unit(torch.cross(helper, nrm, dim=1))
    ty = torch.cross(nrm, tx, dim=1)
    ao_d = unit(tx * (rad * u2.cos())[:, None] + ty * (rad * u2.sin())[:, None] +
                nrm * (1 - u1).clamp_min(0).sqrt()[:, None]).contiguous()
    assert ao_o.shape[0] >= NMAX, "not enough hit points for the ao set: %d" % ao_o.shape[0]

    ro = (lo + (hi - lo) * torch.rand((N, 3), generator=gen, device=gpu)).contiguous()
    rd = unit(torch.randn((N, 3), generator=gen, device=gpu)).contiguous()

    def prefix(o, d, n, total):  # n rays spread over the first `total`, order kept
        idx = (torch.arange(n, device=gpu) * (total // n))
        return o[idx].contiguous(), d[idx].contiguous()

    sets = {"pinhole": prefix(po, pd, N, po.shape[0]), "ao": prefix(ao_o, ao_d, N, ao_o.shape[0]), "random": (ro, rd)}
    res = {"scene": "sponza", "triangles": model.num_triangles, "n": N, "reps": a.reps, "sets": {}, "sweep": {}}
    dev.set_option("query_trace_min", 0)
    if a.chunk:
        dev.set_option("query_chunk", 1 << a.chunk)
        res["query_chunk"] = 1 << a.chunk
    for name, (o, d) in sets.items():
        row, hits = {}, set()
        for route in (0, 1, 2):
            for sort in (0, 1):
                if route == 1 and sort == 1:
                    continue  # (the per-thread kernel has no queue)
                dev.set_option("query_route", route)
                dev.set_option("query_sort", sort)
                ms, nh, _ = timed(dev, o, d, a.reps)
                hits.add(nh)
                row["route%d_sort%d" % (route, sort)] = cell(ms, N)
        assert len(hits) == 1, hits
        row["hits"] = hits.pop()
        res["sets"][name] = row
        print(name, json.dumps(row), flush=True)
    if a.sweep:
        for lg in range(8, 23):
            n = 1 << lg
            o, d = prefix(ao_o, ao_d, n, ao_o.shape[0])
            row = {}
            for key, route, sort in (("per_thread", 1, 0), ("trace_append", 0, 0), ("trace_sorted", 0, 1)):
                dev.set_option("query_route", route)
                dev.set_option("query_sort", sort)
                ms, _, _ = timed(dev, o, d, a.reps)
                row[key] = cell(ms, n)
            res["sweep"][str(n)] = row
            print("sweep", n, json.dumps(row), flush=True)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
