"""Throughput of the SH irradiance probes (cr_probe_sh_device, cr_probe_sample_device) on the sponza stand-in, beside
the gather of DESIGN.md §3.28 measured in the same run, and the agreement of a probe with a direct gather (§3.30).

    python scripts/probe_bench.py [--dims 64x32x64] [--spp 256] [--rounds 3] [--queries 2073600]
                                  [--gather-res 1920x1080] [--gather-spp 64] [--out profiles/probe_bench.jsonl]

Probes: a --dims grid over the scene's bounding box, --spp samples, one layer; one warm-up call, then --rounds rounds
alternating with the gather (the first hits of a --gather-res camera's centre rays, as scripts/radiance_bench.py makes
them).  Mray/s = (closest + shadow queries) / device-event time (cr_get_counters, cr_last_kernel_ms); "other_ms" is
that time less the trace kernels' (generation 0, shade, resolve, sorts and the sum).  The lookup: --queries points
uniform in the box, timed with events around the call.  The time of sum_samples_sh alone comes from a kernel trace of
this script (--rounds 1 --no-gather under rocprofv3 --kernel-trace --stats); "sum_bytes" is what it must move: 12 B per
path and 108 B per probe.  Agreement: at 64 surface points of the cornell box a probe 0.001 off the surface, 4096
samples, evaluated for the surface normal, against cr_gather there at 4096 samples -- L2 truncation and noise both
enter.  Not part of bench.py; one JSON object per line (and into --out).
"""
import argparse
import json
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


def load(name):
    scene = ca.Scene(scenes.config_rtc(name))
    model = ca.Model(scene)
    dev = ca.Device(0)
    dev.upload(ca.KDTree(model, scene).describe())
    dev.set_option("counters", 0)  # the lean default build, as the bench times it
    return scene, model, dev


def surface_points(dev, model, o, d):
    """(pos, nrm) of the rays that hit: the point 0.001 off the surface along the normal turned against the ray."""
    q = dev.intersect_tensors(o, d)
    torch.cuda.synchronize()
    h = q["hit"] == 1
    P = torch.tensor(model.triangles()["pos"], device=o.device).reshape(-1, 3, 3)
    t = q["tri"][h].long()
    nrm = unit(torch.cross(P[t, 1] - P[t, 0], P[t, 2] - P[t, 0], dim=1))
    nrm = torch.where((nrm * d[h]).sum(dim=1, keepdim=True) > 0, -nrm, nrm)
    return (o[h] + q["dist"][h, None] * d[h] + 0.001 * nrm).contiguous(), nrm.contiguous()


def agreement(gpu):
    scene, model, dev = load("cornell")
    info = scene.info
    k, seed, bg = info["k"], info["seed"], tuple(info["background"])
    tri = np.asarray(model.triangles()["pos"], np.float64).reshape(-1, 3)
    lo, hi = tri.min(axis=0), tri.max(axis=0)
    rng = np.random.default_rng(64)
    o = torch.tensor(((lo + hi) / 2 + (hi - lo) * 0.4 * rng.uniform(-1, 1, (512, 3))).astype(np.float32), device=gpu)
    d = torch.tensor(rng.normal(size=(512, 3)).astype(np.float32), device=gpu)
    pos, nrm = surface_points(dev, model, o, d)
    pos, nrm = pos[:64].contiguous(), nrm[:64].contiguous()
    n = int(pos.shape[0])
    spp, layers = 256, 16
    rp = ca.radiance_params(spp, k, seed, bg)
    sh = torch.zeros((n, 27), dtype=torch.float32, device=gpu)
    direct = torch.zeros((n, 3), dtype=torch.float32, device=gpu)
    ev = torch.zeros((n, 3), dtype=torch.float32, device=gpu)
    dev.probe_sh_device(n, pos.data_ptr(), rp, layers, sh.data_ptr(), 0, 0)
    dev.gather_device(n, pos.data_ptr(), nrm.data_ptr(), rp, layers, direct.data_ptr(), 0, 0)
    idx = torch.arange(n, dtype=torch.int32, device=gpu)
    dev.probe_eval_device(n, sh.data_ptr(), idx.data_ptr(), nrm.data_ptr(), ev.data_ptr(), 0)
    torch.cuda.synchronize()
    a, b = ev.cpu().numpy().astype(np.float64), direct.cpu().numpy().astype(np.float64)
    rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-6)
    dev.close()
    return {"kind": "agreement", "scene": "cornell", "points": n, "samples": spp * layers, "k": k,
            "rel_mean": round(float(rel.mean()), 4), "rel_max": round(float(rel.max()), 4),
            "gather_mean": round(float(b.mean()), 5), "probe_mean": round(float(a.mean()), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="64x32x64")
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--queries", type=int, default=2073600)
    ap.add_argument("--gather-res", default="1920x1080")
    ap.add_argument("--gather-spp", type=int, default=64)
    ap.add_argument("--no-gather", action="store_true")
    ap.add_argument("--no-agreement", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dims = tuple(int(v) for v in a.dims.split("x"))
    gpu = torch.device("cuda:0")
    scene, model, dev = load("sponza")
    info = scene.info
    k, seed, bg = info["k"], info["seed"], tuple(info["background"])
    tri = np.asarray(model.triangles()["pos"], np.float64).reshape(-1, 3)
    lo, hi = tri.min(axis=0), tri.max(axis=0)
    grid = ca.probe_grid(lo, (hi - lo) / (np.array(dims) - 1), dims)
    n = grid.count
    pos = torch.from_numpy(ca.probe_grid_positions(grid)).to(gpu)
    sh = torch.zeros((n, 27), dtype=torch.float32, device=gpu)
    rp = ca.radiance_params(a.spp, k, seed, bg)
    calls = {"probe_sh": lambda: dev.probe_sh_device(n, pos.data_ptr(), rp, 1, sh.data_ptr(), 0, 0)}
    rows = [{"kind": "setup", "scene": "sponza", "triangles": model.num_triangles, "dims": a.dims, "probes": n,
             "spp": a.spp, "k": k}]

    if not a.no_gather:
        xres, yres = (int(v) for v in a.gather_res.split("x"))
        cam = ca.camera(info["VP"], info["LA"], info["UP"], info["yview"], xres, yres)
        c = cam.as_array()
        eye, lu, dx, dy = (torch.tensor(c[3 * i: 3 * i + 3], device=gpu) for i in range(4))
        ys, xs = torch.meshgrid(torch.arange(yres, device=gpu), torch.arange(xres, device=gpu), indexing="ij")
        d = (lu + dx * (xs.reshape(-1, 1).float() + 0.5) + dy * (ys.reshape(-1, 1).float() + 0.5)).contiguous()
        gp, gn = surface_points(dev, model, eye.expand_as(d).contiguous(), d)
        idx = torch.arange(xres * yres, device=gpu) % int(gp.shape[0])  # (pixels without a hit reuse the first points)
        gp, gn = gp[idx].contiguous(), gn[idx].contiguous()
        gout = torch.zeros((xres * yres, 3), dtype=torch.float32, device=gpu)
        grp = ca.radiance_params(a.gather_spp, k, seed, bg)
        calls["gather"] = lambda: dev.gather_device(xres * yres, gp.data_ptr(), gn.data_ptr(), grp, 1, gout.data_ptr(), 0, 0)
        rows[0].update(gather_points=xres * yres, gather_spp=a.gather_spp)
    print(json.dumps(rows[0]), flush=True)

    def row(kind, rnd):
        gc, ms = dev.counters(), dev.last_kernel_ms()
        ts = dev.trace_stats()
        trace = {kk: round(v["ms"], 3) for kk, v in ts.items() if isinstance(v, dict) and v.get("launches")}
        r = {"kind": kind, "round": rnd, "paths": gc["paths"], "closest": gc["closest"], "shadow": gc["shadow"],
             "ms": round(ms, 3), "mray_s": round((gc["closest"] + gc["shadow"]) / ms / 1e3, 1),
             "build": dev.last_trace_build(), "trace_ms": trace}
        if kind.startswith("probe_sh"):
            r["sum_bytes"] = gc["paths"] * 12 + n * 108
        print(json.dumps(r), flush=True)
        return r

    for kind, call in calls.items():  # warm-up: the buffers grow here
        call()
        torch.cuda.synchronize()
        row(kind + "_warmup", 0)
    for rnd in range(1, a.rounds + 1):
        for kind, call in calls.items():
            call()
            torch.cuda.synchronize()
            rows.append(row(kind, rnd))

    # the lookup
    m = a.queries
    rng = torch.Generator(device=gpu).manual_seed(7)
    box_lo, box_hi = torch.tensor(lo, dtype=torch.float32, device=gpu), torch.tensor(hi, dtype=torch.float32, device=gpu)
    qp = (box_lo + (box_hi - box_lo) * torch.rand((m, 3), generator=rng, device=gpu)).contiguous()
    qn = unit(torch.randn((m, 3), generator=rng, device=gpu)).contiguous()
    qo = torch.zeros((m, 3), dtype=torch.float32, device=gpu)
    for rnd in range(0, a.rounds + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dev.probe_sample_device(grid, sh.data_ptr(), m, qp.data_ptr(), qn.data_ptr(), qo.data_ptr(), 0)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        r = {"kind": "probe_sample" + ("_warmup" if rnd == 0 else ""), "round": rnd, "queries": m, "ms": round(ms, 4),
             "mquery_s": round(m / ms / 1e3, 1)}
        print(json.dumps(r), flush=True)
        if rnd:
            rows.append(r)

    summary = {"kind": "summary"}
    for kind in calls:
        v = [r["mray_s"] for r in rows if r.get("kind") == kind]
        summary[kind] = {"mray_s_median": float(np.median(v)), "mray_s_min": min(v), "mray_s_max": max(v)}
    v = [r["ms"] for r in rows if r.get("kind") == "probe_sample"]
    summary["probe_sample"] = {"ms_median": float(np.median(v)), "ms_min": min(v), "ms_max": max(v)}
    if "gather" in calls:
        summary["probe_over_gather"] = round(summary["probe_sh"]["mray_s_median"] / summary["gather"]["mray_s_median"], 4)
    print(json.dumps(summary), flush=True)
    rows.append(summary)
    dev.close()
    if not a.no_agreement:
        rows.append(agreement(gpu))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
