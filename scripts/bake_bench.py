"""What a lightmap bake costs, stage by stage, on the sponza stand-in.

    python scripts/bake_bench.py [--cell 4] [--spp 16] [--passes 4] [--rounds 3] [--out profiles/bake_bench.jsonl]

The map is the grid atlas of the scene's triangles at --cell texels per cell (cell 4: 2048 x 2044).  Per round, after
a warm-up round in which the buffers grow:
  surface   cr_bake_surface_device -- owner pass, surface pass and compaction -- between two events on the stream;
  gather    cr_gather_list_device over the covered list, one layer of --spp samples: cr_last_kernel_ms and the
            counters, Mray/s = (closest + shadow queries) / device time, the figure of scripts/radiance_bench.py;
  dilate    cr_bake_dilate_device, --passes passes, between two events.
The texture-space rows also give bytes / time against the bytes the stage must move (surface: the owner map preset,
written by the atomics' texels and read twice, pos, nrm and the list written; dilate: the copy, and per pass the level
map read and the filled texels written).  Not part of bench.py; one JSON object per line (and into --out).
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", type=int, default=4)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    gpu = torch.device("cuda:0")
    scene = ca.Scene(scenes.config_rtc("sponza"))
    model = ca.Model(scene)
    kd = ca.KDTree(model, scene)
    dev = ca.Device(0)
    dev.upload(kd.describe())
    dev.set_option("counters", 0)  # the lean default build, as the bench times it
    info = scene.info
    k, seed, bg = info["k"], info["seed"], tuple(info["background"])
    W, H, uv = ca.bake_atlas_grid(model.num_triangles, a.cell)
    n = W * H
    d_uv = torch.from_numpy(uv).to(gpu)
    owner = torch.zeros(n, dtype=torch.int32, device=gpu)
    lst = torch.zeros(n, dtype=torch.int32, device=gpu)
    count = torch.zeros(1, dtype=torch.int32, device=gpu)
    pos, nrm, out, dil = (torch.zeros((n, 3), dtype=torch.float32, device=gpu) for _ in range(4))
    bp = ca.bake_params(W, H, spp=a.spp, k=k, seed=seed, background=bg)
    rp = ca.radiance_params(a.spp, k, seed, bg)
    rows = [{"kind": "setup", "scene": "sponza", "triangles": model.num_triangles, "cell": a.cell, "map": [W, H],
             "texels": n, "spp": a.spp, "k": k, "passes": a.passes}]
    print(json.dumps(rows[0]), flush=True)

    def surface():
        dev.bake_surface_device(bp, d_uv.data_ptr(), owner.data_ptr(), pos.data_ptr(), nrm.data_ptr(), lst.data_ptr(),
                                count.data_ptr(), 0)

    for rnd in range(a.rounds + 1):  # round 0: the warm-up
        tag = "_warmup" if rnd == 0 else ""
        ms = timed(surface)
        covered = int(count.item())
        # preset 4 n, owner read by the surface pass and the scatter 8 n, pos / nrm 24 n, the list 4 covered
        moved = 36 * n + 4 * covered
        r = {"kind": "surface" + tag, "round": rnd, "ms": round(ms, 3), "covered": covered, "bytes": moved,
             "gb_s": round(moved / ms / 1e6, 1)}
        print(json.dumps(r), flush=True)
        rows.append(r)
        dev.gather_list_device(n, pos.data_ptr(), nrm.data_ptr(), lst.data_ptr(), covered, rp, 1, out.data_ptr(), 0, 0)
        torch.cuda.synchronize()
        gc, gms = dev.counters(), dev.last_kernel_ms()
        r = {"kind": "gather" + tag, "round": rnd, "ms": round(gms, 3), "paths": gc["paths"], "closest": gc["closest"],
             "shadow": gc["shadow"], "mray_s": round((gc["closest"] + gc["shadow"]) / gms / 1e3, 1),
             "build": dev.last_trace_build()}
        print(json.dumps(r), flush=True)
        rows.append(r)
        ms = timed(lambda: dev.bake_dilate_device(W, H, owner.data_ptr(), a.passes, out.data_ptr(), dil.data_ptr(), 0))
        # the copy 24 n and the level map 8 n, then per pass the level map read (4 n) -- the neighbour reads and the
        # filled texels' writes come on top and are not counted: a floor
        moved = 32 * n + a.passes * 4 * n
        r = {"kind": "dilate" + tag, "round": rnd, "ms": round(ms, 3), "bytes_floor": moved,
             "gb_s_floor": round(moved / ms / 1e6, 1)}
        print(json.dumps(r), flush=True)
        rows.append(r)
    summary = {"kind": "summary", "gather_from_camera_hit_points_mray_s": 857.0}  # (§3.28, radiance_bench.jsonl)
    for kind in ("surface", "gather", "dilate"):
        v = [r["ms"] for r in rows if r.get("kind") == kind]
        summary[kind + "_ms"] = {"median": float(np.median(v)), "min": min(v), "max": max(v)}
    summary["gather_mray_s_median"] = float(np.median([r["mray_s"] for r in rows if r.get("kind") == "gather"]))
    total = sum(summary[kind + "_ms"]["median"] for kind in ("surface", "gather", "dilate"))
    summary["share"] = {kind: round(summary[kind + "_ms"]["median"] / total, 4) for kind in ("surface", "gather", "dilate")}
    print(json.dumps(summary), flush=True)
    rows.append(summary)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
