"""CPU checks that go with the device known-answer tests (tests/test_gpu_devmath.py).

1. The restated libstdc++ distributions against the real ones.  oracle.c rng_uniform / rng_index (and
   device_math.hpp, the same lines) restate generate_canonical<float, 24> and the Lemire path of
   uniform_int_distribution of libstdc++ 11; until now they were compared with nothing but each other.
   tests/native/rngdist_check.cpp feeds a scripted URBG through this machine's std::uniform_real_distribution<float>
   and std::uniform_int_distribution<int> on the draws of every case of the GPU test -- the crafted first draws
   0, 1, 0x7F, 0x80, 0xFFFFFF7F, 0xFFFFFF80 (the first that clamps), 0xFFFFFF81, 0xFFFFFFFF in the three call
   shapes, the random streams, every n of the list, and the crafted rejection streams -- and the values and the
   number of draws consumed are compared with the oracle's KAT exports.  An int holds n up to 2^31; the larger n
   go through uniform_int_distribution<unsigned>, the same code path (and so do the small ones, as well).
2. The host-side case generators (tests/devmath_cases.py) meet the coverage conditions the GPU tests rest on:
   rejection counts 0, 1, 2 and >= 3, a clamping draw, each of concentric()'s branches, pdf == 0, hz clamped, and
   the lane mixes of the wave groups.  All of it from the oracle and numpy alone.
"""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import devmath_cases as dc

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def rngdist(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rngdist") / "rngdist_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall",
                    str(ROOT / "tests" / "native" / "rngdist_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)

    def run(lines):
        path = exe.parent / "cases.txt"
        path.write_text("\n".join(lines) + "\n")
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120, check=True)
        out = r.stdout.splitlines()
        assert out[0].startswith("libstdc++ ") and len(out) == len(lines) + 1, out[:2]
        return out[0], out[1:]

    return run


def test_mix32_restatement_and_inverse(po):
    """The Python mix32 the case generators solve streams with is the oracle's, and unmix32 inverts it."""
    for seed, layer, pixel, sample in dc.rng_streams()[:512].tolist():
        key = dc.rng_key(seed, layer, pixel, sample)
        assert dc.raw_draws(key, 0, 8) == po.rng_draws(seed, layer, pixel, sample, 8).tolist()
    r = np.random.default_rng(7)
    for x in [0, 1, 0xFFFFFFFF, 0x80000000] + r.integers(0, 1 << 32, 2000).tolist():
        assert dc.unmix32(dc.mix32(x)) == x and dc.mix32(dc.unmix32(x)) == x
    x = r.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)
    assert dc.mix32(x).tolist() == [dc.mix32(int(v)) for v in x]


def test_uniform_real_distribution_is_the_restated_one(rngdist):
    """std::uniform_real_distribution<float>(a, b) == oracle rng_uniform, value bits and draws consumed, on every
    rng_uniform case of the GPU test.  (libstdc++ newer than the 11 the oracle cites may redraw where the
    restatement clamps: then this is an expected failure naming the version and the draw)"""
    rec, exp, facts = dc.rng_draw_cases()
    assert facts["clamp"] > 0
    lines = ["R %d %d %s" % (c[6], c[7], " ".join(str(d) for d in e[1:9])) for c, e in zip(rec.tolist(), exp.tolist())]
    lib, out = rngdist(lines)
    bad = []
    for c, e, o in zip(rec.tolist(), exp.tolist(), out):
        ctr0 = 0 if c[0] == 0 else c[2]
        want = "%d %d" % (e[10], (e[11] - ctr0) & dc.M32)
        if o != want:
            bad.append("draw 0x%08x a=%r b=%r: library %s, restatement %s" % (
                e[1], float(dc.f32(c[6])), float(dc.f32(c[7])), o, want))
    if bad and int(lib.split()[1]) > 11:
        pytest.xfail("%s differs from the restated libstdc++ 11 generate_canonical in %d cases; first: %s" % (
            lib, len(bad), bad[0]))
    assert not bad, (lib, len(bad), bad[:5])


def test_uniform_int_distribution_is_the_restated_one(rngdist):
    """std::uniform_int_distribution<int>(0, n - 1) == oracle rng_index, value and draws consumed, on every
    rng_index case of the GPU test (n > 2^31 through the unsigned instantiation)."""
    rec, exp, facts = dc.rng_index_cases()
    lines, want = [], []
    for c, e in zip(rec.tolist(), exp.tolist()):
        key, ctr, n = c[1], c[2], c[6]
        consumed = (e[13] - ctr) & dc.M32
        draws = " ".join(str(d) for d in dc.raw_draws(key, ctr, consumed + 2))
        for kind in ("I", "U") if n <= 2 ** 31 else ("U",):
            lines.append("%s %d %s" % (kind, n, draws))
            want.append("%d %d" % (e[12], consumed))
    lib, out = rngdist(lines)
    bad = [(l[:40], o, w) for l, o, w in zip(lines, out, want) if o != w]
    assert not bad, (lib, len(bad), bad[:5])
    assert sum(1 for l in lines if l[0] == "I") > 6 * dc.N_STREAMS


def test_case_generators_meet_the_coverage_conditions():
    """What keeps the GPU tests from hiding a gap, asserted on the oracle's expected values alone."""
    # RNG: a clamping draw; every rejection count; the rejection loop runs for the small n of real scenes too;
    # crafted streams with 0..3 rejections before a draw on thr - 1 and on thr
    _, _, f = dc.rng_draw_cases()
    assert f["clamp"] >= 3 * 3 * 10  # three crafted clamping draws x three counters x ten call shapes
    assert [dc.clamps(d) for d in dc.EDGE_DRAWS] == [False] * 4 + [False, True, True, True]
    _, _, f = dc.rng_index_cases()
    assert all(c > 0 for c in f["rejections"]), f
    assert f["rejections"][3] >= 100, f  # n = 2^31 + 1: one stream in eight
    assert f["rejecting_small_n"] >= 3, f  # n = 3, 5, 7 with the first draw on thr - 1
    assert f["crafted_boundary"] == [(k, w) for k in (0, 1, 2, 3) for w in (-1, 0)], f
    # minmax: all 36 ordered pairs
    rec, exp = dc.minmax_cases()
    assert len({tuple(r) for r in rec.tolist()}) == 36 and exp.shape == (36, 3)
    # BRDF
    grid, rnd = dc.brdf_pairs()
    assert len(grid) == 18 * 18 and len(rnd) == 1 << 15
    assert float(np.abs(rnd).max()) <= 1.0 and len(np.unique(rnd)) > 60000
    ties = [(float(a), float(b)) for a, b in grid if abs(a) == abs(b)]
    assert len(ties) == 4 + 8 * 4  # (+-0, +-0) and every diagonal and anti-diagonal tie
    rec, exp, f = dc.brdf_cases()
    assert all(c > 0 for c in f["branches"]), f  # the (0, 0) return and the five assignments
    assert f["branches"][0] == 4  # (+-0, +-0)
    assert f["pdf_zero"] > 0 and f["hz_clamped"] > 0 and f["pdf_nan"] > 0, f
    n = dc.brdf_normals()
    assert (np.abs(n[:, 0]) == np.abs(n[:, 1])).sum() >= 6 and len(n) >= 6 + 4 + 64 + 3 + 1
    assert len(rec) == len(grid) * len(n) + len(rnd) and len(rec) < 300000
    # wave: per pattern and mask the number of lanes failing each range test is exactly the pattern's, under
    # every mask; the masked runs see mixed, all-failing and all-passing active sets
    lanes, masks, exp, facts = dc.wave_cases()
    want = {"0": 0, "1@0": 1, "1@31": 1, "1@32": 1, "1@63": 1, "32": 32, "63": 63, "64": 64}
    seen = set()
    for g in facts:
        for key in ("rcp_fail", "div_fail", "tri_big", "box_fail"):
            assert g[key] == want[g["pattern"]], g
        seen.add((g["pattern"], g["mask"]))
    assert seen == {(p, m) for p in want for m in dc.MASKS}
    for pos in (0, 31, 32, 63):
        g = [i for i, f_ in enumerate(facts) if f_["pattern"] == "1@%d" % pos]
        assert all(not dc.rcp_in_range(dc.f32(lanes[i, pos, 0])) for i in g)
    assert {g["active"] for g in facts} == {64, 32, 1}
    for key in ("rcp_fail_active", "div_fail_active"):
        mixed = [g for g in facts if 0 < g[key] < g["active"]]
        assert {g["mask"] for g in mixed} == {"full", "low32", "alternate"}, key
        assert any(g[key] == g["active"] == 1 for g in facts) and any(g[key] == 0 and g["active"] == 1 for g in facts)
    tot = {k: sum(g[k] for g in facts) for k in facts[0] if isinstance(facts[0][k], int)}
    assert tot["tri_accept"] > 500 and tot["tri_big_accept"] > 50 and tot["edge_hits"] > 100, tot
    assert tot["t_zero"] > 20 and tot["t_at_tmax"] > 20 and tot["aa_near_eps"] > 200, tot
    assert tot["tri_fail"] > tot["tri_big"]  # degenerate triangles too: rejected lanes that still reach the blend
    runs = dc.wave_expected_runs(masks, exp)
    assert (runs[1] == dc.SENTINEL).all(-1).sum() == sum(64 - g["active"] for g in facts)
    # texture: the reference's 4 x 144 vectors and the NaN coordinates
    _, texs, cases, rgb, n_ref = dc.texture_cases()
    assert n_ref == 4 * 144 == len(rgb) and len(texs) == 4 and len(cases) == n_ref + 16
    one = dc.b1(1.0)
    assert ((cases[:n_ref, 1] == one) | (cases[:n_ref, 2] == one)).sum() > 0  # u == 1.0: the over-read into the pad


def test_triangle_and_box_restatements_agree_with_the_oracle(po):
    """The numpy restatements the wave stage is compared with are the oracle's own tri_test / ray_box: single
    triangles through or_intersect (a one-leaf tree: the root slab, then the triangle) give the same accept flag,
    barycentrics and distance."""
    r = np.random.default_rng(11)
    n_hit = 0
    for _ in range(200):
        A, e1, e2 = (r.uniform(-1, 1, 3).astype(np.float32) for _ in range(3))
        B, Cc = (A + e1).astype(np.float32), (A + e2).astype(np.float32)
        e1, e2 = B - A, Cc - A  # what the records hold: kdtree.cpp:222-223
        tris = {"pos": np.concatenate([A, B, Cc])[None], "vnrm": np.zeros((1, 9), np.float32),
                "uv": np.zeros((1, 6), np.float32), "kd": np.zeros((1, 3), np.float32),
                "ke": np.zeros((1, 3), np.float32), "tex": -np.ones(1, np.int32)}
        sc = po.OracleScene(tris)
        bu, bv = r.uniform(-0.1, 0.7, 2)
        o = r.uniform(-3, 3, (1, 3)).astype(np.float32)
        d = ((A + np.float32(bu) * e1 + np.float32(bv) * e2) - o).astype(np.float32)
        got = sc.intersect(o, d)
        ok, ux, uy, t, _ = dc.tri_model(o, d, A[None], e1[None], e2[None], np.float32(np.inf))
        box = sc.kd_export()["box"]
        first, second = dc.box_model(o, d, box[None, :3], box[None, 3:])
        # kdtree.cpp:210-216: the root slab first, and the leaf accepts t below the slab's exit
        want = bool(not (second[0] < 0 or second[0] < first[0]) and ok[0] and t[0] < second[0])
        assert bool(got["hit"][0]) == want
        if want:
            assert dc.bits(got["bary"][0]).tolist() == [dc.b1(ux[0]), dc.b1(uy[0])]
            assert dc.b1(got["dist"][0]) == dc.b1(t[0])
            n_hit += 1
    assert n_hit > 50
