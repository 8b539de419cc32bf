"""Device known-answer tests of the helpers under the render kernels (csrc/device_math.hpp,
csrc/render_common.hpp): the branches a rendered scene reaches almost never, or never.

tests/native/devmath_check.hip runs one small kernel per stage over the cases tests/devmath_cases.py writes and
returns the raw output words; every expected value is computed on the host -- by the oracle's KAT exports
(pyoracle), by numpy float32 arithmetic (IEEE round-to-nearest), or read from the reference's own recorded output
(tests/golden/ref_texture.json) -- so the reference is never the code under test.  Everything is compared bit for
bit, NaN as NaN.  tests/test_rng_distributions.py asserts on the CPU that the cases reach the branches named here.

  rng     rng_make's key, 8 rng_u32 draws, rng_uniform (the c >= 1.0f clamp: draws >= 0xFFFFFF80) and rng_index
          (Lemire's rejection loop: with the 2 lights of the test scenes its threshold is 0), with the counter after
          each call, i.e. the draws consumed
  minmax  std_min / std_max / glm_max on all ordered pairs of NaN, +-0, +-inf, 1
  brdf    perpendicular, concentric and sample_wi on the branch boundaries of the unit square and on axis, tied,
          un-normalised, denormal-length and zero normals
  wave    rcp_rn_wave, div_by_rcp_wave and tri_test_wave against their scalar forms and the host, and ray_box_inv
          fed by rcp_rn_wave against ray_box, with 0, 1, 32, 63 and 64 lanes of a wave out of range, the whole wave
          active and inside a divergent branch
  tex     tex_lookup on the reference's 4 x 144 recorded lookups, through an atlas laid out by scene_layout

The harness is built once per module with the product's HIPFLAGS (the package Makefile's).
"""
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import devmath_cases as dc

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "chiaroscuro-raytracer_amd"
pytestmark = pytest.mark.gpu


def product_hipflags():
    """HIPFLAGS of the package Makefile with its defaults substituted (the include paths are given here)."""
    text = (PKG / "Makefile").read_text()
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)[ \t]*[:?]?=[ \t]*(.*)$", text, re.M)}
    var["INC"] = ""
    flags = var["HIPFLAGS"]
    for _ in range(4):
        flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), flags)
    flags = flags.split()
    for need in ("--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", "-ffp-contract=off"):
        assert need in flags, (need, flags)
    return flags


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """run(stage, words) -> (output words as uint32, the JSON line); any non-zero exit status fails the test at
    once, so nothing further is launched after it."""
    work = tmp_path_factory.mktemp("devmath")
    exe = work / "devmath_check"
    hipcc = var_hipcc()
    subprocess.run([hipcc, *product_hipflags(), "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "native" / "devmath_check.hip"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    state = {"dead": None}

    def run(stage, words, name=None):
        assert state["dead"] is None, "not launched: %s" % state["dead"]
        name = name or stage
        fin, fout = work / (name + ".in"), work / (name + ".out")
        np.ascontiguousarray(words, np.uint32).tofile(fin)
        try:
            r = subprocess.run([str(exe), stage, str(fin), str(fout)], capture_output=True, text=True, timeout=60)
        except subprocess.TimeoutExpired:
            state["dead"] = "%s ran into its time limit" % name
            raise
        if r.returncode != 0:
            state["dead"] = "%s ended with status %d: %s" % (name, r.returncode, r.stderr[-500:])
        assert r.returncode == 0, state["dead"]
        return np.fromfile(fout, np.uint8), json.loads(r.stdout.strip().splitlines()[-1])

    return run


def var_hipcc():
    m = re.search(r"^HIPCC[ \t]*\?=[ \t]*(\S+)", (PKG / "Makefile").read_text(), re.M)
    return m.group(1)


def report(name, bad, rec, got, exp, limit=5):
    """Zero mismatching words, or the first few cases with their inputs."""
    rows = np.flatnonzero(bad.reshape(len(bad), -1).any(1))
    msg = ["%s: %d of %d cases differ" % (name, len(rows), len(bad))]
    for i in rows[:limit]:
        msg.append("case %d in %s\n   got %s\n   exp %s" % (
            i, ["%08x" % w for w in np.asarray(rec[i]).reshape(-1)[:40]],
            ["%08x" % w for w in got[i].reshape(-1)], ["%08x" % w for w in exp[i].reshape(-1)]))
    assert len(rows) == 0, "\n".join(msg)


_pass1 = {}


def rng_pass1(harness, po):
    """Pass 1, once per session: key, raw draws and rng_uniform with the counters.  The raw draws of the seeded
    streams are compared with pyoracle.rng_draws; rng_uniform with the oracle's own (or_rng_uniform_kat)."""
    if "ok" not in _pass1:
        _pass1["ok"] = False
        rec, exp, facts = dc.rng_draw_cases()
        assert facts["clamp"] > 0
        for i in np.flatnonzero(rec[:, 0] == 0)[::64]:  # (all of them on the CPU: test_rng_distributions)
            assert exp[i, 1:9].tolist() == po.rng_draws(*rec[i, 1:5].tolist(), 8).tolist()
        raw, info = harness("rng", rec.reshape(-1), "rng_draws")
        got = raw.view(np.uint32).reshape(-1, 14)
        assert info["cases"] == len(rec) == len(got)
        report("rng draws / rng_uniform", dc.same_words(got, exp, float_cols=[10]), rec, got, exp)
        _pass1["ok"] = True
    return _pass1["ok"]


def test_rng_draws_and_uniform(harness, po):
    assert rng_pass1(harness, po), "failed earlier in this session"


def test_rng_index(harness, po):
    """Pass 2: rng_index for every n of the list on the random streams and on the crafted rejection streams.
    Runs only after pass 1 passed: the rejection loop ends exactly when the draws are the CPU's, so a wrong draw
    stream has to fail pass 1 and must not spin a kernel here."""
    assert rng_pass1(harness, po), "the raw draws are not the CPU's on this GPU: rng_index is not launched"
    rec, exp, facts = dc.rng_index_cases()
    assert all(c > 0 for c in facts["rejections"]), facts
    raw, info = harness("rng", rec.reshape(-1), "rng_index")
    got = raw.view(np.uint32).reshape(-1, 14)
    assert info["cases"] == len(rec) == len(got)
    report("rng_index", dc.same_words(got, exp, float_cols=[]), rec, got, exp)


def test_rng_distributions_match_reference_libstdcxx(harness, po):
    """G3 (tests/golden/ref_brdf.npz, read by tests/refpin.py): rng_uniform against what libstdc++'s own uniform_real_distribution<float>
    made of the same word in the reference's uniformFloat, and rng_index against Scene::randomLight through
    uniform_int_distribution -- values and words consumed, n = 1 included.  The golden bits, not the oracle's."""
    assert rng_pass1(harness, po), "the raw draws are not the CPU's on this GPU: rng_index is not launched"
    import refpin
    g = refpin.load_brdf()
    rec = [[1, dc.unmix32(c["word"]), 0, 0, 0, 1, c["a"], c["b"]] for c in g["uniform"]]
    rec += [[1, c["key"], 0, 0, 0, 2, c["n"], 0] for c in g["index"]]
    raw, info = harness("rng", np.array(rec, np.uint32).reshape(-1), "rng_refpin")
    got = raw.view(np.uint32).reshape(-1, 14)
    nu = len(g["uniform"])
    assert info["cases"] == len(rec) == len(got) and nu >= 400 and len(g["index"]) >= 256
    exp_u = np.array([[c["out"], c["consumed"]] for c in g["uniform"]], np.uint32)
    assert [int(w) for w in got[:nu, 1]] == [c["word"] for c in g["uniform"]]  # (the scripted word was the draw)
    report("rng_uniform vs libstdc++", dc.same_words(got[:nu, 10:12], exp_u, float_cols=[0]), rec[:nu], got[:nu, 10:12],
           exp_u)
    exp_i = np.array([[c["index"], c["consumed"]] for c in g["index"]], np.uint32)
    assert got[nu:, 1:9].tolist() == [c["words"][:8] for c in g["index"]]
    report("rng_index vs libstdc++", dc.same_words(got[nu:, 12:14], exp_i, float_cols=[]), rec[nu:], got[nu:, 12:14],
           exp_i)


def test_brdf_matches_reference(harness):
    """G3: sample_wi against the reference's own Diffuse::sample_wi (src/brdf.cpp) on the sx, sy its
    uniformFloat(-1, 1) produced: wi and pdf bits."""
    import refpin
    g = refpin.load_brdf()["sample_wi"]
    rec = np.array([c["n"] + [c["sx"], c["sy"]] for c in g], np.uint32)
    exp = np.array([c["wi"] + [c["pdf"]] for c in g], np.uint32)
    raw, info = harness("brdf", rec.reshape(-1), "brdf_refpin")
    got = raw.view(np.uint32).reshape(-1, 9)
    assert info["cases"] == len(rec) == len(got) >= 1500
    report("sample_wi vs the reference", dc.same_words(got[:, 5:9], exp), rec, got[:, 5:9], exp)


def test_minmax(harness):
    rec, exp = dc.minmax_cases()
    raw, info = harness("minmax", rec.reshape(-1))
    got = raw.view(np.uint32).reshape(-1, 3)
    assert info["cases"] == 36 == len(got)
    report("std_min / std_max / glm_max", dc.same_words(got, exp), rec, got, exp, limit=36)


def test_brdf(harness):
    rec, exp, facts = dc.brdf_cases()
    assert all(facts["branches"]) and facts["pdf_zero"] and facts["hz_clamped"], facts
    raw, info = harness("brdf", rec.reshape(-1))
    got = raw.view(np.uint32).reshape(-1, 9)
    assert info["cases"] == len(rec) == len(got)
    bad = dc.same_words(got, exp)
    report("perpendicular", bad[:, 0:3], rec, got, exp)
    report("concentric", bad[:, 3:5], rec, got, exp)
    report("sample_wi", bad[:, 5:9], rec, got, exp)


def test_wave(harness):
    """Required equalities: tri_test_wave == tri_test == restatement on the accept flag (tri_test_wave's with the
    lane's `live`); ux, uy, t bit for bit on accepting lanes (a rejecting lane's are unspecified and not
    compared); rcp_rn_wave == rcp_rn == 1 / a, div_by_rcp_wave == div_by_rcp == a / b, ray_box_inv == ray_box ==
    restatement; lanes outside the active mask hold the sentinel."""
    lanes, masks, exp, facts = dc.wave_cases()
    runs = dc.wave_expected_runs(masks, exp)
    keep = dc.wave_compare_mask(runs)
    raw, info = harness("wave", dc.wave_input_words(lanes, masks))
    got = raw.view(np.uint32).reshape(runs.shape)
    assert info["groups"] == len(lanes)
    bad = dc.same_words(got, runs, float_cols=[0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15]) & keep
    g = len(lanes)
    rec2 = np.concatenate([lanes, lanes]).reshape(2 * g * 64, 32)
    got2, exp2, bad2 = got.reshape(-1, 16), runs.reshape(-1, 16), bad.reshape(-1, 16)
    for name, cols in (("rcp_rn_wave / rcp_rn", [0, 1]), ("div_by_rcp_wave / div_by_rcp", [2, 3]),
                       ("tri_test_wave", [4, 5, 6, 7]), ("tri_test", [8, 9, 10, 11]), ("ray_box", [12, 13]),
                       ("ray_box_inv of rcp_rn_wave", [14, 15])):
        report(name + " (rows: run 0 groups x lanes, then run 1)", bad2[:, cols], rec2, got2, exp2)


def test_tex_lookup(harness):
    """tex_lookup against the reference's own recorded output for its 4 x 144 lookups (wrap loops, u == 1.0 read
    from the pad, negative and > 1 coordinates), with the four textures in one atlas laid out by the product's
    scene_layout.  NaN coordinates: the reference's index is undefined behaviour there (and infinities never
    terminate in it: left out), so the only claim is that the device returns three finite values read from
    inside the texture's own padded part of the atlas."""
    words, texs, cases, rgb, n_ref = dc.texture_cases()
    raw, info = harness("tex", words)
    n = len(cases)
    assert info["cases"] == n and info["textures"] == len(texs)
    got = raw[:12 * n].view(np.uint32).reshape(n, 3)
    layout = raw[12 * n:12 * n + 16 * len(texs)].view(np.uint32).reshape(-1, 4)
    atlas = raw[12 * n + 16 * len(texs):]
    assert len(atlas) == info["atlas_bytes"]
    # the layout the lookups ran on: scene_layout's (16-byte aligned, the image, zeros to the next texture)
    end = 0
    for (w, h, nc, img), (lw, lh, lnc, off) in zip(texs, layout.tolist()):
        assert (lw, lh, lnc) == (w, h, nc) and off % 16 == 0 and off >= end
        assert not atlas[end:off].any() and np.array_equal(atlas[off:off + len(img)], img)
        end = off + len(img)
        pad_end = off + len(img) + (w + 1) * nc + 4
        assert pad_end <= len(atlas) and not atlas[end:pad_end].any()
    report("tex_lookup", got[:n_ref] != rgb, cases, got[:n_ref], rgb)
    scale = np.float32(0.00392156862)
    for (ti, u, v), px in zip(cases[n_ref:].tolist(), got[n_ref:]):
        w, h, nc, img = texs[ti]
        off = int(layout[ti, 3])
        part = atlas[off:off + len(img) + (w + 1) * nc + 4]
        triples = {tuple(dc.bits(part[i:i + 3].astype(np.float32) * scale).tolist()) for i in range(len(part) - 2)}
        assert np.isfinite(px.view(np.float32)).all() and tuple(px.tolist()) in triples, (ti, hex(u), hex(v), px)
