"""One kd decision's short forms (csrc/traverse.hpp kd_step) on the GPU, bit for bit.

kd_step takes the side of the split plane from the sign of the difference it has already formed (device_math.hpp
kd_below), divides with one range test where the scene bounds the dividend (div_by_rcp_wave_bounded, the tc::Fixed
instantiations), and forms the chosen child with a carry-in add.  The answers must stay the reference's:

  helpers   a known-answer run of kd_below and div_by_rcp_wave_bounded on the device (tests/native/kdstep_check.hip)
            over edge vectors: every sign combination, oa == split with da in {-0, +0, tiny, negative, positive, an
            axis whose reciprocal is NaN}, denormal differences, dividends up to 2^20, quotients next to rounding
            midpoints, lanes inside and outside the short division's range mixed in one wave.  Expected values are
            numpy float32 arithmetic (IEEE round-to-nearest) on the host.
  renders   cornell 64 x 64 x 4 spp and the sponza stand-in 160 x 90 x 2 spp under trace builds 59 and 44, lean
            (the tc::Fixed kernels), one layer with per-generation launches and through the tail kernel, and a 2-layer
            pass group in 2 frame pieces; a camera with a coordinate exactly on a split plane; all against the oracle.
  queries   rays with axis-parallel directions (zero components of both signs), half of them starting exactly on a
            split plane of a zero axis, against the oracle's or_intersect / or_intersect_shadow.
"""
import json
import subprocess

import numpy as np
import pytest

from helpers import Pair, assert_bitwise
from test_gpu_devmath import PKG, ROOT, product_hipflags, var_hipcc

pytestmark = pytest.mark.gpu

K, SEED = 6, 0xC41A05C0
SIZES = {"cornell": (64, 64, 4), "sponza": (160, 90, 2)}
LEAN_KEYS = ("closest", "shadow", "hit", "texhit", "paths")


# ------------------------------------------------------------------ helpers --
def f32(x):
    return np.asarray(x, np.float32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def below_cases():
    """(oa, split, da) and the reference's below."""
    tiny, dmin = np.float32(2.0 ** -126), np.float32(2.0 ** -149)
    coords = f32([0.0, -0.0, dmin, -dmin, 3 * dmin, tiny, -tiny, tiny + dmin, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)),
                  np.nextafter(np.float32(1), np.float32(0)), 3.14159274, -523.25, 2.0 ** 19, -2.0 ** 19, 3.0e38, -3.0e38,
                  np.nan])
    das = f32([-0.0, 0.0, dmin, -dmin, tiny, -tiny, 2.0 ** -41, -2.0 ** -41, 0.25, -0.25, 1.0, -1.0, 2.0 ** 41, -2.0 ** 41,
               np.inf, -np.inf, np.nan])
    oa, split, da = [a.reshape(-1) for a in np.meshgrid(coords, coords, das, indexing="ij")]
    # nearby pairs all over the exponent range: exact, tiny and denormal differences, and equality
    rng = np.random.default_rng(7)
    n = 2048
    ob = (rng.integers(0, 255, n).astype(np.uint32) << 23) | rng.integers(0, 1 << 23, n).astype(np.uint32) | \
        (rng.integers(0, 2, n).astype(np.uint32) << 31)
    ob = np.where((ob & 0x7fffffff) < 8, ob + 8, ob).astype(np.uint32)
    sb = (ob.astype(np.int64) + rng.integers(-3, 4, n)).astype(np.uint32)
    oa = np.concatenate([oa, ob.view(np.float32)])
    split = np.concatenate([split, sb.view(np.float32)])
    da = np.concatenate([da, das[rng.integers(0, len(das), n)]])
    with np.errstate(invalid="ignore", over="ignore"):
        want = (oa < split) | ((oa == split) & (da <= 0))
        a = split - oa
    facts = {"equal": int((oa == split).sum()), "denormal": int(((a != 0) & (np.abs(a) < tiny)).sum()),
             "both": int(want.sum()), "neither": int((~want).sum())}
    return oa, split, da, want.astype(np.uint32), facts


def div_cases():
    """(a, b) with |a| <= 2^20 and the IEEE quotient; in blocks of 64 whose lanes mix the short path with the
    full division (b outside 2^-40 .. 2^40: a NaN reciprocal; |q0| < 2^-60; a == 0)."""
    rng = np.random.default_rng(11)
    n = 4096
    eb = rng.integers(-40, 40, n)
    b = np.ldexp(1.0 + rng.random(n), eb).astype(np.float32) * rng.choice(f32([-1, 1]), n)
    ea = np.minimum(19, eb + rng.integers(-50, 51, n))
    a = np.ldexp(1.0 + rng.random(n), ea).astype(np.float32) * rng.choice(f32([-1, 1]), n)
    # half next to rounding midpoints of the quotient
    m = np.arange(n) % 2 == 1
    q = np.ldexp(1.0 + rng.random(n), np.minimum(50, 19 - eb) - rng.integers(0, 101, n)).astype(np.float32)
    mid = (q.astype(np.float64) + np.nextafter(q, np.float32(np.inf)).astype(np.float64)) * 0.5
    am = (mid * b.astype(np.float64)).astype(np.float32)
    am = np.where(rng.random(n) < 0.33, np.nextafter(am, np.float32(np.inf)), am)
    am = np.where(rng.random(n) < 0.33, np.nextafter(am, np.float32(-np.inf)), am)
    a = np.where(m & (np.abs(am) <= 2.0 ** 20), am, a).astype(np.float32)
    # the edges of the domain and the lanes that must take the full division
    edge = rng.random(n)
    a = np.where(edge < 0.02, np.copysign(np.float32(2.0 ** 20), a), a)
    a = np.where((edge >= 0.02) & (edge < 0.04), np.float32(0.0) * a, a)                       # +-0
    b = np.where((edge >= 0.04) & (edge < 0.06), np.copysign(np.float32(2.0 ** -40), b), b)
    b = np.where((edge >= 0.06) & (edge < 0.08), np.copysign(np.float32(2.0 ** 40), b), b)
    b = np.where((edge >= 0.08) & (edge < 0.10), b * np.float32(2.0 ** -60), b)                  # NaN reciprocal
    b = np.where((edge >= 0.10) & (edge < 0.11), np.float32(0.0) * b, b)                       # a / +-0
    a = np.where((edge >= 0.11) & (edge < 0.13), a * np.float32(2.0 ** -90), a)                  # |q0| < 2^-60
    # whole waves of each kind too: block 0 all short, block 1 all full division
    a[:64], b[:64] = np.float32(1.5), np.float32(3.0) + np.arange(64, dtype=np.float32)
    b[64:128] = np.float32(2.0 ** -50)
    a, b = a.astype(np.float32), b.astype(np.float32)
    assert (np.abs(a) <= 2.0 ** 20).all()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        want = (a / b).astype(np.float32)
        ok_b = (np.abs(b) >= 2.0 ** -40) & (np.abs(b) <= 2.0 ** 40)
        q0 = np.where(ok_b, a * (np.float32(1) / b), np.float32(np.nan)).astype(np.float32)
        short = np.abs(q0) >= 2.0 ** -60
    assert not (np.abs(q0[ok_b]) > 2.0 ** 60).any()
    per_wave = short.reshape(-1, 64).sum(1)
    facts = {"short": int(short.sum()), "full": int((~short).sum()), "all_short": int((per_wave == 64).sum()),
             "all_full": int((per_wave == 0).sum()), "mixed": int(((per_wave > 0) & (per_wave < 64)).sum())}
    return a, b, want, facts


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    work = tmp_path_factory.mktemp("kdstep")
    exe = work / "kdstep_check"
    subprocess.run([var_hipcc(), *product_hipflags(), "-I", str(PKG / "csrc"), "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "native" / "kdstep_check.hip"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)

    def run(words):
        fin, fout = work / "cases.in", work / "cases.out"
        np.ascontiguousarray(words, np.uint32).tofile(fin)
        r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, "kdstep_check ended with status %d: %s" % (r.returncode, r.stderr[-500:])
        return np.fromfile(fout, np.uint32).reshape(-1, 3), json.loads(r.stdout.strip().splitlines()[-1])

    return run


def test_helpers_known_answers(harness):
    oa, split, da, below, fb = below_cases()
    a, b, quot, fd = div_cases()
    assert fb["equal"] > 500 and fb["denormal"] > 50 and fb["both"] > 1000 and fb["neither"] > 1000, fb
    assert fd["short"] > 2000 and fd["full"] > 300 and fd["all_short"] and fd["all_full"] and fd["mixed"] > 10, fd
    n = max(len(oa), len(a))
    rec = np.zeros((n, 5), np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2] = bits(np.resize(oa, n)), bits(np.resize(split, n)), bits(np.resize(da, n))
    rec[:, 3], rec[:, 4] = bits(np.resize(a, n)), bits(np.resize(b, n))  # (whole blocks of 64 repeat: the waves' mixes stay)
    got, info = harness(rec.reshape(-1))
    assert info["cases"] == n == len(got)
    bad = np.flatnonzero(got[:len(oa), 0] != below)
    assert len(bad) == 0, "kd_below: %d of %d differ, first oa %r split %r da %r: got %d" % (
        len(bad), len(oa), oa[bad[0]], split[bad[0]], da[bad[0]], got[bad[0], 0])
    want = bits(quot)
    for col, name in ((1, "div_by_rcp_wave_bounded"), (2, "div_by_rcp_wave")):
        g = got[:len(a), col]
        same = (g == want) | (np.isnan(g.view(np.float32)) & np.isnan(quot))
        bad = np.flatnonzero(~same)
        assert len(bad) == 0, "%s: %d of %d differ, first a %r b %r: got %08x want %08x" % (
            name, len(bad), len(a), a[bad[0]], b[bad[0]], g[bad[0]], want[bad[0]])


# ------------------------------------------------------------------ renders --
class Case:
    """A scene's Pair and the oracle's frames of its size, each rendered once: layer 1 (with its counters), and
    layers 1 and 2 blended."""

    def __init__(self, ca, po, scenes, name):
        self.name = name
        self.pair = Pair(ca, po, scenes.config_rtc(name))
        self.x, self.y, self.s = SIZES[name]
        self.cam = self.pair.camera(ca, self.x, self.y)
        arr = self.cam.as_array()
        self.ref, self.ref_counters = self.pair.oracle.render(arr, self.x, self.y, self.s, K, SEED)
        self.two = self.ref.copy()
        self.pair.oracle.render(arr, self.x, self.y, self.s, K, SEED, layer=2, pixels=self.two)
        self.ref.setflags(write=False)
        self.two.setflags(write=False)


@pytest.fixture(scope="module")
def cases(ca, po, scenes):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(ca, po, scenes, name)
        return made[name]

    yield get
    made.clear()


def lean(dev, variant, tail_min=0):
    dev.set_option("kernel", 2)
    dev.set_option("variant", variant)
    dev.set_option("counters", 0)
    dev.set_option("wf_tail_min", tail_min)


def restore(dev):
    dev.set_option("variant", -1)
    dev.set_option("counters", 1)
    dev.set_option("wf_tail_min", 0)


@pytest.mark.parametrize("tail_min", [0, 1 << 20], ids=["per_generation", "tail_kernel"])
@pytest.mark.parametrize("variant", [59, 44])
@pytest.mark.parametrize("scene", ["cornell", "sponza"])
def test_one_layer_bitexact(ca, cases, scene, variant, tail_min):
    case = cases(scene)
    dev = case.pair.dev
    lean(dev, variant, tail_min)
    try:
        g = dev.render(case.cam, ca.render_params(case.x, case.y, case.s, K, SEED))
        c, build = dev.counters(), dev.last_trace_build()
    finally:
        restore(dev)
    what = "%s %dx%dx%d build %d %s" % (scene, case.x, case.y, case.s, variant, "tail" if tail_min else "traces")
    assert build == variant, (what, build)
    assert_bitwise(g, case.ref, what)
    assert {k: c[k] for k in LEAN_KEYS} == {k: case.ref_counters[k] for k in LEAN_KEYS}, what


@pytest.mark.parametrize("variant", [59, 44])
@pytest.mark.parametrize("scene", ["cornell", "sponza"])
def test_two_layer_group_in_two_pieces_bitexact(ca, cases, scene, variant):
    import torch
    case = cases(scene)
    dev = case.pair.dev
    x, y, s, nl, pieces = case.x, case.y, case.s, 2, 2
    lean(dev, variant)
    try:
        frame = torch.zeros((y, x, 3), dtype=torch.float32, device="cuda:0")
        for piece in range(pieces):
            q = ca.render_params(x, y, s, K, SEED, layer=1, rank=piece, nranks=pieces)
            dev.render_layers_device(case.cam, q, nl, frame.data_ptr(), 0)
            assert dev.last_trace_build() == variant
        torch.cuda.synchronize()
        g = frame.cpu().numpy()
    finally:
        restore(dev)
    assert_bitwise(g, case.two, "%s %dx%dx%d build %d, 2 layers in 2 pieces" % (scene, x, y, s, variant))


@pytest.mark.parametrize("variant", [59, 44])
@pytest.mark.parametrize("scene", ["cornell", "sponza"])
def test_eye_on_split_bitexact(ca, cases, scene, variant):
    """The eye exactly on a split plane of each axis: split - oa is 0 at that node for every camera ray, so the side
    is decided by the direction's sign alone (kdtree.cpp:267-268)."""
    pair = cases(scene).pair
    e = pair.kd.export()
    lo, hi = np.array(list(pair.desc.box_min)), np.array(list(pair.desc.box_max))
    lean(pair.dev, variant)
    try:
        for axis in range(3):
            inner = np.nonzero((e["is_leaf"] == 0) & (e["axis"] == axis))[0]
            split = np.float32(e["split"][inner[len(inner) // 2]])
            eye = ((lo + hi) / 2).astype(np.float32)
            eye[axis] = split
            look = eye + np.array([0.31, -0.2, 0.93]) * (hi - lo).max()
            cam = ca.camera(eye, look, (0, 1, 0), 1.4, 40, 30)
            assert cam.as_array()[axis] == split
            g = pair.dev.render(cam, ca.render_params(40, 30, 2, K, 77 + axis))
            assert pair.dev.last_trace_build() == variant
            o, _ = pair.oracle.render(cam.as_array(), 40, 30, 2, K, 77 + axis)
            assert_bitwise(g, o, "%s build %d, eye on a split plane of axis %d" % (scene, variant, axis))
    finally:
        restore(pair.dev)


# ------------------------------------------------------------------ queries --
@pytest.mark.parametrize("scene", ["cornell", "sponza"])
def test_axis_parallel_rays_bitexact(cases, scene):
    """Directions with one or two components exactly +0 or -0 (the reference decides `below` by da <= 0 at
    oa == split, and the slab parameters are +-inf or NaN), half of the origins exactly on a split plane of a zero
    axis; closest and shadow queries through the trace kernels."""
    import torch
    pair = cases(scene).pair
    e = pair.oracle.kd_export()
    lo, hi = e["box"][:3], e["box"][3:]
    rng = np.random.default_rng(97)
    n = 2048
    o = (lo + (hi - lo) * rng.random((n, 3), dtype=np.float32)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    zero_axis = rng.integers(0, 3, n)
    d[np.arange(n), zero_axis] = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0))
    second = (zero_axis + 1 + rng.integers(0, 2, n)) % 3  # a quarter: two zero components, a unit axis direction
    quarter = np.arange(n) % 4 == 0
    d[np.arange(n)[quarter], second[quarter]] = np.float32(-0.0)
    d[quarter] = np.where(d[quarter] == 0, d[quarter], np.sign(d[quarter])).astype(np.float32)
    inner = np.nonzero(e["is_leaf"] == 0)[0]
    for j in range(0, n, 2):  # origins exactly on a split plane of the zero axis
        cand = inner[e["axis"][inner] == zero_axis[j]]
        o[j, zero_axis[j]] = e["split"][cand[rng.integers(0, len(cand))]]
    assert (np.signbit(d) & (d == 0)).any() and (~np.signbit(d) & (d == 0)).any()
    ids, _ = pair.oracle.lights()
    light = ids[rng.integers(0, len(ids), n)].astype(np.uint32)
    limit = (rng.random(n) * float(np.linalg.norm(hi - lo))).astype(np.float32)
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    want = pair.oracle.intersect(o, d)
    want_occ = pair.oracle.intersect_shadow(o, d, limit, light)
    assert (want["hit"] == 1).sum() > n // 4 and (want_occ == 1).any() and (want_occ == 0).any()
    dev = "cuda:0"
    t_o, t_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    t_limit, t_light = torch.from_numpy(limit).to(dev), torch.from_numpy(light.view(np.int32)).to(dev)
    hit = torch.zeros((n,), dtype=torch.int32, device=dev)
    tri = torch.zeros((n,), dtype=torch.int32, device=dev)
    bary = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    dist = torch.zeros((n,), dtype=torch.float32, device=dev)
    occ = torch.zeros((n,), dtype=torch.int32, device=dev)
    pair.dev.set_option("query_trace_min", 0)  # the trace kernels, not the per-thread kernel of small batches
    try:
        pair.dev.intersect_device(n, t_o.data_ptr(), t_d.data_ptr(), hit.data_ptr(), tri.data_ptr(), bary.data_ptr(),
                                  dist.data_ptr(), 0)
        pair.dev.intersect_shadow_device(n, t_o.data_ptr(), t_d.data_ptr(), t_limit.data_ptr(), t_light.data_ptr(),
                                         occ.data_ptr(), 0)
        torch.cuda.synchronize()
    finally:
        pair.dev.set_option("query_trace_min", 1 << 16)
    h = want["hit"] == 1
    assert np.array_equal(hit.cpu().numpy().view(np.uint32), want["hit"])
    assert np.array_equal(tri.cpu().numpy().view(np.uint32)[h], want["tri"][h])
    assert np.array_equal(bary.cpu().numpy()[h].view(np.uint32), want["bary"][h].view(np.uint32))
    assert np.array_equal(dist.cpu().numpy()[h].view(np.uint32), want["dist"][h].view(np.uint32))
    assert np.array_equal(occ.cpu().numpy().view(np.uint32), want_occ)
