"""Radiance queries on the GPU (include/chiaro_hip.h "radiance queries"), bit for bit:

1. camera identity: the radiance along a frame's own camera rays is the frame's layer mean (no oracle);
2. ray mode against the oracle: or_path through the degenerate camera [orig, dir, 0, 0] with xres > id, yres 1, x = id,
   whose two jitter draws multiply zero -- every sample, summed and blended as a frame pixel, and its moments;
3. one call against the same rays split over calls with consecutive id0, and over calls of one layer each;
4. the same bits under forced schedules (path cap, sample buffer, tail threshold, queue sort, counting build);
5. the counters against the oracle's;
6. guard bands, untouched inputs, a null moment array, n == 0;
7. gather mode against the oracle: the two aim draws, the integrator's uniform restated in float32, sample_wi, then
   the same degenerate camera;
8. isolation: the ctx's accumulator and temporal history do not see a radiance call;
9. the RayTracer and C API mirrors.

A direction component of -0 would differ from this reference only because its camera ray is d + 0 * ..., which turns
-0 into +0: the directions (and the normals gather mode draws its directions about) have 0.0 added.
References are computed once per (scene, mode, spp, k) over the longest ray set and shared; nothing here changes them."""
import ctypes as C

import numpy as np
import pytest

from helpers import Pair, assert_bitwise

pytestmark = pytest.mark.gpu

SEED, BG = 0xC41A05C0, (0.1, 0.2, 0.3)
F32 = np.float32
POISON = 0x7FC0DEAD  # a NaN payload: any write shows
NMAX = {"cornell": 1025, "nanobox": 257, "sponza": 257}
OUTSIDE = 16  # origins outside the scene box, aimed away from it: rays 1, 3, .. 31

_PAIRS, _RAYS, _REF = {}, {}, {}


@pytest.fixture(scope="module")
def pairs(ca, po, scenes):
    def get(name):
        if name not in _PAIRS:
            _PAIRS[name] = Pair(ca, po, scenes.config_rtc(name))
        return _PAIRS[name]
    yield get
    for p in _PAIRS.values():
        p.dev.close()
    _PAIRS.clear()


def box_of(pair):
    b = pair.oracle.kd_export()["box"].astype(np.float64)
    return b[:3], b[3:]


def rays_of(pair, name):
    """(orig, dirs) [NMAX][3] float32: origins uniform in the scene box shrunk by 5 %, normal-distributed directions;
    rays 1, 3, .. 31 start outside the box and point away from its centre (misses)."""
    if name not in _RAYS:
        n = NMAX[name]
        rng = np.random.default_rng(20240607)
        lo, hi = box_of(pair)
        c, h = (lo + hi) / 2, (hi - lo) / 2
        orig = c + h * 0.95 * rng.uniform(-1, 1, (n, 3))
        dirs = rng.normal(size=(n, 3))
        for j in range(OUTSIDE):
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            o = c + u * np.linalg.norm(h) * rng.uniform(1.2, 3.0)
            orig[1 + 2 * j], dirs[1 + 2 * j] = o, (o - c) * rng.uniform(0.1, 4.0)
        _RAYS[name] = (orig.astype(F32), (dirs.astype(F32) + F32(0.0)).astype(F32))
    return _RAYS[name]


def degenerate_camera(o, d):
    return np.concatenate([o, d, np.zeros(6, F32)]).astype(F32)


def uniform_f32(u, a, b):
    """rng_uniform on a raw draw, restated in float32: the conversion and division, the guard, the scale."""
    c = F32(np.uint32(u)) / F32(4294967296.0)
    if c >= F32(1.0):
        c = F32(float.fromhex("0x1.fffffep-1"))
    return F32(c * (F32(b) - F32(a)) + F32(a))


def ray_samples(pair, orig, dirs, ids, spp, k, layers):
    """[layers][n][spp][3]: or_path of every sample of ray (orig, dir) on stream id, layers 1 .. layers."""
    out = np.zeros((layers, len(ids), spp, 3), F32)
    for i, j in enumerate(ids):
        cam = degenerate_camera(orig[i], dirs[i])
        for L in range(1, layers + 1):
            for s in range(spp):
                out[L - 1, i, s] = pair.oracle.path(cam, int(j) + 1, 1, k, BG, SEED, L, int(j), 0, s)
    return out


def gather_samples(po, pair, pos, nrm, ids, spp, k, layers):
    out = np.zeros((layers, len(ids), spp, 3), F32)
    for i, j in enumerate(ids):
        for L in range(1, layers + 1):
            for s in range(spp):
                u = po.rng_draws(SEED, L, int(j), s, 2)
                wi, _ = po.sample_wi(nrm[i], uniform_f32(u[0], -1, 1), uniform_f32(u[1], -1, 1))
                cam = degenerate_camera(pos[i], wi)
                out[L - 1, i, s] = pair.oracle.path(cam, int(j) + 1, 1, k, BG, SEED, L, int(j), 0, s)
    return out


def fold(samples, first_layer=1, out=None, m2=None):
    """The frame arithmetic over [layers][n][spp][3] samples: (out, m2) after the last layer."""
    nl, n, spp, _ = samples.shape
    out = np.zeros((n, 3), F32) if out is None else out.copy()
    m2 = np.zeros((n, 3), F32) if m2 is None else m2.copy()
    inv = F32(1.0) / F32(spp)
    for j in range(nl):
        L = first_layer + j
        t, q = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
        for s in range(spp):
            r = samples[j, :, s]
            t = t + r
            q = q + r * r
        out = (out * F32(L - 1) + t * inv) / F32(L)
        m2 = (m2 * F32(L - 1) + q * inv) / F32(L)
    return out, m2


def ray_ref(pairs, name, spp, k, layers=3):
    key = (name, "ray", spp, k)
    if key not in _REF:
        pair = pairs(name)
        orig, dirs = rays_of(pair, name)
        _REF[key] = ray_samples(pair, orig, dirs, np.arange(NMAX[name]), spp, k, layers)
    return _REF[key]


class Guarded:
    """A device array [n][3] between two poisoned guard bands."""

    def __init__(self, n, guard=4096, init=None):
        import torch
        self.n, self.g = 3 * n, guard
        self.t = torch.full((self.n + 2 * guard,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        self.body = self.t[guard:guard + self.n].view(n, 3)
        if init is not None:
            self.body.copy_(torch.from_numpy(np.ascontiguousarray(init, F32)))
        self.ptr = self.body.data_ptr() if n else 0

    def numpy(self):
        return self.body.cpu().numpy()

    def assert_guards(self, what):
        import torch
        bits = self.t.view(torch.int32).cpu().numpy()
        assert (bits[:self.g] == POISON).all() and (bits[self.g + self.n:] == POISON).all(), what + ": guard band"


def run(ca, dev, a, b, spp, k, nlayers=1, layer=1, id0=0, gather=False, m2=True, out0=None, m20=None):
    """One device call over the rays (a, b) -> (out, m2 or None) as numpy, guard bands and inputs checked."""
    import torch
    n = len(a)
    da, db = torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()
    o, m = Guarded(n, init=out0), Guarded(n, init=m20) if m2 else None
    rp = ca.radiance_params(spp, k, SEED, BG, layer=layer, id0=id0)
    fn = dev.gather_device if gather else dev.radiance_device
    fn(n, da.data_ptr(), db.data_ptr(), rp, nlayers, o.ptr, m.ptr if m2 else 0, 0)
    torch.cuda.synchronize()
    o.assert_guards("out")
    if m2:
        m.assert_guards("m2")
    assert np.array_equal(da.cpu().numpy().view(np.uint32), np.ascontiguousarray(a).view(np.uint32)), "inputs changed"
    assert np.array_equal(db.cpu().numpy().view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), "inputs changed"
    return o.numpy(), (m.numpy() if m2 else None)


# --- 1. camera identity ------------------------------------------------------------------------------------

@pytest.mark.parametrize("layer", [1, 3])
def test_camera_identity(ca, po, pairs, layer):
    import torch
    pair = pairs("cornell")
    x, y, spp, k = 16, 12, 1, 6
    cam = pair.camera(ca, x, y)
    c = cam.as_array()
    eye, lu, dx, dy = c[0:3], c[3:6], c[6:9], c[9:12]
    orig, dirs = np.zeros((x * y, 3), F32), np.zeros((x * y, 3), F32)
    for py in range(y):
        for px in range(x):
            u = po.rng_draws(SEED, layer, py * x + px, 0, 2)
            uy, ux = uniform_f32(u[0], 0, 1), uniform_f32(u[1], 0, 1)  # (the y jitter is drawn first)
            sx, sy = F32(px) + ux, F32(py) + uy
            orig[py * x + px] = eye
            dirs[py * x + px] = (lu + dx * sx) + dy * sy
    # the frame's layer mean: the tile means of that layer (one 32 x 32 tile holds the frame)
    tiles = torch.zeros((32, 32, 3), dtype=torch.float32, device="cuda")
    p = ca.render_params(x, y, spp, k, SEED, layer=layer, background=BG)
    pair.dev.render_tiles_device(cam, p, tiles.data_ptr(), 0)
    torch.cuda.synchronize()
    mean = tiles.cpu().numpy()[:y, :x]
    got, _ = run(ca, pair.dev, orig, dirs, spp, k, 1, layer=layer, m2=False, out0=np.zeros((x * y, 3), F32))
    # (layer L over an old value of zero: (0 * (L - 1) + mean) / L)
    want = (np.zeros_like(mean) * F32(layer - 1) + mean) / F32(layer)
    assert float(mean.sum()) > 0
    assert_bitwise(got.reshape(y, x, 3), want, "radiance along the camera rays of layer %d" % layer)


# --- 2. oracle parity, ray mode ----------------------------------------------------------------------------

def test_ray_sets_hit_and_miss(pairs):
    for name in ("cornell", "nanobox"):
        pair = pairs(name)
        orig, dirs = rays_of(pair, name)
        for n in (63, NMAX[name]):
            hit = pair.oracle.intersect(orig[:n], dirs[:n])["hit"]
            assert int(hit.sum()) >= 10 and int((hit == 0).sum()) >= 10, (name, n, int(hit.sum()))
        assert not pair.oracle.intersect(orig[1:2 * OUTSIDE:2], dirs[1:2 * OUTSIDE:2])["hit"].any()
        lo, hi = box_of(pair)
        outside = ((orig < lo) | (orig > hi)).any(axis=1)
        assert outside[1:2 * OUTSIDE:2].all() and int(outside.sum()) == OUTSIDE


@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("spp", [1, 5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_ray_mode_cornell(ca, pairs, n, spp, k):
    pair = pairs("cornell")
    orig, dirs = rays_of(pair, "cornell")
    want = fold(ray_ref(pairs, "cornell", spp, k)[:, :n])
    out, m2 = run(ca, pair.dev, orig[:n], dirs[:n], spp, k, 3)
    assert_bitwise(out, want[0], "radiance n %d spp %d k %d" % (n, spp, k))
    assert_bitwise(m2, want[1], "moments n %d spp %d k %d" % (n, spp, k))


@pytest.mark.parametrize("spp,k", [(1, 1), (5, 6)])
def test_ray_mode_nanobox(ca, pairs, spp, k):
    pair = pairs("nanobox")
    n = 257
    orig, dirs = rays_of(pair, "nanobox")
    want = fold(ray_ref(pairs, "nanobox", spp, k))
    out, m2 = run(ca, pair.dev, orig, dirs, spp, k, 3)
    assert pair.dev.counters()["texhit"] > 0
    assert_bitwise(out, want[0], "nanobox radiance n %d spp %d k %d" % (n, spp, k))
    assert_bitwise(m2, want[1], "nanobox moments n %d spp %d k %d" % (n, spp, k))


def test_large_scene_default_build(ca, po, pairs):
    """The sponza stand-in (>= 65,536 triangles) on the lean default build 59: the first rays -- origins outside the
    scene box among them -- on the closest kernel without a leaf cull, every later generation on the build's own
    leaf-cull kernels with sorted, leaf-keyed queues; ray mode and gather mode."""
    pair = pairs("sponza")
    assert pair.dev.scene_triangles() >= 65536
    n, spp, k, layers = 257, 4, 6, 2
    orig, dirs = rays_of(pair, "sponza")
    pos, nrm = gather_points(pair, "sponza")
    want = fold(ray_ref(pairs, "sponza", spp, k, layers))
    want_g = fold(gather_samples(po, pair, pos, nrm, np.arange(n), spp, k, layers))
    pair.dev.set_option("counters", 0)
    pair.dev.set_option("wf_sort_min", 16)
    try:
        out, m2 = run(ca, pair.dev, orig, dirs, spp, k, layers)
        build = pair.dev.last_trace_build()
        out_g, m2_g = run(ca, pair.dev, pos, nrm, spp, k, layers, gather=True)
    finally:
        pair.dev.set_option("wf_sort_min", 1 << 16)
        pair.dev.set_option("counters", 1)
    assert build == 59
    assert_bitwise(out, want[0], "sponza stand-in, build 59")
    assert_bitwise(m2, want[1], "sponza stand-in, build 59, moments")
    assert_bitwise(out_g, want_g[0], "sponza stand-in, build 59, gather")
    assert_bitwise(m2_g, want_g[1], "sponza stand-in, build 59, gather moments")


# --- 3. split and id invariance ----------------------------------------------------------------------------

def test_split_and_id_invariance(ca, pairs):
    pair = pairs("cornell")
    n, spp, k = 257, 5, 6
    orig, dirs = (a[:n] for a in rays_of(pair, "cornell"))
    whole = run(ca, pair.dev, orig, dirs, spp, k, 3)
    assert_bitwise(whole[0], fold(ray_ref(pairs, "cornell", spp, k)[:, :n])[0], "one call")
    a = run(ca, pair.dev, orig[:100], dirs[:100], spp, k, 3, id0=0)
    b = run(ca, pair.dev, orig[100:], dirs[100:], spp, k, 3, id0=100)
    for i in (0, 1):
        assert_bitwise(np.concatenate([a[i], b[i]]), whole[i], "calls of 100 and 157 rays, id0 0 and 100")
    # other ids are other streams
    other = run(ca, pair.dev, orig[100:], dirs[100:], spp, k, 3, id0=0)
    assert (other[0].view(np.uint32) != b[0].view(np.uint32)).any()
    # layers 1..3 in one call against three calls of one layer each
    out, m2 = None, None
    for layer in (1, 2, 3):
        out, m2 = run(ca, pair.dev, orig, dirs, spp, k, 1, layer=layer, out0=out, m20=m2)
    assert_bitwise(out, whole[0], "three calls of one layer")
    assert_bitwise(m2, whole[1], "three calls of one layer, moments")


# --- 4. forced schedules -----------------------------------------------------------------------------------

SCHEDULES = [("wf_paths", 4096, 256 << 20), ("sample_buf_bytes", 1024 * 12 * 8, 4 << 30), ("wf_tail_min", 1 << 20, 0),
             ("wf_tail_min", 0, 0), ("wf_sort_min", 16, 1 << 16), ("counters", 0, 1), ("counters", 1, 1)]


@pytest.mark.parametrize("name", ["cornell", "nanobox"])
@pytest.mark.parametrize("option,value,restore", SCHEDULES)
def test_forced_schedules(ca, pairs, name, option, value, restore):
    pair = pairs(name)
    n, spp, k = 257, 5, 6
    orig, dirs = (a[:n] for a in rays_of(pair, name))
    want = fold(ray_ref(pairs, name, spp, k)[:, :n])
    pair.dev.set_option(option, value)
    if option == "wf_sort_min":
        pair.dev.set_option("counters", 0)  # (the lean build sorts its queues)
    try:
        out, m2 = run(ca, pair.dev, orig, dirs, spp, k, 3)
        paths = pair.dev.counters()["paths"]
    finally:
        pair.dev.set_option(option, restore)
        pair.dev.set_option("counters", 1)
    assert paths == n * spp * 3
    assert_bitwise(out, want[0], "%s %s = %d" % (name, option, value))
    assert_bitwise(m2, want[1], "%s %s = %d, moments" % (name, option, value))


# --- 5. counters -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cornell", "nanobox"])
def test_counters(ca, pairs, name):
    pair = pairs(name)
    n, spp, k = 257, 5, 6
    orig, dirs = (a[:n] for a in rays_of(pair, name))
    names = ("closest", "shadow", "hit", "texhit", "paths")
    want = dict.fromkeys(names, 0)
    means = np.zeros((n, 3), F32)
    for i in range(n):
        mean, oc = pair.oracle.render_pixels(degenerate_camera(orig[i], dirs[i]), i + 1, 1, spp, k, SEED, [i], [0],
                                             layer=1, bg=BG)
        means[i] = mean[0]
        for key in names:
            want[key] += oc[key]
    pair.dev.set_option("counters", 1)
    out, _ = run(ca, pair.dev, orig, dirs, spp, k, 1)
    gc = pair.dev.counters()
    assert_bitwise(out, means, "or_render_pixels")
    assert_bitwise(out, fold(ray_ref(pairs, name, spp, k)[:1, :n])[0], "or_path")
    assert {key: gc[key] for key in names} == want
    assert want["paths"] == n * spp and want["closest"] >= want["paths"] and want["hit"] > 0
    assert gc["nee_answered"] <= gc["shadow"]
    assert pair.dev.last_kernel_ms() > 0
    ts = pair.dev.trace_stats()
    assert ts["camera"]["launches"] == 0 and ts["closest"]["launches"] >= 1  # (no camera trace: the general closest)


# --- 6. guard bands, null moments, no rays -----------------------------------------------------------------

def test_null_moments_and_no_rays(ca, pairs):
    import torch
    pair = pairs("cornell")
    n, spp, k = 65, 5, 6
    orig, dirs = (a[:n] for a in rays_of(pair, "cornell"))
    want = fold(ray_ref(pairs, "cornell", spp, k)[:, :n])
    out, none = run(ca, pair.dev, orig, dirs, spp, k, 3, m2=False)
    assert none is None
    assert_bitwise(out, want[0], "no moment array")
    before = pair.dev.counters()
    assert before["paths"] == n * spp * 3
    rp = ca.radiance_params(spp, k, SEED, BG)
    t = torch.zeros(3, dtype=torch.float32, device="cuda")
    pair.dev.radiance_device(0, 0, 0, rp, 3, 0, 0, 0)
    pair.dev.gather_device(0, t.data_ptr(), t.data_ptr(), rp, 3, t.data_ptr(), 0, 0)
    assert pair.dev.counters() == before  # nothing launched: the last call's counters are still there
    assert len(pair.dev.radiance(np.zeros((0, 3), F32), np.zeros((0, 3), F32), rp, 3)) == 0
    assert pair.dev.counters() == before


def test_invalid_arguments_on_a_device(ca, pairs):
    pair = pairs("cornell")
    hip = ca.libs()[0]
    import torch
    t = torch.zeros(12, dtype=torch.float32, device="cuda")
    P = C.c_void_p
    for kw in (dict(spp=0), dict(k=0), dict(k=65), dict(layer=0), dict(id0=0xffffffff)):
        args = dict(spp=2, k=3, layer=1, id0=0)
        args.update(kw)
        rp = ca.radiance_params(args["spp"], args["k"], SEED, BG, layer=args["layer"], id0=args["id0"])
        rc = hip.cr_radiance_device(pair.dev._c, 4, P(t.data_ptr()), P(t.data_ptr()), C.byref(rp), 1, P(t.data_ptr()),
                                    None, None)
        assert ca.CR_ERRORS.get(rc) == "CR_E_INVALID", kw
    bare = ca.Device(0)  # no scene
    try:
        rp = ca.radiance_params(2, 3, SEED, BG)
        rc = hip.cr_gather_device(bare._c, 4, P(t.data_ptr()), P(t.data_ptr()), C.byref(rp), 1, P(t.data_ptr()), None,
                                  None)
        assert ca.CR_ERRORS.get(rc) == "CR_E_NOSCENE"
    finally:
        bare.close()


# --- 7. gather parity --------------------------------------------------------------------------------------

def gather_points(pair, name):
    """(pos, nrm): the first hits of NMAX random rays from inside the box, the normal towards the ray's side, the
    point 0.001 normal off the surface (float32)."""
    key = (name, "points")
    if key not in _RAYS:
        rng = np.random.default_rng(7)
        lo, hi = box_of(pair)
        c, h = (lo + hi) / 2, (hi - lo) / 2
        o = (c + h * 0.9 * rng.uniform(-1, 1, (4 * 257, 3))).astype(F32)
        d = rng.normal(size=o.shape).astype(F32)
        q = pair.oracle.intersect(o, d)
        sel = np.flatnonzero(q["hit"])[:257]
        assert len(sel) == 257
        tris = pair.tris["pos"].reshape(-1, 3, 3).astype(F32)[q["tri"][sel]]
        bx, by = q["bary"][sel, 0:1], q["bary"][sel, 1:2]
        pos = (tris[:, 0] * (F32(1) - bx - by) + tris[:, 1] * bx + tris[:, 2] * by).astype(F32)
        nrm = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]).astype(F32)
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
        flip = (nrm * d[sel]).sum(axis=1) > 0
        nrm[flip] = -nrm[flip]
        nrm = (nrm + F32(0.0)).astype(F32)
        pos = (pos + F32(0.001) * nrm).astype(F32)
        _RAYS[key] = (pos, nrm)
    return _RAYS[key]


@pytest.mark.parametrize("name", ["cornell", "nanobox"])
def test_gather(ca, po, pairs, name):
    pair = pairs(name)
    n, spp, k, layers = 257, 4, 6, 2
    pos, nrm = gather_points(pair, name)
    key = (name, "gather", spp, k)
    if key not in _REF:
        _REF[key] = gather_samples(po, pair, pos, nrm, np.arange(n), spp, k, layers)
    want = fold(_REF[key])
    out, m2 = run(ca, pair.dev, pos, nrm, spp, k, layers, gather=True)
    assert_bitwise(out, want[0], name + " gather")
    assert_bitwise(m2, want[1], name + " gather moments")
    if name == "cornell":
        assert float(out.sum()) > 0  # (a guard against a dead light sampler, not a measurement)
    # the ids: the second half alone, on its own streams
    h = n // 2
    part, _ = run(ca, pair.dev, pos[h:], nrm[h:], spp, k, layers, id0=h, gather=True)
    assert_bitwise(part, want[0][h:], name + " gather from id0 %d" % h)


# --- 8. isolation ------------------------------------------------------------------------------------------

def test_isolation(ca, pairs):
    pair = pairs("cornell")
    dev = pair.dev
    x, y, spp, k = 16, 12, 2, 6
    cam = pair.camera(ca, x, y)
    orig, dirs = (a[:65] for a in rays_of(pair, "cornell"))
    want = None
    frames = []
    for layer in (1, 2, 3):
        want, _ = pair.oracle.render(cam.as_array(), x, y, spp, k, SEED, layer=layer, bg=BG,
                                     pixels=None if want is None else want.copy())
        frames.append(want)
    p = lambda layer: ca.render_params(x, y, spp, k, SEED, layer=layer, background=BG)
    dev.render(cam, p(1))
    got2 = dev.render(cam, p(2))
    run(ca, dev, orig, dirs, 5, k, 2)
    got3 = dev.render(cam, p(3))
    assert_bitwise(got2, frames[1], "two plain layers")
    assert_bitwise(got3, frames[2], "layers 1..2, a radiance call, then layer 3")
    # the temporal history
    dev.render_temporal(cam, p(1), 1)
    before = dev.temporal_history(x, y)
    run(ca, dev, orig, dirs, 5, k, 2)
    run(ca, dev, orig, dirs, 5, k, 1, gather=True)
    after = dev.temporal_history(x, y)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "temporal history changed"
    dev.render(cam, p(1))
    run(ca, dev, orig, dirs, 5, k, 1, gather=True)
    assert_bitwise(dev.render(cam, p(2)), frames[1], "layer 1, a gather call, then layer 2")


# --- 9. mirrors --------------------------------------------------------------------------------------------

def test_mirrors(ca, pairs, scenes):
    pair = pairs("cornell")
    n, layers = 65, 2
    orig, dirs = (a[:n] for a in rays_of(pair, "cornell"))
    pos, nrm = (a[:n] for a in gather_points(pair, "cornell"))
    scene = ca.Scene(scenes.config_rtc("cornell"), "samples", "3")
    i = scene.info
    spp, k, bg = i["samples"], i["k"], tuple(i["background"])
    assert (spp, i["seed"]) == (3, SEED)
    rp = ca.radiance_params(spp, k, SEED, bg)
    import torch
    want = []
    for a, b, fn in ((orig, dirs, pair.dev.radiance_device), (pos, nrm, pair.dev.gather_device)):
        da, db = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
        o = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        fn(n, da.data_ptr(), db.data_ptr(), rp, layers, o.data_ptr(), 0, 0)
        want.append(o.cpu().numpy())
    assert float(want[0].sum()) > 0 and float(want[1].sum()) > 0
    # the host forms of the C-ABI
    assert_bitwise(pair.dev.radiance(orig, dirs, rp, layers), want[0], "cr_radiance")
    assert_bitwise(pair.dev.gather(pos, nrm, rp, layers), want[1], "cr_gather")
    # RayTracer and the C API under it
    rt = ca.RayTracer(ca.Model(scene), scene)
    assert_bitwise(rt.radiance(orig, dirs, layers), want[0], "RayTracer.radiance")
    assert_bitwise(rt.gather(pos, nrm, layers), want[1], "RayTracer.gather")
    assert rt.counters()["paths"] == n * spp * layers
    host = ca.libs()[1]
    FP = C.POINTER(C.c_float)
    out = np.zeros((n, 3), F32)
    for fn, a, b, w in ((host.chiaro_raytracer_radiance, orig, dirs, want[0]), (host.chiaro_raytracer_gather, pos, nrm, want[1])):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert fn(rt._h, a.ctypes.data_as(FP), b.ctypes.data_as(FP), n, layers, out.ctypes.data_as(FP)) == 0
        assert_bitwise(out, w, fn.__name__)
    assert host.chiaro_raytracer_radiance(rt._h, None, None, n, layers, out.ctypes.data_as(FP)) == -1
    assert host.chiaro_raytracer_gather(rt._h, a.ctypes.data_as(FP), b.ctypes.data_as(FP), n, 0,
                                        out.ctypes.data_as(FP)) == -1
