"""SH irradiance probes on the GPU (include/chiaro_hip.h "probes"), bit for bit:

1. sphere identity: with spp 1 and layer 1, sh[i][k][c] is Y_k(d) times what cr_radiance_device returns for (pos_i, d)
   on the same stream, d from the model (no oracle);
2. oracle parity: or_path of every sample through the degenerate camera [pos, d + 0.0, 0, 0], folded by the model,
   with and without the moment array;
3. one call against the same probes split over calls with consecutive id0, and over calls of one layer each;
4. the same bits under forced schedules (path cap, a sample buffer so small that the 27 running sums cross sample
   chunks, tail threshold, queue sort, counting build);
5. one case on the sponza stand-in with the lean default build;
6. guard bands around every output, untouched inputs, a null moment array, n == 0;
7. cr_probe_eval_device and cr_probe_sample_device against the model;
8. isolation: frame layers rendered around a probe call are the oracle's, the temporal history and a bake keep
   their bits;
9. the host forms, RayTracer.bakeProbes / sampleProbes and the C API give the device calls' bits.

References are computed once per (scene, spp, k) over the longest probe set and shared; nothing here changes them."""
import ctypes as C

import numpy as np
import pytest

import probe_model as pm
from helpers import Pair, assert_bitwise

pytestmark = pytest.mark.gpu

SEED, BG = 0xC41A05C0, (0.1, 0.2, 0.3)
F32 = np.float32
POISON = 0x7FC0DEAD  # a NaN payload: any write shows
NMAX = {"cornell": 257, "nanobox": 65, "sponza": 65}
LAYERS = 3
GRIDS = [((0.25, -1.0, 2.0), (1.0, 1.0, 1.0), (1, 1, 1)), ((-1.5, 0.5, 0.0), (0.75, 3.0, 0.3), (2, 1, 3)),
         ((0.1, -0.2, 0.3), (0.37, 0.5, 1.25), (4, 3, 2))]

_PAIRS, _POS, _REF = {}, {}, {}


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


def probes_of(pair, name):
    """[NMAX][3] float32: positions uniform in the scene box shrunk by 5 %."""
    if name not in _POS:
        b = pair.oracle.kd_export()["box"].astype(np.float64)
        c, h = (b[:3] + b[3:]) / 2, (b[3:] - b[:3]) / 2
        rng = np.random.default_rng(20241021)
        _POS[name] = (c + h * 0.95 * rng.uniform(-1, 1, (NMAX[name], 3))).astype(F32)
    return _POS[name]


def sample_dirs(po, ids, spp, layers, first_layer=1):
    """[layers][n][spp][3]: the model's direction of every sample of streams ids."""
    raw = np.zeros((layers, len(ids), spp, 2), np.uint32)
    for j in range(layers):
        for i, pid in enumerate(ids):
            for s in range(spp):
                raw[j, i, s] = po.rng_draws(SEED, first_layer + j, int(pid), s, 2)
    return pm.direction(raw[..., 0], raw[..., 1])


def probe_ref(po, pairs, name, spp, k, layers=LAYERS):
    """(dirs, rad) [layers][NMAX][spp][3]: each sample's direction and the oracle's radiance along it."""
    key = (name, spp, k, layers)
    if key not in _REF:
        pair = pairs(name)
        pos = probes_of(pair, name)
        n = len(pos)
        dirs = sample_dirs(po, np.arange(n), spp, layers)
        rad = np.zeros((layers, n, spp, 3), F32)
        for j in range(layers):
            for i in range(n):
                for s in range(spp):
                    cam = np.concatenate([pos[i], dirs[j, i, s] + F32(0.0), np.zeros(6, F32)]).astype(F32)
                    rad[j, i, s] = pair.oracle.path(cam, i + 1, 1, k, BG, SEED, j + 1, i, 0, s)
        _REF[key] = (dirs, rad)
    return _REF[key]


def want_of(po, pairs, name, spp, k, n, layers=LAYERS):
    dirs, rad = probe_ref(po, pairs, name, spp, k, layers)
    return pm.fold(dirs[:, :n], rad[:, :n])


class Guarded:
    """A device array of `count` floats between two poisoned guard bands."""

    def __init__(self, count, guard=4096, init=None):
        import torch
        self.n, self.g = count, guard
        self.t = torch.full((count + 2 * guard,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        self.body = self.t[guard:guard + count]
        if init is not None:
            self.body.copy_(torch.from_numpy(np.ascontiguousarray(init, F32).ravel()))
        self.ptr = self.body.data_ptr() if count else 0

    def numpy(self):
        return self.body.cpu().numpy()

    def assert_guards(self, what):
        import torch
        bits = self.t.view(torch.int32).cpu().numpy()
        assert (bits[:self.g] == POISON).all() and (bits[self.g + self.n:] == POISON).all(), what + ": guard band"


def run(ca, dev, pos, spp, k, nlayers=1, layer=1, id0=0, m2=True, sh0=None, m20=None):
    """One cr_probe_sh_device call -> (sh, m2 or None) [n][9][3], guard bands and inputs checked."""
    import torch
    n = len(pos)
    dp = torch.from_numpy(np.ascontiguousarray(pos)).cuda()
    o, m = Guarded(27 * n, init=sh0), Guarded(27 * n, init=m20) if m2 else None
    rp = ca.radiance_params(spp, k, SEED, BG, layer=layer, id0=id0)
    dev.probe_sh_device(n, dp.data_ptr(), rp, nlayers, o.ptr, m.ptr if m2 else 0, 0)
    torch.cuda.synchronize()
    o.assert_guards("sh")
    if m2:
        m.assert_guards("m2")
    assert np.array_equal(dp.cpu().numpy().view(np.uint32), np.ascontiguousarray(pos).view(np.uint32)), "inputs changed"
    return o.numpy().reshape(n, 9, 3), (m.numpy().reshape(n, 9, 3) if m2 else None)


# --- 1. sphere identity ------------------------------------------------------------------------------------

def test_sphere_identity(ca, po, pairs):
    import torch
    pair = pairs("cornell")
    n, k, id0 = 257, 6, 40
    pos = probes_of(pair, "cornell")[:n]
    dirs = sample_dirs(po, id0 + np.arange(n), 1, 1)  # [1][n][1][3]
    d = np.ascontiguousarray(dirs[0, :, 0])
    dp, dd = torch.from_numpy(pos.copy()).cuda(), torch.from_numpy(d).cuda()
    out = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    rp = ca.radiance_params(1, k, SEED, BG, layer=1, id0=id0)
    pair.dev.radiance_device(n, dp.data_ptr(), dd.data_ptr(), rp, 1, out.data_ptr(), 0, 0)
    rad = out.cpu().numpy()
    assert float(rad.sum()) > 0
    want, want2 = pm.fold(dirs, rad[None, :, None, :])
    sh, m2 = run(ca, pair.dev, pos, 1, k, 1, id0=id0)
    assert_bitwise(sh, want, "sh = Y(d) * radiance along d")
    assert_bitwise(m2, want2, "moments = (Y(d) * radiance along d)^2")
    assert_bitwise(sh[:, 0], (pm.K0 * rad).astype(F32) + F32(0), "the constant coefficient")


# --- 2. oracle parity --------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("spp", [1, 5, 16])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_oracle_parity_cornell(ca, po, pairs, n, spp, k):
    pair = pairs("cornell")
    pos = probes_of(pair, "cornell")[:n]
    want = want_of(po, pairs, "cornell", spp, k, n)
    sh, m2 = run(ca, pair.dev, pos, spp, k, LAYERS)
    assert pair.dev.counters()["paths"] == n * spp * LAYERS
    assert_bitwise(sh, want[0], "sh n %d spp %d k %d" % (n, spp, k))
    assert_bitwise(m2, want[1], "moments n %d spp %d k %d" % (n, spp, k))
    alone, none = run(ca, pair.dev, pos, spp, k, LAYERS, m2=False)
    assert none is None
    assert_bitwise(alone, want[0], "sh without moments n %d spp %d k %d" % (n, spp, k))
    if n == 257:
        assert float(np.abs(sh).sum()) > 0 and float(sh[:, 0].min()) >= 0


@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("spp", [1, 5, 16])
def test_oracle_parity_nanobox(ca, po, pairs, spp, k):
    pair = pairs("nanobox")
    n = NMAX["nanobox"]
    pos = probes_of(pair, "nanobox")
    want = want_of(po, pairs, "nanobox", spp, k, n)
    sh, m2 = run(ca, pair.dev, pos, spp, k, LAYERS)
    assert_bitwise(sh, want[0], "nanobox sh spp %d k %d" % (spp, k))
    assert_bitwise(m2, want[1], "nanobox moments spp %d k %d" % (spp, k))
    alone, _ = run(ca, pair.dev, pos, spp, k, LAYERS, m2=False)
    assert_bitwise(alone, want[0], "nanobox sh without moments spp %d k %d" % (spp, k))


# --- 3. split and id invariance ----------------------------------------------------------------------------

def test_split_and_id_invariance(ca, po, pairs):
    pair = pairs("cornell")
    n, spp, k = 257, 5, 6
    pos = probes_of(pair, "cornell")
    whole = run(ca, pair.dev, pos, spp, k, LAYERS)
    assert_bitwise(whole[0], want_of(po, pairs, "cornell", spp, k, n)[0], "one call")
    a = run(ca, pair.dev, pos[:100], spp, k, LAYERS, id0=0)
    b = run(ca, pair.dev, pos[100:], spp, k, LAYERS, id0=100)
    for i in (0, 1):
        assert_bitwise(np.concatenate([a[i], b[i]]), whole[i], "calls of 100 and 157 probes, id0 0 and 100")
    other = run(ca, pair.dev, pos[100:], spp, k, LAYERS, id0=0)  # other ids are other streams
    assert (other[0].view(np.uint32) != b[0].view(np.uint32)).any()
    sh, m2 = None, None
    for layer in (1, 2, 3):
        sh, m2 = run(ca, pair.dev, pos, spp, k, 1, layer=layer, sh0=sh, m20=m2)
    assert_bitwise(sh, whole[0], "three calls of one layer")
    assert_bitwise(m2, whole[1], "three calls of one layer, moments")


# --- 4. forced schedules -----------------------------------------------------------------------------------

# (1024 work items x 8 samples of 12 bytes: a pass of 16 samples is summed in two chunks)
SCHEDULES = [("wf_paths", 4096, 256 << 20), ("sample_buf_bytes", 1024 * 12 * 8, 4 << 30), ("wf_tail_min", 1 << 20, 0),
             ("wf_tail_min", 0, 0), ("wf_sort_min", 16, 1 << 16), ("counters", 0, 1), ("counters", 1, 1)]


@pytest.mark.parametrize("name", ["cornell", "nanobox"])
@pytest.mark.parametrize("option,value,restore", SCHEDULES)
def test_forced_schedules(ca, po, pairs, name, option, value, restore):
    pair = pairs(name)
    n, spp, k = NMAX[name], 16, 6
    pos = probes_of(pair, name)
    want = want_of(po, pairs, name, spp, k, n)
    pair.dev.set_option(option, value)
    if option == "wf_sort_min":
        pair.dev.set_option("counters", 0)  # (the lean build sorts its queues)
    try:
        sh, m2 = run(ca, pair.dev, pos, spp, k, LAYERS)
        paths = pair.dev.counters()["paths"]
        alone, _ = run(ca, pair.dev, pos, spp, k, LAYERS, m2=False)
    finally:
        pair.dev.set_option(option, restore)
        pair.dev.set_option("counters", 1)
    assert paths == n * spp * LAYERS
    assert_bitwise(sh, want[0], "%s %s = %d" % (name, option, value))
    assert_bitwise(m2, want[1], "%s %s = %d, moments" % (name, option, value))
    assert_bitwise(alone, want[0], "%s %s = %d, without moments" % (name, option, value))


# --- 5. the sponza stand-in on the lean default build ------------------------------------------------------

def test_large_scene_default_build(ca, po, pairs):
    pair = pairs("sponza")
    assert pair.dev.scene_triangles() >= 65536
    n, spp, k, layers = NMAX["sponza"], 5, 6, 2
    pos = probes_of(pair, "sponza")
    want = want_of(po, pairs, "sponza", spp, k, n, layers)
    pair.dev.set_option("counters", 0)
    pair.dev.set_option("wf_sort_min", 16)
    try:
        sh, m2 = run(ca, pair.dev, pos, spp, k, layers)
        build = pair.dev.last_trace_build()
    finally:
        pair.dev.set_option("wf_sort_min", 1 << 16)
        pair.dev.set_option("counters", 1)
    assert build == 59
    assert_bitwise(sh, want[0], "sponza stand-in, build 59")
    assert_bitwise(m2, want[1], "sponza stand-in, build 59, moments")


# --- 6. null moments, no probes, bad arguments -------------------------------------------------------------

def test_no_probes_and_bad_arguments(ca, po, pairs):
    import torch
    pair = pairs("cornell")
    n, spp, k = 65, 5, 6
    run(ca, pair.dev, probes_of(pair, "cornell")[:n], spp, k, LAYERS, m2=False)
    before = pair.dev.counters()
    assert before["paths"] == n * spp * LAYERS
    rp = ca.radiance_params(spp, k, SEED, BG)
    t = torch.zeros(27, dtype=torch.float32, device="cuda")
    pair.dev.probe_sh_device(0, 0, rp, 3, 0, 0, 0)
    pair.dev.probe_sh_device(0, t.data_ptr(), rp, 3, t.data_ptr(), 0, 0)
    assert pair.dev.counters() == before  # nothing launched: the last call's counters are still there
    assert len(pair.dev.probe_sh(np.zeros((0, 3), F32), rp, 3)) == 0
    pair.dev.probe_eval_device(0, 0, 0, 0, 0, 0)
    pair.dev.probe_sample_device(ca.probe_grid(*GRIDS[2]), 0, 0, 0, 0, 0, 0)
    assert pair.dev.counters() == before
    hip = ca.libs()[0]
    P = C.c_void_p
    bare = ca.Device(0)  # no scene: the projection needs one, the lookups do not
    try:
        rc = hip.cr_probe_sh_device(bare._c, 1, P(t.data_ptr()), C.byref(rp), 1, P(t.data_ptr()), None, None)
        assert ca.CR_ERRORS.get(rc) == "CR_E_NOSCENE"
        sh = np.ones((1, 9, 3), F32)
        got = bare.probe_eval(sh, [0], [[0, 0, 1]])
        assert_bitwise(got, pm.evaluate(sh, np.array([[0, 0, 1]], F32)), "a lookup without a scene")
    finally:
        bare.close()
    pair.dev.set_option("perf_counters", 1)
    try:
        rc = hip.cr_probe_sh_device(pair.dev._c, 1, P(t.data_ptr()), C.byref(rp), 1, P(t.data_ptr()), None, None)
    finally:
        pair.dev.set_option("perf_counters", 0)
    assert ca.CR_ERRORS.get(rc) == "CR_E_INVALID"


# --- 7. evaluation and lookup ------------------------------------------------------------------------------

def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def lookup_points(origin, step, dims, m):
    """Inside the grid, on its probes, and outside it on every side."""
    origin, step, d = np.array(origin, np.float64), np.array(step, np.float64), np.array(dims)
    rng = np.random.default_rng(m + sum(dims))
    span = step * np.maximum(d - 1, 1)
    pts = np.concatenate([origin + span * rng.uniform(0, 1, (m, 3)), origin + span * rng.uniform(-1.5, 2.5, (m, 3)),
                          pm.grid_positions(origin, step, dims).astype(np.float64)])
    return pts[rng.permutation(len(pts))[:m]].astype(F32)


@pytest.mark.parametrize("m", [1, 63, 65, 1025])
def test_evaluation_and_lookup(ca, po, pairs, m):
    import torch
    pair = pairs("cornell")
    sh = want_of(po, pairs, "cornell", 5, 6, 257)[0]
    dsh = torch.from_numpy(sh.copy()).cuda()
    rng = np.random.default_rng(m)
    probe = rng.integers(0, 257, m).astype(np.uint32)
    probe[0] = 256
    nrm = unit_normals(m, m + 1)
    dn = torch.from_numpy(nrm).cuda()
    dpr = torch.from_numpy(probe.view(np.int32).copy()).cuda()
    out = Guarded(3 * m)
    pair.dev.probe_eval_device(m, dsh.data_ptr(), dpr.data_ptr(), dn.data_ptr(), out.ptr, 0)
    torch.cuda.synchronize()
    out.assert_guards("eval")
    want = pm.evaluate(sh[probe], nrm)
    assert_bitwise(out.numpy().reshape(m, 3), want, "cr_probe_eval_device m %d" % m)
    assert float(want.sum()) > 0
    assert np.array_equal(dsh.cpu().numpy().view(np.uint32), sh.view(np.uint32)), "coefficients changed"
    for origin, step, dims in GRIDS:
        count = dims[0] * dims[1] * dims[2]
        pos = lookup_points(origin, step, dims, m)
        dpos = torch.from_numpy(pos).cuda()
        out = Guarded(3 * m)
        pair.dev.probe_sample_device(ca.probe_grid(origin, step, dims), dsh.data_ptr(), m, dpos.data_ptr(),
                                     dn.data_ptr(), out.ptr, 0)
        torch.cuda.synchronize()
        out.assert_guards("sample")
        want = pm.lookup(origin, step, dims, sh[:count], pos, nrm)
        assert_bitwise(out.numpy().reshape(m, 3), want, "cr_probe_sample_device m %d dims %s" % (m, dims))


# --- 8. isolation ------------------------------------------------------------------------------------------

def test_isolation(ca, pairs):
    pair = pairs("cornell")
    dev = pair.dev
    x, y, spp, k = 16, 12, 2, 6
    cam = pair.camera(ca, x, y)
    pos = probes_of(pair, "cornell")[:65]
    want = None
    frames = []
    for layer in (1, 2, 3):
        want, _ = pair.oracle.render(cam.as_array(), x, y, spp, k, SEED, layer=layer, bg=BG,
                                     pixels=None if want is None else want.copy())
        frames.append(want)
    p = lambda layer: ca.render_params(x, y, spp, k, SEED, layer=layer, background=BG)
    dev.render(cam, p(1))
    got2 = dev.render(cam, p(2))
    run(ca, dev, pos, 5, k, 2)
    got3 = dev.render(cam, p(3))
    assert_bitwise(got2, frames[1], "two plain layers")
    assert_bitwise(got3, frames[2], "layers 1..2, a probe call, then layer 3")
    # the temporal history
    dev.render_temporal(cam, p(1), 1)
    before = dev.temporal_history(x, y)
    run(ca, dev, pos, 5, k, 2)
    after = dev.temporal_history(x, y)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "temporal history changed"
    # a bake
    W, H, uv = ca.bake_atlas_grid(dev.scene_triangles(), 4)
    bp = ca.bake_params(W, H, spp=2, k=k, seed=SEED, background=BG)
    first = dev.bake(bp, uv, 2)
    run(ca, dev, pos, 5, k, 2)
    again = dev.bake(bp, uv, 2)
    for key in ("lightmap", "m2"):
        assert_bitwise(again[key], first[key], "a bake after a probe call: " + key)
    assert np.array_equal(again["owner"], first["owner"])


# --- 9. mirrors --------------------------------------------------------------------------------------------

def test_mirrors(ca, pairs, scenes):
    import torch
    pair = pairs("cornell")
    layers = 2
    grid_def = ((-0.8, 0.2, -0.8), (0.4, 0.5, 0.8), (4, 3, 2))
    grid = ca.probe_grid(*grid_def)
    pos = ca.probe_grid_positions(grid)
    n = len(pos)
    scene = ca.Scene(scenes.config_rtc("cornell"), "samples", "3")
    i = scene.info
    spp, k, bg = i["samples"], i["k"], tuple(i["background"])
    assert (spp, i["seed"]) == (3, SEED)
    rp = ca.radiance_params(spp, k, SEED, bg)
    dp = torch.from_numpy(pos.copy()).cuda()
    dsh = torch.zeros((n, 27), dtype=torch.float32, device="cuda")
    pair.dev.probe_sh_device(n, dp.data_ptr(), rp, layers, dsh.data_ptr(), 0, 0)
    sh = dsh.cpu().numpy().reshape(n, 9, 3)
    assert float(np.abs(sh).sum()) > 0
    m = 65
    q = lookup_points(*grid_def, m)
    nrm = unit_normals(m, 3)
    dq, dn = torch.from_numpy(q).cuda(), torch.from_numpy(nrm).cuda()
    dout = torch.zeros((m, 3), dtype=torch.float32, device="cuda")
    pair.dev.probe_sample_device(grid, dsh.data_ptr(), m, dq.data_ptr(), dn.data_ptr(), dout.data_ptr(), 0)
    torch.cuda.synchronize()
    looked = dout.cpu().numpy()
    assert float(looked.sum()) > 0
    # the host forms of the C-ABI
    assert_bitwise(pair.dev.probe_sh(pos, rp, layers), sh, "cr_probe_sh")
    one = pair.dev.probe_sh(pos, ca.radiance_params(spp, k, SEED, bg, layer=1), 1)
    m2 = np.zeros_like(one)
    two = pair.dev.probe_sh(pos, ca.radiance_params(spp, k, SEED, bg, layer=2), 1, sh=one.copy(), m2=m2)
    assert_bitwise(two, sh, "cr_probe_sh, layer 2 blended onto the caller's layer 1")
    assert_bitwise(pair.dev.probe_sample(grid, sh, q, nrm), looked, "cr_probe_sample")
    probe = np.arange(m, dtype=np.uint32) % n
    assert_bitwise(pair.dev.probe_eval(sh, probe, nrm), pm.evaluate(sh[probe], nrm), "cr_probe_eval")
    # RayTracer and the C API under it
    rt = ca.RayTracer(ca.Model(scene), scene)
    assert_bitwise(rt.bakeProbes(grid, layers), sh, "RayTracer.bakeProbes(grid)")
    assert rt.counters()["paths"] == n * spp * layers
    assert_bitwise(rt.bakeProbes(pos, layers), sh, "RayTracer.bakeProbes(positions)")
    assert_bitwise(rt.sampleProbes(grid, sh, q, nrm), looked, "RayTracer.sampleProbes")
    host = ca.libs()[1]
    FP = C.POINTER(C.c_float)
    f = lambda a: a.ctypes.data_as(FP)
    out = np.zeros((n, 9, 3), F32)
    assert host.chiaro_raytracer_probes(rt._h, C.byref(grid), None, 0, layers, f(out)) == 0
    assert_bitwise(out, sh, "chiaro_raytracer_probes(grid)")
    out[:] = 0
    assert host.chiaro_raytracer_probes(rt._h, None, f(pos), n, layers, f(out)) == 0
    assert_bitwise(out, sh, "chiaro_raytracer_probes(positions)")
    res = np.zeros((m, 3), F32)
    flat = np.ascontiguousarray(sh.reshape(n, 27))
    assert host.chiaro_raytracer_probes_sample(rt._h, C.byref(grid), f(flat), f(q), f(nrm), m, f(res)) == 0
    assert_bitwise(res, looked, "chiaro_raytracer_probes_sample")
    assert host.chiaro_raytracer_probes(rt._h, None, None, n, layers, f(out)) == -1
    assert host.chiaro_raytracer_probes(rt._h, C.byref(grid), None, 0, 0, f(out)) == -1
    assert host.chiaro_raytracer_probes_sample(rt._h, None, f(flat), f(q), f(nrm), m, f(res)) == -1
