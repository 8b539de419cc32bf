"""Lightmap baking on the GPU (include/chiaro_hip.h "lightmap baking" and the list forms of "radiance queries",
DESIGN.md §3.29), bit for bit:

1. the texture-space kernels against tests/bake_model.py: owner, surface point, normal, covered list and count for the
   UV sets of tests/bake_cases.py at maps of 1 x 1, 7 x 5, 64 x 64, 65 x 63 and 130 x 3 and for the grid atlas at cells
   4 and 5, between guard bands, the inputs unchanged;
2. the list forms of the radiance queries against the non-list calls: listed entries equal, unlisted ones untouched;
3. a bake against the oracle: every covered texel is the fold of or_path over the model's surface points;
4. a bake against its parts, and a bake of half the triangles against the full one: a texel does not depend on which
   other texels are covered;
5. the adaptive bake against fixed bakes of each texel's layer count, its schedule replayed from cr_noise maps;
6. the dilation against the model;
7. isolation: the ctx's accumulators and temporal history do not see a bake;
8. the RayTracer and C API mirrors;
9. the errors on a device.

References are computed once and shared; nothing here changes them."""
import ctypes as C

import numpy as np
import pytest

import bake_cases as bc
import bake_model as bm
from helpers import Pair, assert_bitwise

pytestmark = pytest.mark.gpu

SEED, BG = 0xC41A05C0, (0.1, 0.2, 0.3)
F32 = np.float32
POISON = 0x7FC0DEAD  # a NaN payload: any write shows
NONE = bm.NONE

_PAIRS, _REF = {}, {}


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
    _REF.clear()


class Band:
    """`words` 32-bit words of device memory between two poisoned guard bands, poisoned themselves unless init."""

    def __init__(self, words, init=None, guard=1024):
        import torch
        self.n, self.g = int(words), guard
        self.t = torch.full((self.n + 2 * guard,), POISON, dtype=torch.int32, device="cuda")
        self.body = self.t[guard:guard + self.n]
        if init is not None:
            self.body.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1).view(np.int32)))
        self.ptr = self.body.data_ptr()

    def u32(self):
        return self.body.cpu().numpy().view(np.uint32)

    def f32(self):
        return self.body.cpu().numpy().view(F32)

    def assert_guards(self, what):
        bits = self.t.cpu().numpy()
        assert (bits[:self.g] == POISON).all() and (bits[self.g + self.n:] == POISON).all(), what + ": guard band"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def scene_arrays(pair):
    """(tri_pos [n][9], tri_normal [n][3], tri_uv [n][6]) float32 as uploaded."""
    d = pair.desc
    n = int(d.n_tris)
    get = lambda p, k: np.ctypeslib.as_array(p, shape=(n * k,)).copy().reshape(n, k)
    return get(d.tri_pos, 9), get(d.tri_normal, 3), get(d.tri_uv, 6)


def surface_gpu(ca, dev, uv, W, H, offset=None):
    """cr_bake_surface_device -> (owner [H][W], pos, nrm [H][W][3], list [count]); guards and inputs checked."""
    import torch
    n = W * H
    d_uv = torch.from_numpy(np.ascontiguousarray(uv).view(np.int32)).cuda() if uv is not None else None
    owner, pos, nrm, lst, cnt = Band(n), Band(3 * n), Band(3 * n), Band(n), Band(1)
    bp = ca.bake_params(W, H, offset=offset)
    dev.bake_surface_device(bp, d_uv.data_ptr() if uv is not None else 0, owner.ptr, pos.ptr, nrm.ptr, lst.ptr, cnt.ptr, 0)
    torch.cuda.synchronize()
    for b, what in ((owner, "owner"), (pos, "pos"), (nrm, "nrm"), (lst, "list"), (cnt, "count")):
        b.assert_guards(what)
    if uv is not None:
        assert same_bits(d_uv.cpu().numpy().view(np.uint32), np.ascontiguousarray(uv).view(np.uint32)), "UVs changed"
    count = int(cnt.u32()[0])
    assert count <= n
    full = lst.u32()
    assert (full[count:] == POISON).all(), "the list is written past its count"
    return owner.u32().reshape(H, W), pos.f32().reshape(H, W, 3), nrm.f32().reshape(H, W, 3), full[:count]


# --- 1. raster against the model ---------------------------------------------------------------------------

def raster_cases():
    for name, uv in (("crafted", bc.crafted_uv()), ("random", bc.random_uv())):
        for W, H in bc.MAPS:
            yield pytest.param(uv, W, H, id="%s-%dx%d" % (name, W, H))
    for cell in (4, 5):
        W, H, uv = bm.atlas_grid(bc.N_TRIS, cell)
        yield pytest.param(uv, W, H, id="atlas%d-%dx%d" % (cell, W, H))


@pytest.mark.parametrize("uv,W,H", list(raster_cases()))
def test_raster_against_the_model(ca, pairs, uv, W, H):
    pair = pairs("cornell")
    tri_pos, tri_nrm, _ = scene_arrays(pair)
    assert len(tri_pos) == bc.N_TRIS
    want = bm.surface(uv, tri_pos, tri_nrm, W, H, 0.001)
    if (W, H) != (1, 1):
        assert 0 < len(want[3]) < W * H  # (a dead kernel cannot pass)
    got = surface_gpu(ca, pair.dev, uv, W, H)
    for g, w, part in zip(got, want, ("owner", "pos", "nrm", "list")):
        assert same_bits(g, w), part


def test_raster_scene_uvs_and_offset(ca, pairs):
    """A null d_uv is the scene's own tri_uv (the textured nanobox stand-in: thousands of triangles, more than one
    block of the owner pass); an offset other than the default."""
    pair = pairs("nanobox")
    tri_pos, tri_nrm, tri_uv = scene_arrays(pair)
    W, H = 65, 63
    for uv, offset in ((None, None), (tri_uv, 0.25)):
        want = bm.surface(tri_uv, tri_pos, tri_nrm, W, H, 0.001 if offset is None else offset)
        got = surface_gpu(ca, pair.dev, uv, W, H, offset)
        assert len(want[3]) > 0
        for g, w, part in zip(got, want, ("owner", "pos", "nrm", "list")):
            assert same_bits(g, w), part


# --- 2. list gathers ---------------------------------------------------------------------------------------

def gather_points(pair):
    """(pos, nrm) [257][3]: test_gpu_radiance.gather_points -- the first hits of random rays from inside the box, the
    normal towards the ray's side, the point 0.001 normal off the surface (float32)."""
    if "points" not in _REF:
        rng = np.random.default_rng(7)
        b = pair.oracle.kd_export()["box"].astype(np.float64)
        lo, hi = b[:3], b[3:]
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
        _REF["points"] = ((pos + F32(0.001) * nrm).astype(F32), nrm)
    return _REF["points"]


def query(ca, dev, a, b, lst, spp, k, nlayers, gather, layer=1, id0=0, out0=None, m20=None):
    """One device call over the n entries (a, b): the list form when lst is given.  -> (out, m2) [n][3], whose
    unwritten entries still hold the poison (or out0 / m20); guards and inputs checked."""
    import torch
    n = len(a)
    da, db = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    o, m = Band(3 * n, init=out0), Band(3 * n, init=m20)
    rp = ca.radiance_params(spp, k, SEED, BG, layer=layer, id0=id0)
    if lst is None:
        (dev.gather_device if gather else dev.radiance_device)(n, da.data_ptr(), db.data_ptr(), rp, nlayers, o.ptr, m.ptr, 0)
    else:
        dl = torch.from_numpy(np.ascontiguousarray(lst, np.uint32).view(np.int32)).cuda()
        fn = dev.gather_list_device if gather else dev.radiance_list_device
        fn(n, da.data_ptr(), db.data_ptr(), dl.data_ptr() if len(lst) else 0, len(lst), rp, nlayers, o.ptr, m.ptr, 0)
        torch.cuda.synchronize()
        assert same_bits(dl.cpu().numpy().view(np.uint32), np.ascontiguousarray(lst, np.uint32)), "list changed"
    torch.cuda.synchronize()
    o.assert_guards("out"), m.assert_guards("m2")
    assert same_bits(da.cpu().numpy(), a) and same_bits(db.cpu().numpy(), b), "inputs changed"
    return o.f32().reshape(n, 3), m.f32().reshape(n, 3)


def lists_of(n):
    rng = np.random.default_rng(3)
    out = {}
    for m in (1, 63, 64, 65, 257):
        out["%d entries" % m] = np.sort(rng.permutation(n)[:m]).astype(np.uint32)
    out["out of order"] = rng.permutation(n)[:100].astype(np.uint32)
    skipped = rng.permutation(n)[:80].astype(np.uint32)
    skipped[::5] = 0xFFFFFFFF
    out["skipped entries"] = skipped
    beyond = rng.permutation(n)[:80].astype(np.uint32)
    beyond[1::4] = n + np.arange(len(beyond[1::4]), dtype=np.uint32) * 1000
    out["entries >= n"] = beyond
    out["empty"] = np.zeros(0, np.uint32)
    return out


@pytest.mark.parametrize("gather", [True, False], ids=["gather", "radiance"])
def test_list_forms(ca, pairs, gather):
    pair = pairs("cornell")
    n, spp, k, layers = 257, 2, 6, 2
    a, b = gather_points(pair)
    full = query(ca, pair.dev, a, b, None, spp, k, layers, gather)
    assert float(full[0].sum()) > 0
    for what, lst in lists_of(n).items():
        got = query(ca, pair.dev, a, b, lst, spp, k, layers, gather)
        listed = np.zeros(n, bool)
        listed[lst[lst < n]] = True
        for g, w, part in zip(got, full, ("out", "m2")):
            assert_bitwise(g[listed], w[listed], "%s: listed entries, %s" % (what, part))
            assert (g[~listed].view(np.uint32) == POISON).all(), "%s: unlisted entries of %s written" % (what, part)
    # two list calls of one layer each are one call of two layers
    lst = lists_of(n)["out of order"]
    one = query(ca, pair.dev, a, b, lst, spp, k, 1, gather)
    two = query(ca, pair.dev, a, b, lst, spp, k, 1, gather, layer=2, out0=one[0], m20=one[1])
    for g, w in zip(two, full):
        assert_bitwise(g[lst], w[lst], "two list calls of one layer")
    # id0 = 5: other streams, those of the non-list call with id0 = 5
    moved = query(ca, pair.dev, a, b, None, spp, k, layers, gather, id0=5)
    got = query(ca, pair.dev, a, b, lst, spp, k, layers, gather, id0=5)
    assert (moved[0].view(np.uint32) != full[0].view(np.uint32)).any()
    for g, w in zip(got, moved):
        assert_bitwise(g[lst], w[lst], "id0 = 5")


# --- 3. bake against the oracle ----------------------------------------------------------------------------

def uniform_f32(u, a, b):
    """rng_uniform on a raw draw, restated in float32: the conversion and division, the guard, the scale."""
    c = F32(np.uint32(u)) / F32(4294967296.0)
    if c >= F32(1.0):
        c = F32(float.fromhex("0x1.fffffep-1"))
    return F32(c * (F32(b) - F32(a)) + F32(a))


def gather_samples(po, pair, pos, nrm, ids, spp, k, layers):
    """[layers][n][spp][3]: or_path of every sample gathered at (pos, nrm) on stream id, layers 1 .. layers."""
    out = np.zeros((layers, len(ids), spp, 3), F32)
    for i, j in enumerate(ids):
        for L in range(1, layers + 1):
            for s in range(spp):
                u = po.rng_draws(SEED, L, int(j), s, 2)
                wi, _ = po.sample_wi(nrm[i], uniform_f32(u[0], -1, 1), uniform_f32(u[1], -1, 1))
                cam = np.concatenate([pos[i], wi, np.zeros(6, F32)]).astype(F32)
                out[L - 1, i, s] = pair.oracle.path(cam, int(j) + 1, 1, k, BG, SEED, L, int(j), 0, s)
    return out


def fold(samples):
    """The frame arithmetic over [layers][n][spp][3] samples from layer 1: (out, m2) after the last layer."""
    nl, n, spp, _ = samples.shape
    out, m2 = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    inv = F32(1.0) / F32(spp)
    for j in range(nl):
        L = 1 + j
        t, q = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
        for s in range(spp):
            r = samples[j, :, s]
            t = t + r
            q = q + r * r
        out = (out * F32(L - 1) + t * inv) / F32(L)
        m2 = (m2 * F32(L - 1) + q * inv) / F32(L)
    return out, m2


def cornell_atlas(pair):
    """The 24 x 24 grid atlas of cornell's 36 triangles and the model's surface over it."""
    if "atlas" not in _REF:
        tri_pos, tri_nrm, _ = scene_arrays(pair)
        W, H, uv = bm.atlas_grid(len(tri_pos), 4)
        assert (W, H) == (24, 24)
        _REF["atlas"] = (W, H, uv) + bm.surface(uv, tri_pos, tri_nrm, W, H, 0.001)
    return _REF["atlas"]


def bake(ca, dev, W, H, uv, spp, k, **kw):
    return dev.bake(ca.bake_params(W, H, spp=spp, k=k, seed=SEED, background=BG), uv, **kw)


def test_bake_against_the_oracle(ca, po, pairs):
    pair = pairs("cornell")
    W, H, uv, owner, pos, nrm, lst = cornell_atlas(pair)
    spp, k, layers = 2, 6, 2
    assert 36 <= len(lst) < W * H
    want = fold(gather_samples(po, pair, pos.reshape(-1, 3)[lst], nrm.reshape(-1, 3)[lst], lst, spp, k, layers))
    r = bake(ca, pair.dev, W, H, uv, spp, k, nlayers=layers)
    out, m2 = r["lightmap"].reshape(-1, 3), r["m2"].reshape(-1, 3)
    assert same_bits(r["owner"], owner)
    assert_bitwise(out[lst], want[0], "covered texels")
    assert_bitwise(m2[lst], want[1], "covered texels, moments")
    uncovered = owner.reshape(-1) == NONE
    assert not out[uncovered].view(np.uint32).any() and not m2[uncovered].view(np.uint32).any()
    assert float(out.sum()) > 0
    assert same_bits(r["layers"].reshape(-1), np.where(uncovered, 0, layers).astype(np.uint32))
    assert r["stats"] == {"covered": len(lst), "texel_layers": len(lst) * layers, "active": 0, "layers": layers,
                          "checks": 0, "max_err": 0.0}
    assert pair.dev.counters()["paths"] == len(lst) * spp * layers


# --- 4. bake = its parts ------------------------------------------------------------------------------------

def test_bake_equals_its_parts(ca, pairs):
    import torch
    pair = pairs("nanobox")
    dev = pair.dev
    n_tris = dev.scene_triangles()
    W, H, uv = ca.bake_atlas_grid(n_tris, 2)
    n, spp, k, layers, passes = W * H, 1, 4, 2, 2
    r = bake(ca, dev, W, H, uv, spp, k, nlayers=layers, dilate=passes)
    covered = int(r["stats"]["covered"])
    assert n_tris // 2 < covered < n and float(r["lightmap"].sum()) > 0
    # the parts
    owner, pos, nrm, lst = surface_gpu(ca, dev, uv, W, H)
    assert len(lst) == covered and same_bits(owner, r["owner"])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.int32)).cuda()
    d_pos, d_nrm, d_list, d_owner = d(pos), d(nrm), d(lst), d(owner)
    out = torch.zeros(3 * n, dtype=torch.float32, device="cuda")
    m2, dil = torch.zeros_like(out), torch.zeros_like(out)
    rp = ca.radiance_params(spp, k, SEED, BG)
    dev.gather_list_device(n, d_pos.data_ptr(), d_nrm.data_ptr(), d_list.data_ptr(), covered, rp, layers, out.data_ptr(),
                           m2.data_ptr(), 0)
    dev.bake_dilate_device(W, H, d_owner.data_ptr(), passes, out.data_ptr(), dil.data_ptr(), 0)
    torch.cuda.synchronize()
    assert_bitwise(out.cpu().numpy().reshape(H, W, 3), r["lightmap"], "surface + gather_list")
    assert_bitwise(m2.cpu().numpy().reshape(H, W, 3), r["m2"], "surface + gather_list, moments")
    assert_bitwise(dil.cpu().numpy().reshape(H, W, 3), r["dilated"], "... + dilate")
    assert_bitwise(r["dilated"], bm.dilate(owner, r["lightmap"], passes), "the dilated map against the model")
    # half the triangles: the others' UVs are NaN, and the texels that remain hold the full bake's bits
    half = uv.copy()
    half[1::2] = np.nan
    h = bake(ca, dev, W, H, half, spp, k, nlayers=layers)
    kept = h["owner"] != NONE
    assert 0 < kept.sum() < covered and (h["owner"][kept] % 2 == 0).all()
    assert same_bits(h["owner"][kept], r["owner"][kept])
    assert_bitwise(h["lightmap"][kept], r["lightmap"][kept], "half the triangles")
    assert_bitwise(h["m2"][kept], r["m2"][kept], "half the triangles, moments")
    assert not h["lightmap"][~kept].view(np.uint32).any()


# --- 5. adaptive bake ---------------------------------------------------------------------------------------

def err_map(dev, frame, m2, layers, spp, floor):
    """cr_noise_device's error map of a host (frame, m2) pair [H][W][3]."""
    import torch
    H, W, _ = frame.shape
    f, m = torch.from_numpy(frame.copy()).cuda(), torch.from_numpy(m2.copy()).cuda()
    err = torch.zeros(H * W, dtype=torch.float32, device="cuda")
    st = torch.zeros(8, dtype=torch.int32, device="cuda")
    dev.noise_device(W * H, 1, layers, spp, 0.0, floor, f.data_ptr(), m.data_ptr(), err.data_ptr(), st.data_ptr(), 0)
    torch.cuda.synchronize()
    return err.cpu().numpy().reshape(H, W)


def test_adaptive_bake(ca, pairs):
    pair = pairs("cornell")
    dev = pair.dev
    W, H, uv, owner, _, _, lst = cornell_atlas(pair)
    spp, k, floor, max_layers = 2, 6, 1e-3, 4
    fixed = [None] + [bake(ca, dev, W, H, uv, spp, k, nlayers=L) for L in range(1, max_layers + 1)]
    covered = owner != NONE
    errs = [None] + [err_map(dev, fixed[L]["lightmap"], fixed[L]["m2"], L, spp, floor) for L in range(1, max_layers + 1)]
    assert not errs[1][~covered].any()  # (0 / floor: an uncovered texel is never above a threshold)
    threshold = float(np.median(errs[1][covered]))
    # the schedule replayed: min 1, max 4, a check after every layer; a texel whose err is not above the threshold
    # at a check is frozen at that layer
    active, want_layers, checks, last = covered.copy(), np.zeros((H, W), np.uint32), 0, None
    texel_layers = 0
    for L in range(1, max_layers + 1):
        if not active.any():
            break
        want_layers[active] = L
        texel_layers += int(active.sum())
        checks += 1
        last = (L, active.copy())
        if L < max_layers:
            active = active & (errs[L] > F32(threshold))
    assert len(np.unique(want_layers[covered])) >= 2, "some texels freeze and some do not"
    ap = ca.CrAdaptiveParams(1, max_layers, 1)
    r = bake(ca, dev, W, H, uv, spp, k, adaptive=ap, threshold=threshold, floor=floor)
    assert same_bits(r["layers"], want_layers)
    for L in range(1, max_layers + 1):
        at = want_layers == L
        assert_bitwise(r["lightmap"][at], fixed[L]["lightmap"][at], "texels of %d layers" % L)
        assert_bitwise(r["m2"][at], fixed[L]["m2"][at], "texels of %d layers, moments" % L)
    assert not r["lightmap"][~covered].view(np.uint32).any()
    L, was = last
    st = r["stats"]
    assert (st["covered"], st["texel_layers"], st["layers"], st["checks"]) == (len(lst), texel_layers, L, checks)
    assert st["texel_layers"] == int(want_layers.sum())
    assert st["active"] == int((was & (errs[L] > F32(threshold))).sum())
    assert F32(st["max_err"]) == errs[L][was].max()
    # the same schedule and bits when every pass is cut into small path chunks
    dev.set_option("wf_paths", 4096)
    try:
        small = bake(ca, dev, W, H, uv, spp, k, adaptive=ap, threshold=threshold, floor=floor)
    finally:
        dev.set_option("wf_paths", 256 << 20)
    assert same_bits(small["layers"], r["layers"]) and small["stats"] == st
    assert_bitwise(small["lightmap"], r["lightmap"], "forced small wf_paths")
    assert_bitwise(small["m2"], r["m2"], "forced small wf_paths, moments")


# --- 6. dilation against the model ---------------------------------------------------------------------------

def dilate_cases():
    W, H = 65, 63
    owner = bm.surface(bc.crafted_uv(), *bc.mesh(), W, H)[0]
    for passes in (0, 1, 3):
        yield pytest.param(owner, passes, id="crafted-%d-passes" % passes)
    yield pytest.param(np.full((H, W), NONE, np.uint32), 3, id="empty-owner-map")
    one = np.full((H, W), NONE, np.uint32)
    one[31, 40] = 7
    yield pytest.param(one, 3, id="single-owned-texel")
    corner = np.full((H, W), NONE, np.uint32)
    corner[0, 0] = corner[H - 1, W - 1] = 0
    yield pytest.param(corner, 1000, id="corners-every-pass")


@pytest.mark.parametrize("owner,passes", list(dilate_cases()))
def test_dilation_against_the_model(ca, pairs, owner, passes):
    import torch
    dev = pairs("cornell").dev
    H, W = owner.shape
    values = bc.dilate_values(W, H)
    want = bm.dilate(owner, values, passes)
    d_owner = torch.from_numpy(owner.view(np.int32).copy()).cuda()
    d_in = torch.from_numpy(values.copy()).cuda()
    out = Band(3 * W * H)
    dev.bake_dilate_device(W, H, d_owner.data_ptr(), passes, d_in.data_ptr(), out.ptr, 0)
    torch.cuda.synchronize()
    out.assert_guards("dilated")
    assert same_bits(d_in.cpu().numpy(), values) and same_bits(d_owner.cpu().numpy().view(np.uint32), owner)
    got = out.f32().reshape(H, W, 3)
    assert_bitwise(got, want, "dilation")
    if passes == 0 or not (owner != NONE).any():
        assert_bitwise(got, values, "a copy")
    else:
        assert (got.view(np.uint32) != values.view(np.uint32)).any()


# --- 7. isolation -------------------------------------------------------------------------------------------

def test_isolation(ca, pairs):
    pair = pairs("cornell")
    dev = pair.dev
    W, H, uv = cornell_atlas(pair)[:3]
    x, y, spp, k = 16, 12, 2, 6
    cam = pair.camera(ca, x, y)
    p = lambda layer: ca.render_params(x, y, spp, k, SEED, layer=layer, background=BG)
    ap = ca.CrAdaptiveParams(1, 3, 1)
    plain = [dev.render(cam, p(layer)).copy() for layer in (1, 2, 3)]
    dev.render(cam, p(1))
    dev.render(cam, p(2))
    bake(ca, dev, W, H, uv, spp, k, nlayers=2, dilate=2)
    bake(ca, dev, W, H, uv, spp, k, adaptive=ap, threshold=0.05)
    assert_bitwise(dev.render(cam, p(3)), plain[2], "layers 1..2, two bakes, then layer 3")
    # the moment accumulator of a noise render
    dev.render_layers_noise(cam, p(1), 2)
    st_before, err_before = dev.noise(x, y, 2, spp, 0.05, 1e-3)
    bake(ca, dev, W, H, uv, spp, k, adaptive=ap, threshold=0.05)
    bake(ca, dev, W, H, uv, spp, k, nlayers=1)
    st_after, err_after = dev.noise(x, y, 2, spp, 0.05, 1e-3)
    assert st_before == st_after and same_bits(err_before, err_after) and float(err_before.sum()) > 0
    # the temporal history
    dev.render_temporal(cam, p(1), 1)
    before = dev.temporal_history(x, y)
    bake(ca, dev, W, H, uv, spp, k, nlayers=1, dilate=1)
    after = dev.temporal_history(x, y)
    for a, b in zip(before, after):
        assert same_bits(a, b), "temporal history changed"


# --- 8. mirrors ---------------------------------------------------------------------------------------------

def test_mirrors(ca, pairs, scenes):
    pair = pairs("cornell")
    W, H, uv = cornell_atlas(pair)[:3]
    scene = ca.Scene(scenes.config_rtc("cornell"), "samples", "3")
    i = scene.info
    spp, k, bg = i["samples"], i["k"], tuple(i["background"])
    assert (spp, i["seed"]) == (3, SEED)
    bp = ca.bake_params(W, H, spp=spp, k=k, seed=SEED, background=bg)
    want = pair.dev.bake(bp, uv, nlayers=2, dilate=2)
    assert float(want["lightmap"].sum()) > 0
    rt = ca.RayTracer(ca.Model(scene), scene)
    got, dil = rt.bakeLightmap(W, H, uv, layers=2, dilate=2)
    assert_bitwise(got, want["lightmap"], "RayTracer.bakeLightmap")
    assert_bitwise(dil, want["dilated"], "RayTracer.bakeLightmap, dilated")
    assert rt.counters()["paths"] == want["stats"]["covered"] * spp * 2
    # no UVs: the grid atlas of the scene's triangles at the largest cell that fits -- at 24 x 24 the atlas above
    assert_bitwise(rt.bakeLightmap(W, H, None, layers=2), want["lightmap"], "RayTracer.bakeLightmap, grid atlas")
    # ... and in the top-left corner of a larger map
    big = rt.bakeLightmap(W + 3, H + 9, None, layers=2)
    assert not big[H:].view(np.uint32).any() and not big[:, W:].view(np.uint32).any() and float(big.sum()) > 0
    # the adaptive overload
    ap = ca.CrAdaptiveParams(1, 3, 1)
    wa = pair.dev.bake(bp, uv, adaptive=ap, threshold=0.05, floor=1e-3, dilate=1)
    ga, gd, gl = rt.bakeLightmap(W, H, uv, dilate=1, threshold=0.05, maxLayers=3)
    assert_bitwise(ga, wa["lightmap"], "adaptive bakeLightmap")
    assert_bitwise(gd, wa["dilated"], "adaptive bakeLightmap, dilated")
    assert same_bits(gl, wa["layers"])
    # the C API under it
    host = ca.libs()[1]
    FP = C.POINTER(C.c_float)
    out, d2 = np.zeros((H, W, 3), F32), np.zeros((H, W, 3), F32)
    u = np.ascontiguousarray(uv)
    assert host.chiaro_raytracer_bake(rt._h, W, H, u.ctypes.data_as(FP), 2, 2, out.ctypes.data_as(FP),
                                      d2.ctypes.data_as(FP)) == 0
    assert_bitwise(out, want["lightmap"], "chiaro_raytracer_bake")
    assert_bitwise(d2, want["dilated"], "chiaro_raytracer_bake, dilated")
    assert host.chiaro_raytracer_bake(rt._h, W, H, None, 2, 0, out.ctypes.data_as(FP), None) == 0
    assert_bitwise(out, want["lightmap"], "chiaro_raytracer_bake, grid atlas")
    assert host.chiaro_raytracer_bake(rt._h, W, H, None, 0, 0, out.ctypes.data_as(FP), None) == -1
    assert host.chiaro_raytracer_bake(rt._h, 0, H, None, 2, 0, out.ctypes.data_as(FP), None) == -1
    assert host.chiaro_raytracer_bake(rt._h, W, H, None, 2, 0, None, None) == -1
    assert host.chiaro_raytracer_bake(rt._h, 3, 3, None, 2, 0, out.ctypes.data_as(FP), None) == -2  # (no room for a cell)


# --- 9. errors on a device ----------------------------------------------------------------------------------

def test_invalid_arguments_on_a_device(ca, pairs):
    import torch
    pair = pairs("cornell")
    hip = ca.libs()[0]
    P = C.c_void_p
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = P(t.data_ptr())
    err = lambda rc: ca.CR_ERRORS.get(rc)
    bp = ca.bake_params(4, 4)
    assert err(hip.cr_bake_surface_device(pair.dev._c, C.byref(bp), None, p, p, p, p, None, None)) == "CR_E_INVALID"
    assert err(hip.cr_bake_surface_device(pair.dev._c, None, None, p, p, p, p, p, None)) == "CR_E_INVALID"
    for w, h in ((0, 4), (4, 0), (65536, 32769)):
        bad = ca.bake_params(w, h)
        assert err(hip.cr_bake_surface_device(pair.dev._c, C.byref(bad), None, p, p, p, p, p, None)) == "CR_E_INVALID"
        assert err(hip.cr_bake_dilate_device(pair.dev._c, w, h, p, 1, p, P(t.data_ptr() + 4), None)) == "CR_E_INVALID"
        out = np.zeros(16 * 3, F32)
        assert err(hip.cr_bake(pair.dev._c, C.byref(bad), None, 1, None, None, 0, out.ctypes.data_as(C.POINTER(C.c_float)),
                               None, None, None, None, None)) == "CR_E_INVALID"
    assert err(hip.cr_bake_dilate_device(pair.dev._c, 4, 4, p, 1, p, p, None)) == "CR_E_INVALID"
    rp = ca.radiance_params(2, 3, SEED, BG)
    assert err(hip.cr_gather_list_device(pair.dev._c, 4, p, p, None, 2, C.byref(rp), 1, p, None, None)) == "CR_E_INVALID"
    bare = ca.Device(0)  # no scene
    try:
        assert err(hip.cr_bake_surface_device(bare._c, C.byref(bp), None, p, p, p, p, p, None)) == "CR_E_NOSCENE"
        assert err(hip.cr_gather_list_device(bare._c, 4, p, p, p, 2, C.byref(rp), 1, p, None, None)) == "CR_E_NOSCENE"
        out = np.zeros(16 * 3, F32)
        assert err(hip.cr_bake(bare._c, C.byref(bp), None, 1, None, None, 0, out.ctypes.data_as(C.POINTER(C.c_float)),
                               None, None, None, None, None)) == "CR_E_NOSCENE"
        # the dilation needs no scene
        owner = torch.full((16,), -1, dtype=torch.int32, device="cuda")
        src, dst = torch.ones(48, dtype=torch.float32, device="cuda"), torch.zeros(48, dtype=torch.float32, device="cuda")
        assert hip.cr_bake_dilate_device(bare._c, 4, 4, P(owner.data_ptr()), 2, P(src.data_ptr()), P(dst.data_ptr()),
                                         None) == 0
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == 1).all()
    finally:
        bare.close()
