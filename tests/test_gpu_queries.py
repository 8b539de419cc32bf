"""Device-resident batched ray queries (cr_intersect_device / cr_intersect_shadow_device) on the GPU.

Every comparison is bit for bit, on uint32 views, against the oracle's or_intersect / or_intersect_shadow
and against the legacy host-array entry points on the same rays: cornell runs trace build 44, the sponza
stand-in build 59 (compressed leaf-cull records and the leaf exchange).

The 4096 rays per scene (fixed seed) start from test_gpu_parity.test_ray_queries_bitexact's mix -- random
in-box origins with normal-distributed directions, one eighth with two zero components, one eighth with
one, one eighth with origins exactly on split planes -- and add a quarter normalised to unit length in
float32 (so the leaf-cull records are really evaluated) and 512 origins outside the scene's coordinate
bound, on a sphere of three box diagonals, aimed at random in-box points, half unit and half not (the
kernels without the leaf cull).  No NaN or infinite rays: tests/test_queryroute.py covers their routing
on the CPU and they then run cr_intersect's own kernel.
"""
import ctypes

import numpy as np
import pytest

from helpers import Pair, assert_bitwise

pytestmark = pytest.mark.gpu

N = 4096
N_OUT = 512
SENT_U, SENT_F = 0x5EED5EED, -12345.5
WORK_KEYS = ("closest", "shadow", "inner", "leaf", "tritest", "hit", "texhit", "paths", "pixels")
DEFAULTS = {"query_route": 0, "query_sort": -1, "query_chunk": 1 << 24, "query_trace_min": 1 << 16}


class Case:
    """A scene pair, its ray set on the host and the device, and the oracle's answers (computed once)."""

    def __init__(self, ca, po, scenes, name, seed, device=True):
        self.pair = Pair(ca, po, scenes.config_rtc(name), device=device)
        rng = np.random.default_rng(seed)
        e = self.pair.oracle.kd_export()
        lo, hi = e["box"][:3], e["box"][3:]
        diag = float(np.linalg.norm(hi - lo))
        n = N
        o = (lo + (hi - lo) * rng.random((n, 3), dtype=np.float32)).astype(np.float32)
        d = rng.normal(size=(n, 3)).astype(np.float32)
        d[: n // 8, 1:] = 0.0                 # axis-parallel (inf / NaN slabs)
        d[n // 8: n // 4, 0] = 0.0
        inner = np.nonzero(e["is_leaf"] == 0)[0][: n // 8]
        for j, ni in enumerate(inner):        # origins exactly on split planes
            o[n // 4 + j, e["axis"][ni]] = e["split"][ni]

        def unit(v):
            v = v.astype(np.float32)
            return (v / np.sqrt((v * v).sum(axis=1, dtype=np.float32), dtype=np.float32)[:, None]).astype(np.float32)

        d[n // 2: 3 * n // 4] = unit(d[n // 2: 3 * n // 4])
        # outside the coordinate bound: on a sphere of three diagonals about the box centre
        s = unit(rng.normal(size=(N_OUT, 3)))
        centre = (0.5 * (lo + hi)).astype(np.float32)
        oo = (centre + np.float32(3.0 * diag) * s).astype(np.float32)
        target = (lo + (hi - lo) * rng.random((N_OUT, 3), dtype=np.float32)).astype(np.float32)
        dd = (target - oo).astype(np.float32)
        dd[: N_OUT // 2] = unit(dd[: N_OUT // 2])
        o[n - N_OUT:], d[n - N_OUT:] = oo, dd
        # (cr_upload_scene's coordinate bound)
        db = np.float32(max(1.0, float(np.abs(e["box"]).max()) + 1.0) * 1.0001)
        self.outside = np.zeros(n, bool)
        self.outside[n - N_OUT:] = True
        assert (np.abs(o[self.outside]) > db).any(axis=1).all()
        assert (np.abs(o[~self.outside]) <= db).all()
        dn = (d.astype(np.float64) ** 2).sum(axis=1)
        assert (np.abs(dn[n // 2: 3 * n // 4] - 1.0) < 4e-7).all()  # inside lc_unit's window of 12 * 2^-24
        ids, _ = self.pair.oracle.lights()
        self.light = ids[rng.integers(0, len(ids), n)].astype(np.uint32)
        self.limit = (rng.random(n) * diag).astype(np.float32)
        self.o, self.d = np.ascontiguousarray(o), np.ascontiguousarray(d)
        self.want = self.pair.oracle.intersect(self.o, self.d)
        self.want_occ = self.pair.oracle.intersect_shadow(self.o, self.d, self.limit, self.light)
        # conditions on the oracle's answers alone
        h = self.want["hit"] == 1
        assert h[~self.outside].sum() > (n - N_OUT) // 4
        assert h[self.outside].sum() > N_OUT // 4
        assert (self.want_occ == 0).any() and (self.want_occ == 1).any()
        if not device:  # (the ray set and the oracle's answers alone: what the conditions above are about)
            return
        import torch
        dev = "cuda:0"
        self.t_o, self.t_d = torch.from_numpy(self.o).to(dev), torch.from_numpy(self.d).to(dev)
        self.t_limit = torch.from_numpy(self.limit).to(dev)
        self.t_light = torch.from_numpy(self.light.view(np.int32)).to(dev)

    def options(self, **kw):
        for k, v in {**DEFAULTS, **kw}.items():
            self.pair.dev.set_option(k, v)


@pytest.fixture(scope="module")
def cornell(ca, po, scenes):
    c = Case(ca, po, scenes, "cornell", 51)
    yield c
    c.options()


@pytest.fixture(scope="module")
def sponza(ca, po, scenes):
    c = Case(ca, po, scenes, "sponza", 52)
    yield c
    c.options()


@pytest.fixture(params=["cornell", "sponza"])
def case(request, cornell, sponza):
    c = {"cornell": cornell, "sponza": sponza}[request.param]
    c.options()
    yield c
    c.options()


def closest(case, idx=None, stream=0, nulls=False):
    """cr_intersect_device over the case's rays (idx: a subset / repetition), outputs pre-filled with a
    sentinel; returns host arrays."""
    import torch
    t_o, t_d = (case.t_o, case.t_d) if idx is None else (case.t_o[idx].contiguous(), case.t_d[idx].contiguous())
    n = t_o.shape[0]
    hit = torch.full((n,), SENT_U, dtype=torch.int32, device=t_o.device)
    tri = torch.full((n,), SENT_U, dtype=torch.int32, device=t_o.device)
    bary = torch.full((n, 2), SENT_F, dtype=torch.float32, device=t_o.device)
    dist = torch.full((n,), SENT_F, dtype=torch.float32, device=t_o.device)
    if nulls:
        case.pair.dev.intersect_device(n, t_o.data_ptr(), t_d.data_ptr(), hit.data_ptr(), 0, 0, 0, stream)
    else:
        case.pair.dev.intersect_device(n, t_o.data_ptr(), t_d.data_ptr(), hit.data_ptr(), tri.data_ptr(),
                                       bary.data_ptr(), dist.data_ptr(), stream)
    torch.cuda.synchronize()
    return {"hit": hit.cpu().numpy().view(np.uint32), "tri": tri.cpu().numpy().view(np.uint32),
            "bary": bary.cpu().numpy(), "dist": dist.cpu().numpy()}


def shadow(case, idx=None, stream=0):
    import torch
    sel = (lambda t: t) if idx is None else (lambda t: t[idx].contiguous())
    t_o, t_d, t_l, t_i = sel(case.t_o), sel(case.t_d), sel(case.t_limit), sel(case.t_light)
    n = t_o.shape[0]
    occ = torch.full((n,), SENT_U, dtype=torch.int32, device=t_o.device)
    case.pair.dev.intersect_shadow_device(n, t_o.data_ptr(), t_d.data_ptr(), t_l.data_ptr(), t_i.data_ptr(),
                                          occ.data_ptr(), stream)
    torch.cuda.synchronize()
    return occ.cpu().numpy().view(np.uint32)


def check_closest(case, got, idx=None, what=""):
    """hit everywhere; tri, bary, dist bit for bit on hits and the sentinel on misses."""
    want = case.want if idx is None else {k: v[idx] for k, v in case.want.items()}
    assert np.array_equal(got["hit"], want["hit"]), what
    h = want["hit"] == 1
    assert np.array_equal(got["tri"][h], want["tri"][h]), what
    assert np.array_equal(got["bary"][h].view(np.uint32), want["bary"][h].view(np.uint32)), what
    assert np.array_equal(got["dist"][h].view(np.uint32), want["dist"][h].view(np.uint32)), what
    assert (got["tri"][~h] == SENT_U).all(), what
    assert (got["bary"][~h] == np.float32(SENT_F)).all() and (got["dist"][~h] == np.float32(SENT_F)).all(), what


def check_shadow(case, got, idx=None, what=""):
    want = case.want_occ if idx is None else case.want_occ[idx]
    assert np.array_equal(got, want), what


def test_bitexact_vs_oracle_and_legacy(case):
    """The trace path (automatic routing: the default build inside the coordinate bound, the kernels without
    the leaf cull outside) against the oracle and the legacy entry points, untouched-on-miss included."""
    case.options(query_trace_min=0)
    got = closest(case)
    check_closest(case, got, what="closest vs oracle")
    legacy = case.pair.dev.intersect(case.o, case.d)
    h = legacy["hit"] == 1
    assert np.array_equal(got["hit"], legacy["hit"])
    for k in ("tri", "bary", "dist"):
        assert np.array_equal(got[k][h].view(np.uint32), legacy[k][h].view(np.uint32)), k
    occ = shadow(case)
    check_shadow(case, occ, what="shadow vs oracle")
    assert np.array_equal(occ, case.pair.dev.intersect_shadow(case.o, case.d, case.limit, case.light))


@pytest.mark.parametrize("route", [0, 1, 2])
@pytest.mark.parametrize("sort", [0, 1])
def test_routes_and_sort_agree(case, route, sort):
    """Identical output arrays (sentinels on misses included) under every route and queue order."""
    case.options(query_trace_min=0, query_route=route, query_sort=sort)
    check_closest(case, closest(case), what="route %d sort %d" % (route, sort))
    check_shadow(case, shadow(case), what="route %d sort %d" % (route, sort))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257])
def test_small_sizes(case, n):
    """Partial waves and blocks through the trace path; the rays are spread over the whole set so that every
    kind (axis-parallel, on split planes, unit, outside) takes part."""
    case.options(query_trace_min=0)
    idx = np.linspace(0, N - 1, n).astype(np.int64)
    check_closest(case, closest(case, idx), idx, "n %d" % n)
    check_shadow(case, shadow(case, idx), idx, "n %d" % n)


def test_around_trace_min(case):
    """One batch just below query_trace_min (the per-thread kernel whole) and one just above (traced)."""
    case.options(query_trace_min=1000)
    for n in (999, 1001):
        idx = np.arange(N - n, N)
        check_closest(case, closest(case, idx), idx, "n %d" % n)
        check_shadow(case, shadow(case, idx), idx, "n %d" % n)


@pytest.mark.parametrize("route", [0, 1])
def test_several_chunks(case, route):
    """5000 rays in chunks of 1024: four full chunks and a ragged last one of 904."""
    case.options(query_trace_min=0, query_chunk=1024, query_route=route)
    idx = np.arange(5000) % N
    check_closest(case, closest(case, idx), idx, "chunks")
    check_shadow(case, shadow(case, idx), idx, "chunks")


def test_null_outputs_accepted(case):
    case.options(query_trace_min=0)
    got = closest(case, nulls=True)
    assert np.array_equal(got["hit"], case.want["hit"])
    case.options(query_route=1)
    got = closest(case, nulls=True)
    assert np.array_equal(got["hit"], case.want["hit"])


def test_tensor_methods(case):
    """Device.intersect_tensors / intersect_shadow_tensors: torch tensors in and out, torch's current stream."""
    import torch
    case.options(query_trace_min=0)
    r = case.pair.dev.intersect_tensors(case.t_o, case.t_d)
    occ = case.pair.dev.intersect_shadow_tensors(case.t_o, case.t_d, case.t_limit, case.t_light)
    torch.cuda.synchronize()
    h = case.want["hit"] == 1
    assert np.array_equal(r["hit"].cpu().numpy().view(np.uint32), case.want["hit"])
    assert np.array_equal(r["tri"].cpu().numpy().view(np.uint32)[h], case.want["tri"][h])
    assert np.array_equal(r["dist"].cpu().numpy().view(np.uint32)[h], case.want["dist"][h].view(np.uint32))
    assert np.array_equal(r["bary"].cpu().numpy().view(np.uint32)[h], case.want["bary"][h].view(np.uint32))
    assert np.array_equal(occ.cpu().numpy().view(np.uint32), case.want_occ)
    with pytest.raises(ValueError):
        case.pair.dev.intersect_tensors(case.t_o.cpu(), case.t_d)


def test_stream_order(case):
    """Inputs produced by a torch op on a non-default stream, the query on that stream, the outputs consumed
    by a torch op on it, one synchronisation at the end; then a larger batch (the buffers regrow) and a call
    on another stream directly after it."""
    import torch
    case.options(query_trace_min=0)
    dev = case.t_o.device
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    n1 = 1024
    half_o, half_d = (0.5 * case.t_o[:n1]).contiguous(), (0.5 * case.t_d[:n1]).contiguous()
    rep = torch.arange(3 * N, device=dev) % N
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        o1, d1 = half_o + half_o, half_d * 2.0  # exactly the rays again (x / 2 * 2 and x / 2 + x / 2 are exact)
        r1 = case.pair.dev.intersect_tensors(o1, d1)
        hits1 = r1["hit"].sum()
        tri1 = r1["tri"] + 0
        # a larger batch on the same stream: the query buffers regrow
        o2, d2 = case.t_o[rep].contiguous(), case.t_d[rep].contiguous()
        r2 = case.pair.dev.intersect_tensors(o2, d2)
        hits2 = r2["hit"].sum()
    with torch.cuda.stream(s2):
        # another stream, directly after (its inputs were ready before s1 started)
        r3 = case.pair.dev.intersect_shadow_tensors(case.t_o, case.t_d, case.t_limit, case.t_light)
        occ3 = r3.sum()
    torch.cuda.synchronize()
    want = case.want
    assert int(hits1.item()) == int(want["hit"][:n1].sum())
    h = want["hit"][:n1] == 1
    assert np.array_equal(tri1.cpu().numpy().view(np.uint32)[h], want["tri"][:n1][h])
    assert np.array_equal(r1["dist"].cpu().numpy().view(np.uint32)[h], want["dist"][:n1][h].view(np.uint32))
    assert int(hits2.item()) == 3 * int(want["hit"].sum())
    idx = rep.cpu().numpy()
    assert np.array_equal(r2["hit"].cpu().numpy().view(np.uint32), want["hit"][idx])
    h2 = want["hit"][idx] == 1
    assert np.array_equal(r2["dist"].cpu().numpy().view(np.uint32)[h2], want["dist"][idx][h2].view(np.uint32))
    assert int(occ3.item()) == int(case.want_occ.sum())
    assert np.array_equal(r3.cpu().numpy().view(np.uint32), case.want_occ)


@pytest.mark.parametrize("counting", [0, 1])
def test_render_is_not_disturbed(ca, cornell, counting):
    """A render, a query, the render again: identical frames, and cr_get_counters after the render is what it
    was without the query (the queries keep counters of their own).  Lean build (option "counters" 0): the
    whole struct is compared after the second render.  Counting build: the whole struct directly after the
    query; after the second render the per-query tallies -- its wave_* fields count what the persistent
    waves happened to do between refills, and the test shows that by its own control, two renders with no
    query between them, which are held to exactly the same comparison."""
    cornell.options(query_trace_min=0)
    dev = cornell.pair.dev
    dev.set_option("counters", counting)
    try:
        cam = cornell.pair.camera(ca, 64, 64)
        p = ca.render_params(64, 64, 4, 6, 77)
        keys = WORK_KEYS if counting else None

        def same(x, y):
            return x == y if keys is None else {k: x[k] for k in keys} == {k: y[k] for k in keys}

        a = dev.render(cam, p)
        c0 = dev.counters()
        a2 = dev.render(cam, p)  # the control: no query in between
        assert_bitwise(a, a2, "render twice")
        assert same(dev.counters(), c0)
        c1 = dev.counters()
        check_closest(cornell, closest(cornell))
        assert dev.counters() == c1  # the query leaves the last render's counters alone, every field
        check_shadow(cornell, shadow(cornell))
        assert dev.counters() == c1
        b = dev.render(cam, p)
        assert_bitwise(a, b, "render after a query")
        assert same(dev.counters(), c0)
        if not counting:
            assert c0["closest"] > 0 and c0["shadow"] > 0  # (the lean build's tallies are not all zero)
    finally:
        dev.set_option("counters", 1)
        cornell.options()


def test_inside_coordinate_bound_outside_padded_box(case):
    """Origins with every |o_i| <= db that lie more than 1 outside the padded root box on a short axis: the
    leaf cull's fixed pads were not derived for them (smax = the largest extent + 2), so they take the
    kernels without the leaf cull.  Unit directions aimed into the box, so a leaf-cull build would evaluate
    its records for them."""
    import torch
    case.options(query_trace_min=0)
    e = case.pair.oracle.kd_export()
    lo, hi = e["box"][:3].astype(np.float64), e["box"][3:].astype(np.float64)
    db = (max(1.0, float(np.abs(e["box"]).max()) + 1.0)) * 1.0001
    room = np.minimum(db - (hi + 1.0), (lo - 1.0) + db)  # per axis: the shell between the widened box and +-db
    ax = int(np.argmax(room))
    if room[ax] < 1e-3:
        pytest.skip("the scene's box leaves no room inside its coordinate bound")
    rng = np.random.default_rng(77)
    n = 512
    o = lo + (hi - lo) * rng.random((n, 3))
    side = rng.random(n) < 0.5
    gap_hi, gap_lo = db - (hi[ax] + 1.0), (lo[ax] - 1.0) + db
    f = 0.05 + 0.9 * rng.random(n)
    o[:, ax] = np.where((side & (gap_hi > 1e-3)) | (gap_lo <= 1e-3), hi[ax] + 1.0 + f * gap_hi, lo[ax] - 1.0 - f * gap_lo)
    o = o.astype(np.float32)
    assert (np.abs(o) <= np.float32(db)).all()
    assert ((o[:, ax] > np.float32(hi[ax] + 1.0)) | (o[:, ax] < np.float32(lo[ax] - 1.0))).all()
    target = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    d = (target - o).astype(np.float32)
    d = (d / np.sqrt((d * d).sum(axis=1, dtype=np.float32), dtype=np.float32)[:, None]).astype(np.float32)
    want = case.pair.oracle.intersect(o, d)
    assert (want["hit"] == 1).sum() > n // 4
    t_o, t_d = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0")
    for route in (0, 2):
        case.options(query_trace_min=0, query_route=route)
        r = case.pair.dev.intersect_tensors(t_o, t_d)
        torch.cuda.synchronize()
        h = want["hit"] == 1
        assert np.array_equal(r["hit"].cpu().numpy().view(np.uint32), want["hit"])
        assert np.array_equal(r["tri"].cpu().numpy().view(np.uint32)[h], want["tri"][h])
        assert np.array_equal(r["bary"].cpu().numpy().view(np.uint32)[h], want["bary"][h].view(np.uint32))
        assert np.array_equal(r["dist"].cpu().numpy().view(np.uint32)[h], want["dist"][h].view(np.uint32))


def test_errors(ca, cornell):
    import torch
    hip = ca.libs()[0]
    t = torch.zeros((4, 3), dtype=torch.float32, device="cuda:0")
    u = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    P = ctypes.c_void_p
    c = cornell.pair.dev._c
    # n == 0: nothing to do, whatever the pointers
    assert hip.cr_intersect_device(c, 0, None, None, None, None, None, None, None) == ca.CR_OK
    assert hip.cr_intersect_shadow_device(c, 0, None, None, None, None, None, None) == ca.CR_OK
    # a null required pointer
    for args in ((None, P(t.data_ptr()), P(u.data_ptr())), (P(t.data_ptr()), None, P(u.data_ptr())),
                 (P(t.data_ptr()), P(t.data_ptr()), None)):
        assert ca.CR_ERRORS.get(hip.cr_intersect_device(c, 4, *args, None, None, None, None)) == "CR_E_INVALID"
    f = torch.zeros(4, dtype=torch.float32, device="cuda:0")
    for dp, lp in ((None, P(u.data_ptr())), (P(f.data_ptr()), None)):
        rc = hip.cr_intersect_shadow_device(c, 4, P(t.data_ptr()), P(t.data_ptr()), dp, lp, P(u.data_ptr()), None)
        assert ca.CR_ERRORS.get(rc) == "CR_E_INVALID"
    assert ca.CR_ERRORS.get(hip.cr_intersect_device(c, 0xffffffff, P(t.data_ptr()), P(t.data_ptr()), P(u.data_ptr()),
                                                    None, None, None, None)) == "CR_E_INVALID"
    # a ctx with a device and no scene
    bare = ca.Device(0)
    rc = hip.cr_intersect_device(bare._c, 4, P(t.data_ptr()), P(t.data_ptr()), P(u.data_ptr()), None, None, None, None)
    assert ca.CR_ERRORS.get(rc) == "CR_E_NOSCENE"
    assert hip.cr_last_error(bare._c)
