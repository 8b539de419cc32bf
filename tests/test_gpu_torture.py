"""The trace kernels on the adversarial scenes and rays of tests/torture.py, bit for bit against the oracle.

The kernels' own evaluation of the exactness arguments -- leaf_mask with the reciprocal and the fused grid
planes of the compressed records, tri_test_wave's ballot exits, leaf_exchange's closest reduction on equal
t, the 2^-40 .. 2^40 guards of the short division, the scalar-load paths of wave-uniform leaves -- meets
the inputs the arguments exist for: rays within 2 ulps of an edge, in a triangle's plane, with the limit
at the hit distance, with direction components around 2^-40, in leaves that mix 10-unit and 2^-12
triangles, at the origin and translated so that the scene lies entirely below zero on y (the reference's
FLT_MIN box).  tests/test_torture_oracle.py holds the floors that keep these comparisons from passing
vacuously.  Every comparison is on uint32 views.
"""
import numpy as np
import pytest

import torture
from helpers import assert_bitwise
from test_gpu_queries import DEFAULTS, check_closest, check_shadow, closest, shadow

pytestmark = pytest.mark.gpu

ORACLE_KEYS = ("closest", "shadow", "inner", "leaf", "tritest", "hit", "texhit", "paths")
LEAN_KEYS = ("closest", "shadow", "hit", "texhit", "paths", "pixels")
SCENES = [(d, p) for d in ("full", "mini") for p in ("origin", "translated")]
XRES, YRES, SPP, K, SEED = 48, 36, 4, 6, 0xC41A05C0


class GpuCase(torture.Case):
    def __init__(self, *args):
        import torch
        super().__init__(*args)
        dev = "cuda:0"
        self.t_o, self.t_d = torch.from_numpy(self.o).to(dev), torch.from_numpy(self.d).to(dev)
        self.t_limit = torch.from_numpy(self.limit).to(dev)
        self.t_light = torch.from_numpy(self.light.view(np.int32)).to(dev)
        # one fixed permutation: the class-sorted set's coherent waves become divergent ones
        self.perm = np.random.default_rng(3).permutation(len(self.o))
        self.renders = {}

    def options(self, **kw):
        for k, v in {**DEFAULTS, **kw}.items():
            self.pair.dev.set_option(k, v)

    def oracle_render(self, ca, name):
        """The oracle's layers 1 and 2 of a camera (computed once, handed out as copies' sources)."""
        if name not in self.renders:
            cam = ca.camera(*torture.cameras(self.soup)[name], XRES, YRES)
            o1, c1 = self.pair.oracle.render(cam.as_array(), XRES, YRES, SPP, K, SEED, layer=1)
            o2, c2 = self.pair.oracle.render(cam.as_array(), XRES, YRES, SPP, K, SEED, layer=2, pixels=o1.copy())
            assert np.isfinite(o2).all() and o1.mean() > 0.01
            self.renders[name] = (cam, (o1, c1), (o2, c2))
        return self.renders[name]


@pytest.fixture(scope="module")
def cases(ca, po, scenes, tmp_path_factory):
    directory = tmp_path_factory.mktemp("torture")
    made = {}

    def get(detail, placement, *overrides):
        key = (detail, placement) + overrides
        if key not in made:
            made[key] = GpuCase(ca, po, scenes, directory, detail, placement, *overrides)
        made[key].options()
        return made[key]

    yield get
    made.clear()


def _queries(c, what):
    """Closest and shadow queries over the whole set, class-sorted and permuted: each against the oracle,
    sentinels on misses included, and the two orders equal after un-permuting."""
    a = closest(c)
    check_closest(c, a, what=what + ", class-sorted")
    b = closest(c, c.perm)
    check_closest(c, b, c.perm, what + ", permuted")
    for k in ("hit", "tri", "bary", "dist"):
        assert np.array_equal(a[k][c.perm].view(np.uint32), b[k].view(np.uint32)), (what, k)
    sa = shadow(c)
    check_shadow(c, sa, what=what + ", class-sorted")
    sb = shadow(c, c.perm)
    check_shadow(c, sb, c.perm, what + ", permuted")
    assert np.array_equal(sa[c.perm], sb), what
    return a, sa


@pytest.mark.parametrize("sort", [0, 1])
@pytest.mark.parametrize("route", [0, 1, 2])
@pytest.mark.parametrize("detail,placement", SCENES)
def test_queries_bitexact(cases, detail, placement, route, sort):
    """cr_intersect_device / cr_intersect_shadow_device over the aimed ray set under every route and queue
    order.  The full scenes take the scene-size default build 59 (compressed cull records, leaf exchange),
    the mini ones build 44 and the fat no-cull query kernels."""
    c = cases(detail, placement)
    n = c.pair.dev.scene_triangles()
    assert n >= 65536 if detail == "full" else 1024 <= n < 65536
    try:
        c.options(query_trace_min=0, query_route=route, query_sort=sort)
        _queries(c, "%s %s route %d sort %d" % (detail, placement, route, sort))
    finally:
        c.options()


@pytest.mark.parametrize("detail,placement", SCENES)
def test_queries_equal_legacy(cases, detail, placement):
    """The device-resident calls against the legacy host-array cr_intersect / cr_intersect_shadow."""
    c = cases(detail, placement)
    try:
        c.options(query_trace_min=0)
        got, occ = closest(c), shadow(c)
    finally:
        c.options()
    legacy = c.pair.dev.intersect(c.o, c.d)
    check_closest(c, got, what="device")
    assert np.array_equal(legacy["hit"], c.want["hit"])
    h = legacy["hit"] == 1
    for k in ("tri", "bary", "dist"):
        assert np.array_equal(got[k][h].view(np.uint32), legacy[k][h].view(np.uint32)), k
    assert np.array_equal(occ, c.pair.dev.intersect_shadow(c.o, c.d, c.limit, c.light))
    assert np.array_equal(occ, c.want_occ)


@pytest.mark.parametrize("sort", [0, 1])
@pytest.mark.parametrize("route", [0, 1, 2])
def test_queries_leaf_size_24_bitexact(cases, route, sort):
    """The full scene with kdtree-leaf-size 24: leaves of 17 - 24 references take no packed or compressed
    cull record, so both branches of the leaf cull mask run next to each other."""
    c = cases("full", "origin", "kdtree-leaf-size", "24")
    e = c.pair.oracle.kd_export()
    lc = e["leaf_count"][e["is_leaf"] == 1]
    assert ((lc > 16) & (lc <= 24)).sum() >= 1000 and ((lc >= 1) & (lc <= 16)).sum() >= 1000
    try:
        c.options(query_trace_min=0, query_route=route, query_sort=sort)
        _queries(c, "leaf size 24 route %d sort %d" % (route, sort))
    finally:
        c.options()


def _two_layers_both(ca, c, cam, l1, l2, what, build):
    """Layers 1 and 2 on the same buffers (cr_render blends into the context's accumulator), by the counting
    build and by the lean build, against the oracle's pixels and counters; the lean renders ran trace build
    `build`."""
    dev = c.pair.dev
    got = {}
    try:
        for counting in (1, 0):
            dev.set_option("counters", counting)
            for layer, (o, oc) in ((1, l1), (2, l2)):
                g = dev.render(cam, ca.render_params(XRES, YRES, SPP, K, SEED, layer=layer), None)
                gc = dev.counters()
                name = "%s layer %d (%s build)" % (what, layer, "counting" if counting else "lean")
                assert_bitwise(g, o, name)
                if counting:
                    assert {k: gc[k] for k in ORACLE_KEYS} == oc, name
                    got[layer] = gc
                else:
                    assert {k: gc[k] for k in LEAN_KEYS} == {k: got[layer][k] for k in LEAN_KEYS}, name
                assert dev.last_trace_build() == (-1 if counting else build), name
    finally:
        dev.set_option("counters", 1)


@pytest.mark.parametrize("variant", [0, 18, 26, 44, 49, 59])
@pytest.mark.parametrize("camera", ["room", "floor", "wall"])
@pytest.mark.parametrize("placement", ["origin", "translated"])
def test_renders_bitexact(ca, cases, placement, camera, variant):
    """48 x 36 x 4 spp, k 6, layers 1 and 2 on the same buffers: the room view, an eye exactly in the
    floor's plane looking along it and an eye exactly in the x = 0 wall's plane (the camera cull boxes and
    the packet trace with every primary ray starting on a split plane), every queue sorted."""
    c = cases("full", placement)
    cam, l1, l2 = c.oracle_render(ca, camera)
    dev = c.pair.dev
    dev.set_option("kernel", 2)
    dev.set_option("variant", variant)
    dev.set_option("wf_sort_min", 0)
    try:
        what = "%s %s build %d" % (placement, camera, variant)
        _two_layers_both(ca, c, cam, l1, l2, what, variant)
    finally:
        dev.set_option("variant", -1)
        dev.set_option("wf_sort_min", 1 << 20)


@pytest.mark.parametrize("detail,placement", SCENES)
def test_render_default_build_by_size(ca, cases, detail, placement):
    """The scene-size defaults: trace build 59 on the full scenes, build 44 (no leaf cull, desc_quorum 0)
    on the mini ones."""
    c = cases(detail, placement)
    cam, l1, l2 = c.oracle_render(ca, "room")
    c.pair.dev.set_option("kernel", 2)
    _two_layers_both(ca, c, cam, l1, l2, "%s %s default build" % (detail, placement), 59 if detail == "full" else 44)


@pytest.mark.parametrize("placement", ["origin", "translated"])
def test_render_tail_kernel_bitexact(ca, cases, placement):
    """The same frame with every generation after the first in the tail kernel (wf_tail_min 1 << 30)."""
    c = cases("full", placement)
    cam, l1, l2 = c.oracle_render(ca, "room")
    dev = c.pair.dev
    dev.set_option("kernel", 2)
    dev.set_option("wf_tail_min", 1 << 30)
    try:
        _two_layers_both(ca, c, cam, l1, l2, placement + " tail kernel", 59)
    finally:
        dev.set_option("wf_tail_min", 0)


@pytest.mark.parametrize("placement", ["origin", "translated"])
def test_render_tile_split_bitexact(ca, cases, placement):
    """The frame as 3 ranks with 16-pixel tiles render it, blended on the root."""
    import torch
    c = cases("full", placement)
    cam, (o1, _), _ = c.oracle_render(ca, "room")
    dev = c.pair.dev
    nranks, tile = 3, 16
    p0 = ca.render_params(XRES, YRES, SPP, K, SEED, nranks=nranks, tile=tile)
    maxt = ca.Device.tiles_for_rank(p0, 0)
    gathered = torch.zeros((nranks, maxt, tile, tile, 3), dtype=torch.float32, device="cuda")
    for r in range(nranks):
        dev.render_tiles_device(cam, ca.render_params(XRES, YRES, SPP, K, SEED, rank=r, nranks=nranks, tile=tile),
                                gathered[r].data_ptr())
    frame = torch.zeros((YRES, XRES, 3), dtype=torch.float32, device="cuda")
    dev.blend_tiles_device(p0, gathered.data_ptr(), frame.data_ptr())
    torch.cuda.synchronize()
    assert_bitwise(frame.cpu().numpy(), o1, placement + " 3 ranks x tile 16")


@pytest.mark.parametrize("placement", ["origin", "translated"])
def test_leaf_exchange_multi_window_rounds_ran(ca, cases, placement):
    """Build 54 with the performed-work counters on the full scene: the same bits, and exchange rounds of
    more than one 64-pair window really ran in the secondary closest and the shadow trace."""
    c = cases("full", placement)
    cam, (o1, _), _ = c.oracle_render(ca, "room")
    dev = c.pair.dev
    dev.set_option("kernel", 2)
    dev.set_option("variant", 54)
    dev.set_option("wf_sort_min", 0)
    dev.set_option("counters", 0)
    dev.set_option("perf_counters", 1)
    try:
        g = dev.render(cam, ca.render_params(XRES, YRES, SPP, K, SEED, layer=1), None)
        perf = dev.perf()
    finally:
        dev.set_option("perf_counters", 0)
        dev.set_option("counters", 1)
        dev.set_option("variant", -1)
        dev.set_option("wf_sort_min", 1 << 20)
    assert_bitwise(g, o1, placement + " performed-work build 54")
    for kind in ("closest", "shadow"):
        pk = perf[kind]
        assert pk["drounds"] > 0 and pk["diters"] > pk["drounds"], (kind, pk)
