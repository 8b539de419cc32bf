"""The HIP kernels against what the reference's own compiled code gave (tests/golden/ref_*, tests/refpin.py).

Every other GPU test compares the kernels with the oracle; these compare them with the fixtures directly, so a
misreading shared by oracle.c and the kernels cannot hide.  They read tests/golden/ and the product library only:
neither the reference nor oracle/_ref, and the oracle not at all.

G2  cr_intersect_device / cr_intersect_shadow_device over the fixture rays of every G1 scene, each loaded from
    OBJ as the product loads any scene (its triangles are asserted to be the fixture's, so ids agree): default
    options, every query route and queue order, and the legacy host-array calls.  The queries pick their trace
    build by scene size alone; the trace builds of test_gpu_parity's sweep are covered by G4.
G4  cr_render of the four tiny frames equals the in-order float32 sum and layer blend of the reference's
    per-sample sendRay radiances, for every layer, with sum_staged 0 and 1 and on every build of the sweep.
    Per path: the radiance query (ray mode, one sample) along the reference's own camera ray of sample 0 of
    every pixel, keyed to the pixel's stream, equals that sample's sendRay radiance.
G3  (Diffuse::sample_wi and the two libstdc++ distributions through devmath_check) lives in
    tests/test_gpu_devmath.py, which owns that harness's build.

Bit for bit throughout, on uint32 views.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import refpin
from helpers import assert_bitwise
from test_gpu_parity import TRACE_BUILDS
from test_gpu_queries import DEFAULTS, check_closest, check_shadow, closest, shadow

pytestmark = pytest.mark.gpu


class RefCase:
    """A fixture scene on the device with its closest and shadow ray sets (two views the query helpers of
    test_gpu_queries take) and the reference's answers."""

    def __init__(self, ca, scenes, directory, name):
        import torch
        self.gs = refpin.GoldenScene(name)
        self.loaded = refpin.Loaded(ca, scenes, directory / name, self.gs)
        self.kd = ca.KDTree(self.loaded.model, self.loaded.scene)
        self.dev = ca.Device(0)
        self.dev.upload(self.kd.describe())
        self.dev.set_option("wf_tail_min", 0)
        pair = SimpleNamespace(dev=self.dev)
        r = self.rays = refpin.load_rays(name)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        self.closest = SimpleNamespace(pair=pair, o=r["o"], d=r["d"], t_o=to(r["o"]), t_d=to(r["d"]),
                                       want={"hit": r["hit"], "tri": r["tri"], "bary": refpin.f32(r["bary"]),
                                             "dist": refpin.f32(r["dist"])})
        self.shadow = SimpleNamespace(pair=pair, o=r["so"], d=r["sd"], limit=r["slimit"], light=r["slight"],
                                      t_o=to(r["so"]), t_d=to(r["sd"]), t_limit=to(r["slimit"]),
                                      t_light=to(r["slight"].view(np.int32)), want_occ=r["occ"])

    def options(self, **kw):
        for k, v in {**DEFAULTS, **kw}.items():
            self.dev.set_option(k, v)


@pytest.fixture(scope="module")
def cases(ca, scenes, tmp_path_factory):
    directory = tmp_path_factory.mktemp("refpin")
    made = {}

    def get(name):
        if name not in made:
            made[name] = RefCase(ca, scenes, directory, name)
        made[name].options()
        return made[name]

    yield get
    made.clear()


def _check_queries(c, what):
    check_closest(c.closest, closest(c.closest), what=what + ": closest")
    check_shadow(c.shadow, shadow(c.shadow), what=what + ": shadow")


@pytest.mark.parametrize("name", refpin.SCENES)
def test_g2_queries_match_reference(cases, name):
    """Default options (short batches take the query kernel) and the trace path, against
    KDTree::intersectRay / intersectShadowRay; then the legacy host-array calls."""
    c = cases(name)
    assert c.rays["hit"].sum() > 1000 and 0 < c.rays["occ"].sum() < len(c.rays["occ"])
    try:
        _check_queries(c, name + " default")
        c.options(query_trace_min=0)
        _check_queries(c, name + " trace path")
    finally:
        c.options()
    r = c.rays
    got = c.dev.intersect(r["o"], r["d"])
    assert not refpin.closest_differences(got, r).any(), name
    assert np.array_equal(c.dev.intersect_shadow(r["so"], r["sd"], r["slimit"], r["slight"]), r["occ"]), name


@pytest.mark.parametrize("sort", [0, 1])
@pytest.mark.parametrize("route", [0, 1, 2])
@pytest.mark.parametrize("name", refpin.SCENES)
def test_g2_queries_routes_and_sort_match_reference(cases, name, route, sort):
    c = cases(name)
    try:
        c.options(query_trace_min=0, query_route=route, query_sort=sort)
        _check_queries(c, "%s route %d sort %d" % (name, route, sort))
    finally:
        c.options()


@pytest.fixture(scope="module")
def paths():
    p = refpin.load_paths()
    for c in p.values():
        c["frames"] = refpin.blend_frames(c)
    return p


def _render_layers(ca, c, case, what):
    """cr_render layer after layer into the context's accumulator, each against the fixture's blend."""
    cam = ca.camera(*(c.gs.view[i: i + 3].tolist() for i in (0, 3, 6)), float(c.gs.view[9]), case["xres"], case["yres"])
    # (the camera the reference's glm gave for this view: the fixture's paths were traced through it)
    assert np.array_equal(cam.as_array().view(np.uint32), np.ascontiguousarray(case["cam"], np.float32).view(np.uint32))
    for li in range(case["layers"]):
        p = ca.render_params(case["xres"], case["yres"], case["spp"], case["k"], case["seed"], layer=li + 1,
                             background=tuple(float(v) for v in case["bg"]))
        g = c.dev.render(cam, p, None)
        assert_bitwise(g, case["frames"][li], "%s layer %d" % (what, li + 1))


@pytest.mark.parametrize("staged", [1, 0])
@pytest.mark.parametrize("case", sorted(refpin.PATH_CASES))
def test_g4_render_matches_reference_paths(ca, cases, paths, case, staged):
    c = cases(refpin.PATH_CASES[case])
    assert np.isfinite(paths[case]["frames"][-1]).all() and paths[case]["frames"][-1].max() > 0
    c.dev.set_option("sum_staged", staged)
    try:
        _render_layers(ca, c, paths[case], "%s sum_staged %d" % (case, staged))
    finally:
        c.dev.set_option("sum_staged", 1)


@pytest.mark.parametrize("variant", TRACE_BUILDS)
def test_g4_render_trace_builds_match_reference_paths(ca, cases, paths, variant):
    """Every trace build of test_gpu_parity's sweep (set the same way) on the four frames."""
    for case in sorted(refpin.PATH_CASES):
        c = cases(refpin.PATH_CASES[case])
        c.dev.set_option("kernel", 2)
        c.dev.set_option("variant", variant)
        try:
            _render_layers(ca, c, paths[case], "%s build %d" % (case, variant))
        finally:
            c.dev.set_option("variant", -1)


@pytest.mark.parametrize("case", sorted(refpin.PATH_CASES))
def test_g4_radiance_query_matches_reference_per_path(ca, cases, paths, case):
    """cr_radiance with one sample per ray draws from stream (seed, layer, id0 + i, 0) from counter 2 on: given
    the camera rays the reference made from draws 0 and 1 of sample 0 of pixel i, each value is that one path's
    sendRay radiance (summed from zero, times 1 / 1, blended into a zero frame: layer L gives mean / L)."""
    c, P = cases(refpin.PATH_CASES[case]), paths[case]
    n = P["xres"] * P["yres"]
    orig = np.tile(P["cam"][0:3], (n, 1)).astype(np.float32)
    for li in range(P["layers"]):
        dirs = refpin.f32(P["dir"][li, :, :, 0]).reshape(n, 3)
        r = refpin.f32(P["rad"][li, :, :, 0]).reshape(n, 3)
        zero, L = np.zeros_like(r), np.float32(li + 1)
        with np.errstate(all="ignore"):
            mean = ((zero + r).astype(np.float32) * np.float32(1.0)).astype(np.float32)
            want = mean if li == 0 else (((zero * np.float32(li)).astype(np.float32) + mean).astype(np.float32) / L).astype(np.float32)
        rp = ca.radiance_params(1, P["k"], P["seed"], tuple(float(v) for v in P["bg"]), layer=li + 1, id0=0)
        got = c.dev.radiance(orig, dirs, rp, 1)
        assert_bitwise(got, want, "%s layer %d per path" % (case, li + 1))
