"""The camera packet's unanimous kd steps (csrc/wavefront.hip wf_trace_packet) on the GPU.

A step at which every active ray of the packet takes the same single child is decided once per packet, from
the hull of the live rays' direction components and two bounds over the active rays' intervals.  Every case
renders with the switch `wf_packet_unanimous` at 1 and at 0 (every step per lane) and compares the frames as
uint32 with each other and with the oracle, and the lean counters with each other and with the oracle's: the
cornell box (trace build 44) and the torture scene of tests/torture.py (build 59), packets of one pixel
(128 spp), packets that straddle pixels and tile rows (1, 4, 100 spp), an axis-parallel view whose direction
components are 0 or change sign inside packets, an eye one ulp off a split plane and one exactly on it (the
per-lane camera trace), a frame with partial tiles, a 2-layer pass group in 2 frame pieces, and the
performed-work build.  tests/test_packet_unanimous.py checks the scheme itself on the CPU.
"""
import numpy as np
import pytest

import torture
from helpers import Pair, assert_bitwise

pytestmark = pytest.mark.gpu

SEED, K = 0xC41A05C0, 6
LEAN_KEYS = ("closest", "shadow", "hit", "texhit", "paths")


@pytest.fixture(scope="module")
def pairs(ca, po, scenes, tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            if name == "cornell":
                made[name] = (Pair(ca, po, scenes.config_rtc("cornell")), 44)
            else:
                made[name] = (torture.pair(ca, po, scenes, tmp_path_factory.mktemp("unanimous"), "full", "origin"), 59)
            made[name][0].dev.set_option("kernel", 2)
        return made[name]

    yield get
    made.clear()


def _both(ca, pair, cam, xres, yres, spp, seed=SEED, perf=False):
    """The lean (or performed-work) render with the switch at 1 and at 0: frames, counters, perf, build."""
    dev, out = pair.dev, []
    dev.set_option("counters", 0)
    dev.set_option("perf_counters", 1 if perf else 0)
    try:
        for sw in (1, 0):
            dev.set_option("wf_packet_unanimous", sw)
            g = dev.render(cam, ca.render_params(xres, yres, spp, K, seed))
            out.append((g, dev.counters(), dev.perf() if perf else None, dev.last_trace_build(),
                        dev.trace_stats()["camera"]["launches"]))
    finally:
        dev.set_option("wf_packet_unanimous", 1)
        dev.set_option("perf_counters", 0)
        dev.set_option("counters", 1)
    return out


def _check(ca, pair, cam, xres, yres, spp, what, seed=SEED, build=None):
    (g1, c1, _, b1, l1), (g0, c0, _, b0, _) = _both(ca, pair, cam, xres, yres, spp, seed)
    o, oc = pair.oracle.render(cam.as_array(), xres, yres, spp, K, seed)
    assert l1 == 1, what  # the camera trace ran as its own launch
    if build is not None:
        assert b1 == build and b0 == build, (what, b1, b0)
    assert_bitwise(g1, g0, what + ": switch 1 vs 0")
    assert_bitwise(g1, o, what + ": vs oracle")
    assert {k: c1[k] for k in LEAN_KEYS} == {k: c0[k] for k in LEAN_KEYS} == {k: oc[k] for k in LEAN_KEYS}, what


# 128 spp: a packet is one pixel's samples; 1 / 4 / 100: packets straddle pixels, tiles and tile rows.  61 x 37
# and 23 x 13 leave partial tiles (dead slots in the last packets of a tile row)
@pytest.mark.parametrize("spp,res", [(1, (96, 54)), (4, (61, 37)), (100, (23, 13)), (128, (24, 14))])
@pytest.mark.parametrize("scene", ["cornell", "torture"])
def test_unanimous_steps_bitexact(ca, pairs, scene, spp, res):
    pair, build = pairs(scene)
    cam = pair.camera(ca, *res) if scene == "cornell" else ca.camera(*torture.cameras(pair.soup)["room"], *res)
    _check(ca, pair, cam, res[0], res[1], spp, "%s %dx%dx%d" % (scene, res[0], res[1], spp), build=build)


@pytest.mark.parametrize("scene", ["cornell", "torture"])
def test_axis_parallel_view(ca, pairs, scene):
    """The view direction along -z (and along +x) from inside the scene: the middle columns' and rows' rays
    have x / y components that are 0 or change sign inside a packet, so those axis hulls are unusable."""
    pair, build = pairs(scene)
    lo, hi = np.array(list(pair.desc.box_min), np.float64), np.array(list(pair.desc.box_max), np.float64)
    eye = lo + (hi - lo) * np.array([0.5013, 0.4171, 0.8207])
    for i, look in enumerate((eye + np.array([0, 0, -1.0]) * (hi - lo)[2], eye + np.array([1.0, 0, 0]) * (hi - lo)[0])):
        for (x, y, s) in ((48, 28, 4), (17, 9, 128)):
            cam = ca.camera(eye, look, (0, 1, 0), 1.1, x, y)
            _check(ca, pair, cam, x, y, s, "%s axis-parallel view %d %dx%dx%d" % (scene, i, x, y, s), build=build)


@pytest.mark.parametrize("scene", ["cornell", "torture"])
def test_eye_next_to_and_on_a_split_plane(ca, pairs, scene):
    """An eye one ulp either side of a split plane of each axis (the packet trace: the numerator split - eye is
    one ulp) and exactly on it (the host hands that render to the per-lane camera trace)."""
    pair, _ = pairs(scene)
    e = pair.kd.export()
    lo, hi = np.array(list(pair.desc.box_min)), np.array(list(pair.desc.box_max))
    for axis in range(3):
        inner = np.nonzero((e["is_leaf"] == 0) & (e["axis"] == axis))[0]
        split = np.float32(e["split"][inner[len(inner) // 2]])
        for k, v in enumerate((np.nextafter(split, np.float32(-np.inf)), np.nextafter(split, np.float32(np.inf)), split)):
            eye = ((lo + hi) / 2).astype(np.float32)
            eye[axis] = v
            look = eye + np.array([0.31, -0.2, 0.93]) * (hi - lo).max()
            cam = ca.camera(eye, look, (0, 1, 0), 1.4, 40, 30)
            assert cam.as_array()[axis] == v
            _check(ca, pair, cam, 40, 30, 4, "%s eye at split %+d ulp, axis %d" % (scene, (-1, 1, 0)[k], axis), seed=77 + axis)


@pytest.mark.parametrize("scene", ["cornell", "torture"])
def test_pass_group_in_pieces(ca, pairs, scene):
    """A 2-layer pass group in 2 frame pieces, blended on the device (the path the benchmark's timed groups
    take), with the switch at 1 and at 0."""
    import torch
    pair, build = pairs(scene)
    xres, yres, spp, nl, pieces = 61, 37, 3, 2, 2
    cam = pair.camera(ca, xres, yres) if scene == "cornell" else ca.camera(*torture.cameras(pair.soup)["room"], xres, yres)
    frames = []
    pair.dev.set_option("counters", 0)
    try:
        for sw in (1, 0):
            pair.dev.set_option("wf_packet_unanimous", sw)
            frame = torch.zeros((yres, xres, 3), dtype=torch.float32, device="cuda:0")
            for piece in range(pieces):
                q = ca.render_params(xres, yres, spp, K, SEED, layer=1, rank=piece, nranks=pieces)
                pair.dev.render_layers_device(cam, q, nl, frame.data_ptr(), 0)
                assert pair.dev.last_trace_build() == build
            torch.cuda.synchronize()
            frames.append(frame.cpu().numpy())
    finally:
        pair.dev.set_option("wf_packet_unanimous", 1)
        pair.dev.set_option("counters", 1)
    o = np.zeros((yres, xres, 3), np.float32)
    for layer in range(1, nl + 1):
        pair.oracle.render(cam.as_array(), xres, yres, spp, K, SEED, layer=layer, pixels=o)
    assert_bitwise(frames[0], frames[1], scene + " pieces: switch 1 vs 0")
    assert_bitwise(frames[0], o, scene + " pieces: vs oracle")


@pytest.mark.parametrize("scene", ["cornell", "torture"])
def test_performed_work_counts_unchanged(ca, pairs, scene):
    """The performed-work build: a ray active at a level counts one step whoever decided it, so the camera
    trace's steps / leaves / tests (and its queries) are the same with the switch at 1 and at 0."""
    pair, _ = pairs(scene)
    x, y, s = 48, 27, 16
    cam = pair.camera(ca, x, y) if scene == "cornell" else ca.camera(*torture.cameras(pair.soup)["room"], x, y)
    (g1, c1, p1, _, _), (g0, c0, p0, _, _) = _both(ca, pair, cam, x, y, s, perf=True)
    assert_bitwise(g1, g0, scene + " performed-work build: switch 1 vs 0")
    assert p1["camera"]["steps"] > 0 and p1["camera"]["leaves"] > 0 and p1["camera"]["tests"] > 0
    for k in ("queries", "steps", "leaves", "tests", "waves"):
        assert p1["camera"][k] == p0["camera"][k], (scene, k, p1["camera"], p0["camera"])
    assert {k: c1[k] for k in LEAN_KEYS} == {k: c0[k] for k in LEAN_KEYS}
