"""The trace kernels' fixed options and point-of-use arguments, bit for bit against the oracle.

The default builds (59 on the sponza stand-in, 44 on nanobox) launch trace instantiations with WfArgs::vis_mark 1,
WfArgs::ended_only 0 and RenderArgs::lc_debug 0 fixed at compile time (wfbuilds.hpp tc::Fixed); any other
value of such an option selects the build's generic kernels.  Every trace instantiation reads the queues,
their counters and order and the result arrays from the kernel-argument segment once per query.  Each case
below takes one of these paths; pixels and per-query counters must equal the oracle's in all of them.
Sizes: those of test_wavefront_trace_builds_bitexact (80 x 45 x 4 spp) and a 64 x 36 x 2 spp nanobox.
"""
import numpy as np
import pytest

from helpers import Pair, assert_bitwise

pytestmark = pytest.mark.gpu

ORACLE_KEYS = ("closest", "shadow", "inner", "leaf", "tritest", "hit", "texhit", "paths")
LEAN_KEYS = ("closest", "shadow", "hit", "texhit", "paths", "pixels")
K, SEED = 6, 0xC41A05C0
SIZES = {"sponza": (80, 45, 4), "nanobox": (64, 36, 2)}
BUILD = {"sponza": 59, "nanobox": 44}
# ctx.hpp defaults of the options the cases change (Pair sets wf_tail_min 0)
DEFAULTS = {"wf_vis_mark": 1, "wf_vis_dw": 1, "wf_tail_overlap": 0, "wf_tail_min": 0, "wf_xcd": 7, "wf_sort": -1,
            "wf_sort_min": 1 << 20, "wf_app_chunk": 0, "wf_lanes": 1, "wf_sort_g1": 3, "wf_tail_waves": 4}


class Case:
    """A scene's Pair with the oracle's frame and counters of its size, rendered once."""

    def __init__(self, ca, po, scenes, name):
        self.name = name
        self.pair = Pair(ca, po, scenes.config_rtc(name))
        self.x, self.y, self.s = SIZES[name]
        self.cam = self.pair.camera(ca, self.x, self.y)
        self.ref, self.ref_counters = self.pair.oracle.render(self.cam.as_array(), self.x, self.y, self.s, K, SEED)
        self.ref.setflags(write=False)
        self.layers = None  # (layers 1 and 2 blended, their closest + shadow queries): the pass-group case, on first use


@pytest.fixture(scope="module")
def cases(ca, po, scenes):
    return {name: Case(ca, po, scenes, name) for name in SIZES}


def check(ca, case, options, what, stats=None):
    """Counting and lean renders with `options` set: both equal the oracle's frame, the counting build's
    counters the oracle's, the lean build's per-query counters the counting build's.  stats (a list): gets each
    of the two renders' (chunked wf_shade launches, trace launches per kind)."""
    dev = case.pair.dev
    dev.set_option("kernel", 2)
    p = ca.render_params(case.x, case.y, case.s, K, SEED)
    try:
        for key, v in options.items():
            dev.set_option(key, v)
        g = dev.render(case.cam, p)
        gc = dev.counters()
        launches = lambda: {kind: v["launches"] for kind, v in dev.trace_stats().items()}
        if stats is not None:
            stats.append((dev.chunked_shades(), launches()))
        dev.set_option("counters", 0)
        g_lean = dev.render(case.cam, p)
        lc = dev.counters()
        if stats is not None:
            stats.append((dev.chunked_shades(), launches()))
        build = dev.last_trace_build()
        chunked = dev.chunked_shades()
    finally:
        dev.set_option("counters", 1)
        for key in options:
            dev.set_option(key, DEFAULTS[key])
    tag = "%s %dx%dx%d %s" % (case.name, case.x, case.y, case.s, what)
    assert_bitwise(g, case.ref, tag + " (counting build)")
    assert_bitwise(g_lean, case.ref, tag + " (lean build)")
    assert {k: gc[k] for k in ORACLE_KEYS} == case.ref_counters, tag
    assert {k: lc[k] for k in LEAN_KEYS} == {k: gc[k] for k in LEAN_KEYS}, tag
    assert build == BUILD[case.name], (tag, build)  # the options change the instantiation, never the build
    return chunked


@pytest.mark.parametrize("scene", ["sponza", "nanobox"])
def test_default_options_fixed_instantiations(ca, cases, scene):
    """All defaults: the tc::Fixed closest and shadow traces of builds 59 / 44."""
    check(ca, cases[scene], {}, "defaults")


@pytest.mark.parametrize("scene", ["sponza", "nanobox"])
@pytest.mark.parametrize("options", [
    {"wf_vis_mark": 0, "wf_vis_dw": 1},                 # results into the dw records
    {"wf_vis_mark": 0, "wf_vis_dw": 0},                 # results into occ[]
    {"wf_tail_overlap": 1, "wf_tail_min": 3000},        # ended_only set for the overlapped generation
], ids=["vis_dw", "occ", "ended_only"])
def test_generic_fallback_one_fixed_option_flipped(ca, cases, scene, options):
    """A non-default value of a fixed option: the generic instantiations, the same bits."""
    check(ca, cases[scene], options, str(options))


@pytest.mark.parametrize("scene", ["sponza", "nanobox"])
@pytest.mark.parametrize("options", [
    {"wf_sort": 1, "wf_sort_min": 0},                   # every queue sorted: order != nullptr
    {"wf_xcd": 0, "wf_sort": 0},                        # the unpartitioned work counter, order == nullptr
    {"wf_app_chunk": 256},                              # dead queue entries: the shadow-dead kernel
    {"wf_lanes": 2},                                    # run_wavefront_lanes' launches
], ids=["sorted", "xcd0_unsorted", "chunked", "lanes2"])
def test_point_of_use_argument_branches(ca, cases, scene, options):
    """The refill's branches whose arguments come from the kernel-argument segment."""
    chunked = check(ca, cases[scene], options, str(options))
    if "wf_app_chunk" in options:
        assert chunked > 0, "the lean render used no chunked appends"


@pytest.mark.parametrize("scene", ["sponza", "nanobox"])
def test_lanes_driver_keeps_its_policy(ca, cases, scene):
    """run_wavefront_lanes ignores wf_sort_g1, never appends in chunks, never overlaps the tail and runs its lean
    tail at 4 waves per SIMD (wfgen.hpp WF_DRIVER_LANES): with those four options set against it, the same
    launches and the same bits."""
    lanes = {"wf_lanes": 2, "wf_tail_min": 3000}
    against = dict(lanes, wf_app_chunk=256, wf_sort_g1=0, wf_tail_overlap=1, wf_tail_waves=6)
    plain, opposed = [], []
    check(ca, cases[scene], lanes, str(lanes), plain)
    check(ca, cases[scene], against, str(against), opposed)
    assert [c for c, _ in plain + opposed] == [0, 0, 0, 0], (plain, opposed)
    assert [l for _, l in plain] == [l for _, l in opposed], (plain, opposed)
    assert sum(plain[1][1].values()) > 0


@pytest.mark.parametrize("scene", ["sponza", "nanobox"])
def test_two_layer_group_in_two_pieces(ca, cases, scene):
    """One pass group of 2 progressive layers cut into 2 frame pieces: launches of the same kernels with
    different w0 / P / order, blended in place on the device."""
    import torch
    case = cases[scene]
    dev = case.pair.dev
    x, y, s, nl, pieces = case.x, case.y, case.s, 2, 2
    if case.layers is None:
        o, rays = np.zeros((y, x, 3), np.float32), 0
        for layer in range(1, nl + 1):
            _, oc = case.pair.oracle.render(case.cam.as_array(), x, y, s, K, SEED, layer=layer, pixels=o)
            rays += oc["closest"] + oc["shadow"]
        o.setflags(write=False)
        case.layers = (o, rays)
    dev.set_option("kernel", 2)
    dev.set_option("counters", 0)
    dev.set_option("wf_sort_min", 0)  # (sorted queues: each piece's launches get their own order)
    try:
        frame = torch.zeros((y, x, 3), dtype=torch.float32, device="cuda:0")
        rays = 0
        for piece in range(pieces):
            q = ca.render_params(x, y, s, K, SEED, layer=1, rank=piece, nranks=pieces)
            dev.render_layers_device(case.cam, q, nl, frame.data_ptr(), 0)
            assert dev.last_trace_build() == BUILD[scene]
            c = dev.counters()
            rays += c["closest"] + c["shadow"]
        torch.cuda.synchronize()
        g = frame.cpu().numpy()
    finally:
        dev.set_option("counters", 1)
        dev.set_option("wf_sort_min", DEFAULTS["wf_sort_min"])
    assert_bitwise(g, case.layers[0], "%s %dx%dx%d, 2 layers in 2 pieces" % (scene, x, y, s))
    assert rays == case.layers[1], (rays, case.layers[1])  # the pieces' queries: the oracle's of both layers
