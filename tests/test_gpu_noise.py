"""The noise estimate on the GPU (include/chiaro_hip.h "noise estimate"), bit for bit:

* the moment frame the sum kernels keep beside the frame against the oracle -- every sample's radiance from
  or_path, squared and summed in float32 in sample order, blended as the frame is;
* noise_eval against the numpy float32 restatement of the per-pixel error;
* cr_render_until's stop layer, statistic and frame against the oracle's own sequence.

References are computed once per shape (REF) and shared; nothing here changes them."""
import subprocess

import numpy as np
import pytest

from helpers import Pair, assert_bitwise

pytestmark = pytest.mark.gpu

SEED, K = 0xC41A05C0, 6
F32 = np.float32
FLOOR = 1e-3
# cr_render_until on cornell 32x32 x 4 spp (test 6): a pixel counts while its error (relative to brightness +
# UNTIL_FLOOR) is above UNTIL_T, and the render stops once at most UNTIL_ABOVE pixels do.  Fixed from the
# oracle's own sequence -- `above` after layers 1..6 is 108, 99, 75, 64, 57, 53, so the oracle alone stops at
# layer 3, and at layer 4 when it checks every second layer (test_render_until_stop_layer asserts that it stops
# strictly between layers 2 and 5 before it looks at the GPU).  With 4 samples per layer and a floor near zero
# the count still GROWS over these layers -- dark pixels with no lit sample yet report no variance at all -- so
# the floor is part of the fixture.
UNTIL_T, UNTIL_FLOOR, UNTIL_ABOVE = 0.25, 0.25, 80
# the CLI's `noise T` (max_above 0, floor 1e-3): cornell 12x12 x 64 spp, where the oracle's max_err after layers
# 1..6 is 0.890, 0.759, 0.758, 0.657, 0.596, 0.575 -- it first falls to T at layer 4 (asserted to lie inside 2..5)
CLI_T, CLI_X, CLI_Y, CLI_SPP = 0.7, 12, 12, 64

_REF = {}
_PAIRS = {}


def _pair(ca, po, scenes, name):
    if name not in _PAIRS:
        _PAIRS[name] = Pair(ca, po, scenes.config_rtc(name))
    return _PAIRS[name]


@pytest.fixture(scope="module")
def pairs(ca, po, scenes):
    yield lambda name: _pair(ca, po, scenes, name)
    for p in _PAIRS.values():
        p.dev.close()
    _PAIRS.clear()


def oracle_moments(ca, pair, x, y, spp, layers):
    """[(frame_L, m2_L) for L = 1..layers]: the oracle's frame, and the moment frame restated from or_path --
    q = (((0 + r_0 * r_0) + r_1 * r_1) + ...) per channel in float32, m2 = (m2 * (L-1) + q * (1/spp)) / L."""
    cam = pair.camera(ca, x, y).as_array()
    bg = (0.0, 0.0, 0.0)
    out, frame, m2 = [], None, np.zeros((y, x, 3), F32)
    inv = F32(1.0) / F32(spp)
    for layer in range(1, layers + 1):
        frame, _ = pair.oracle.render(cam, x, y, spp, K, SEED, layer=layer,
                                      pixels=None if frame is None else frame.copy())
        q, t = np.zeros((y, x, 3), F32), np.zeros((y, x, 3), F32)
        r = np.zeros((y, x, 3), F32)
        for s in range(spp):
            for py in range(y):
                for px in range(x):
                    r[py, px] = pair.oracle.path(cam, x, y, K, bg, SEED, layer, px, py, s)
            t = t + r
            q = q + r * r
        m2 = (m2 * F32(layer - 1) + q * inv) / F32(layer)
        # the samples are the ones the frame is made of: their plain sum blends to the oracle's frame
        prev = out[-1][0] if out else np.zeros((y, x, 3), F32)
        assert_bitwise((prev * F32(layer - 1) + t * inv) / F32(layer), frame, "or_path samples vs or_render")
        out.append((frame, m2.copy()))
    return out


def ref(ca, pairs, name, x, y, spp, layers):
    key = (name, x, y, spp)
    if key not in _REF or len(_REF[key]) < layers:
        _REF[key] = oracle_moments(ca, pairs(name), x, y, spp, layers)
    return _REF[key][:layers]


def noise_ref(frame, m2, layers, spp, threshold, floor):
    """The per-pixel error and the frame statistic, restated in numpy float32 in the header's operation order."""
    with np.errstate(all="ignore"):
        f, q, n = np.asarray(frame, F32), np.asarray(m2, F32), F32(layers * spp)
        v = q - f * f
        v = np.where(v > 0, v, F32(0))
        se = np.sqrt(v / n)
        err = ((se[..., 0] + se[..., 1]) + se[..., 2]) / (((f[..., 0] + f[..., 1]) + f[..., 2]) + F32(floor))
        err = np.where(np.isnan(err), F32(0), err).astype(F32)
        pos = err[err > 0]
        stats = {"pixels": int(err.size), "above": int((err > F32(threshold)).sum()),
                 "max_err": float(pos.max()) if pos.size else 0.0, "layers": int(layers)}
    return err, stats


POISON = 0x7FC0DEAD  # a NaN payload: any write shows


class Guarded:
    """A device buffer [y][x][3] between two poisoned guard bands."""

    def __init__(self, y, x, guard=4096, fill=None):
        import torch
        self.n, self.g = y * x * 3, guard
        self.t = torch.full((self.n + 2 * guard,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        self.body = self.t[guard:guard + self.n].view(y, x, 3)
        if fill is not None:
            self.body.fill_(fill)
        self.ptr = self.body.data_ptr()

    def numpy(self):
        return self.body.cpu().numpy()

    def assert_guards(self, what):
        import torch
        bits = self.t.view(torch.int32).cpu().numpy()
        assert (bits[:self.g] == POISON).all() and (bits[self.g + self.n:] == POISON).all(), what + ": guard band"


def render_single_layers(ca, dev, cam, x, y, spp, layers, **kw):
    """Layers 1..layers as single cr_render_layers_noise_device calls -> [(frame, m2)] after each."""
    import torch
    fr, mo = Guarded(y, x), Guarded(y, x)
    out = []
    for layer in range(1, layers + 1):
        p = ca.render_params(x, y, spp, K, SEED, layer=layer, **kw)
        dev.render_layers_noise_device(cam, p, 1, fr.ptr, mo.ptr, 0)
        torch.cuda.synchronize()
        out.append((fr.numpy(), mo.numpy()))
    fr.assert_guards("frame")
    mo.assert_guards("m2")
    return out


# --- 1. single layers, both sum kernels --------------------------------------------------------------------

@pytest.mark.parametrize("name,x,y,spp,staged", [
    ("cornell", 24, 16, 4, 1),    # sum_samples_lds: s_count % 4 == 0
    ("cornell", 24, 16, 5, 1),    # the thread-per-pixel kernel: s_count % 4 != 0
    ("nanobox", 20, 12, 20, 1),   # textured; the stage of 16 samples is straddled
    ("nanobox", 20, 12, 20, 0),   # the same through the thread-per-pixel kernel
    ("sponza", 32, 18, 8, 1),
])
def test_single_layers_both_sum_kernels(ca, pairs, name, x, y, spp, staged):
    pair = pairs(name)
    want = ref(ca, pairs, name, x, y, spp, 3)
    pair.dev.set_option("sum_staged", staged)
    try:
        got = render_single_layers(ca, pair.dev, pair.camera(ca, x, y), x, y, spp, 3)
    finally:
        pair.dev.set_option("sum_staged", 1)
    for layer, ((gf, gm), (of, om)) in enumerate(zip(got, want), 1):
        assert_bitwise(gf, of, "%s %dx%dx%d frame, layer %d" % (name, x, y, spp, layer))
        assert_bitwise(gm, om, "%s %dx%dx%d m2, layer %d" % (name, x, y, spp, layer))
    assert float(got[-1][1].mean()) > 0.0


# --- 2. several layers in one pass -------------------------------------------------------------------------

@pytest.mark.parametrize("staged", [1, 0])
def test_layers_in_one_pass(ca, pairs, staged):
    """3 layers x 20 spp of nanobox in one pass: the layer boundaries at samples 20 and 40 fall inside stages."""
    import torch
    x, y, spp = 20, 12, 20
    pair = pairs("nanobox")
    dev, cam = pair.dev, pair.camera(ca, x, y)
    want = ref(ca, pairs, "nanobox", x, y, spp, 3)
    dev.set_option("counters", 0)
    dev.set_option("sum_staged", staged)
    try:
        p = ca.render_params(x, y, spp, K, SEED, layer=1)
        assert dev.layers_per_pass(p, 3) == 3
        fr, mo = Guarded(y, x), Guarded(y, x)
        dev.render_layers_noise_device(cam, p, 3, fr.ptr, mo.ptr, 0)
        torch.cuda.synchronize()
        singles = render_single_layers(ca, dev, cam, x, y, spp, 3)
    finally:
        dev.set_option("counters", 1)
        dev.set_option("sum_staged", 1)
    fr.assert_guards("frame")
    mo.assert_guards("m2")
    assert_bitwise(fr.numpy(), want[2][0], "3 layers in one pass, frame vs oracle")
    assert_bitwise(mo.numpy(), want[2][1], "3 layers in one pass, m2 vs oracle")
    assert_bitwise(fr.numpy(), singles[2][0], "3 layers in one pass, frame vs single calls")
    assert_bitwise(mo.numpy(), singles[2][1], "3 layers in one pass, m2 vs single calls")


# --- 3. sample chunks --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,x,y,spp,per_chunk,chunks", [
    ("nanobox", 20, 12, 20, 8, 3),   # 8 + 8 + 4 through sum_samples_lds
    ("cornell", 24, 16, 5, 2, 3),    # 2 + 2 + 1 through the thread-per-pixel kernel
])
def test_sample_chunks_carry_the_moment_sum(ca, pairs, name, x, y, spp, per_chunk, chunks):
    """A sample buffer of per_chunk samples per work item (the pass's items are whole 32x32 tiles, so the
    budget is items x 12 B x per_chunk): the squares' running sum carries across the chunks in run2."""
    pair = pairs(name)
    dev = pair.dev
    want = ref(ca, pairs, name, x, y, spp, 3)
    p = ca.render_params(x, y, spp, K, SEED)
    items = dev.tiles_for_rank(p, 0) * 32 * 32
    dev.set_option("sample_buf_bytes", items * 12 * per_chunk)
    try:
        got = render_single_layers(ca, dev, pair.camera(ca, x, y), x, y, spp, 3)
        launches = dev.trace_stats()["camera"]["launches"]
    finally:
        dev.set_option("sample_buf_bytes", 4 << 30)
    assert launches == chunks, "the pass was not cut into %d sample chunks (%d camera traces)" % (chunks, launches)
    for layer, ((gf, gm), (of, om)) in enumerate(zip(got, want), 1):
        assert_bitwise(gf, of, "chunked %s frame, layer %d" % (name, layer))
        assert_bitwise(gm, om, "chunked %s m2, layer %d" % (name, layer))


# --- 4. partial tiles and frame pieces ---------------------------------------------------------------------

def test_partial_tiles_and_frame_pieces(ca, pairs):
    """70x45: 3 x 2 tiles whose right and bottom ones hang over the frame.  Single device calls, the frame as
    two tile-split pieces blended in place, and the host cr_render_layers_noise made to cut its pass group into
    pieces (wf_paths caps the chunk, as test_layer_groups_frame_pieces_bitexact does): all equal the oracle."""
    import torch
    x, y, spp = 70, 45, 2
    pair = pairs("sponza")
    dev, cam = pair.dev, pair.camera(ca, x, y)
    want = ref(ca, pairs, "sponza", x, y, spp, 2)
    got = render_single_layers(ca, dev, cam, x, y, spp, 2)
    for layer in (1, 2):
        assert_bitwise(got[layer - 1][0], want[layer - 1][0], "70x45 frame, layer %d" % layer)
        assert_bitwise(got[layer - 1][1], want[layer - 1][1], "70x45 m2, layer %d" % layer)
    # pieces through the device call: rank k of a 2-way split, both frames blended in place
    fr, mo = Guarded(y, x), Guarded(y, x)
    for layer in (1, 2):
        for piece in range(2):
            q = ca.render_params(x, y, spp, K, SEED, layer=layer, rank=piece, nranks=2)
            dev.render_layers_noise_device(cam, q, 1, fr.ptr, mo.ptr, 0)
    torch.cuda.synchronize()
    fr.assert_guards("frame")
    mo.assert_guards("m2")
    assert_bitwise(fr.numpy(), want[1][0], "70x45 in 2 pieces, frame")
    assert_bitwise(mo.numpy(), want[1][1], "70x45 in 2 pieces, m2")
    # the host call's pass group in pieces
    dev.set_option("counters", 0)
    dev.set_option("wf_paths", 13000)  # a layer of the frame is 6 tiles x 1024 x 2 = 12288 paths
    try:
        p = ca.render_params(x, y, spp, K, SEED, layer=1)
        assert dev.layers_per_pass(p, 2) == 1 and dev.layers_per_group(p, 2) == 2
        gf, gm = dev.render_layers_noise(cam, p, 2)
        assert dev.counters()["pixels"] == 2 * x * y
        st, err = dev.noise(x, y, 2, spp, 0.5, FLOOR)
    finally:
        dev.set_option("wf_paths", 256 << 20)
        dev.set_option("counters", 1)
    assert_bitwise(gf, want[1][0], "cr_render_layers_noise in pieces, frame")
    assert_bitwise(gm, want[1][1], "cr_render_layers_noise in pieces, m2")
    oerr, ost = noise_ref(want[1][0], want[1][1], 2, spp, 0.5, FLOOR)
    assert_bitwise(err, oerr, "cr_noise of the accumulators")
    assert st == ost


# --- 5. noise_eval alone -----------------------------------------------------------------------------------

EVAL_T, EVAL_FLOOR, EVAL_LAYERS, EVAL_SPP = 0.125, 0.5, 1, 4


def crafted(x, y, finite=False):
    """(frame, m2) [y][x][3]: random plausible pixels, and from pixel 0 on (as far as the frame reaches) the
    edge cases.  Pixel 0 has err == EVAL_T exactly: mean 0.5 per channel and floor 0.5 make the denominator 2,
    v_r = 0.25 and n = 4 make se_r = 0.25, the other channels 0 -> err = 0.125.
    finite: without the two cases whose err is infinite or huge, so that max_err is some ordinary pixel's."""
    rng = np.random.default_rng(x * 1000 + y)
    n = x * y
    f = rng.random((n, 3), dtype=F32) * F32(2.0)
    m = (f * f) * (F32(1.0) + rng.random((n, 3), dtype=F32) * F32(0.6))
    nan, inf, sub = F32(np.nan), F32(np.inf), F32(1e-40)
    special = [
        ((0.5, 0.5, 0.5), (0.5, 0.25, 0.25)),          # err == threshold exactly: must not count
        ((0, 0, 0), (0, 0, 0)),                          # zeros
        ((1.0, 2.0, 3.0), (0.5, 1.0, 2.0)),              # m2 < mean^2 in every channel
        ((1.0, 1.0, 1.0), (nan, 2.0, 2.0)),              # a NaN moment: that channel's variance is 0
        ((nan, 1.0, 1.0), (2.0, 2.0, 2.0)),              # a NaN mean: the error is NaN -> 0
        ((1.0, 1.0, 1.0), (inf, 2.0, 2.0)),              # an infinite moment: err = inf
        ((inf, 1.0, 1.0), (inf, 2.0, 2.0)),              # inf - inf
        ((1e30, 1.0, 1.0), (3e38, 2.0, 2.0)),            # mean^2 overflows
        ((1e-3, 1e-3, 1e-3), (3e38, 3e38, 3e38)),        # a huge variance
        ((sub, sub, sub), (sub, sub, sub)),              # subnormal mean and moment
        ((0, 0, 0), (sub, 0, 0)),                        # a subnormal variance over n
        ((0.5, 0.5, 0.5), (np.nextafter(F32(0.5), F32(1)), 0.25, 0.25)),  # one ulp above the threshold pixel
    ]
    for i, (a, b) in enumerate(special[:n]):
        if not (finite and i in (5, 8)):
            f[i], m[i] = np.array(a, F32), np.array(b, F32)
    return f.reshape(y, x, 3), m.reshape(y, x, 3)


@pytest.mark.parametrize("finite", [False, True])
# (700 x 400 = 280000 pixels: more than the kernel's 1024 blocks of 256 hold, so the blocks stride over the frame)
@pytest.mark.parametrize("x,y", [(1, 1), (63, 1), (65, 3), (70, 45), (700, 400)])
def test_noise_eval_matches_numpy(ca, pairs, x, y, finite):
    import torch
    dev = pairs("cornell").dev
    f, m = crafted(x, y, finite)
    oerr, ost = noise_ref(f, m, EVAL_LAYERS, EVAL_SPP, EVAL_T, EVAL_FLOOR)
    assert oerr[0, 0] == F32(EVAL_T)  # the crafted pixel sits exactly on the threshold
    if x * y > 11:
        assert oerr.reshape(-1)[11] > F32(EVAL_T) and np.isinf(oerr.reshape(-1)[5]) == (not finite)
        assert 0 < ost["above"] < x * y and np.isinf(ost["max_err"]) == (not finite)
    df, dm = torch.from_numpy(f).cuda(), torch.from_numpy(m).cuda()
    results = []
    for with_err in (True, False):
        derr = torch.full((y, x), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        dst = torch.full((6,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")  # (the call zeroes it)
        dev.noise_device(x, y, EVAL_LAYERS, EVAL_SPP, EVAL_T, EVAL_FLOOR, df.data_ptr(), dm.data_ptr(),
                         derr.data_ptr() if with_err else 0, dst.data_ptr(), 0)
        torch.cuda.synchronize()
        st = ca.CrNoiseStats.from_buffer_copy(dst.cpu().numpy().tobytes()).as_dict()
        results.append(st)
        assert st["pixels"] == ost["pixels"] and st["above"] == ost["above"] and st["layers"] == EVAL_LAYERS
        assert F32(st["max_err"]).view(np.uint32) == F32(ost["max_err"]).view(np.uint32), (st, ost)
        if with_err:
            assert_bitwise(derr.cpu().numpy(), oerr, "error map %dx%d" % (x, y))
        else:
            assert (derr.view(torch.int32) == POISON).all()
    assert results[0] == results[1]
    assert_bitwise(df.cpu().numpy(), f, "frame untouched")
    assert_bitwise(dm.cpu().numpy(), m, "m2 untouched")


# --- 6. render_until ---------------------------------------------------------------------------------------

UX, UY, USPP, UMAX = 32, 32, 4, 6


def until_sequence(ca, pairs, name, x, y, spp, threshold, floor):
    """The oracle's statistic after each of layers 1..UMAX."""
    return [noise_ref(f, m, layer, spp, threshold, floor)[1]
            for layer, (f, m) in enumerate(ref(ca, pairs, name, x, y, spp, UMAX), 1)]


def first_stop(seq, max_above, check_every=1, min_layers=1):
    for st in seq:
        if (st["layers"] % check_every == 0 or st["layers"] == len(seq)) and st["layers"] >= min_layers and \
                st["above"] <= max_above:
            return st["layers"]
    return len(seq)


def assert_stats(got, want, what):
    assert {k: got[k] for k in ("pixels", "above", "layers")} == {k: want[k] for k in ("pixels", "above", "layers")}, \
        (what, got, want)
    assert F32(got["max_err"]).view(np.uint32) == F32(want["max_err"]).view(np.uint32), (what, got, want)


def test_render_until_stop_layer(ca, pairs):
    pair = pairs("cornell")
    seq = until_sequence(ca, pairs, "cornell", UX, UY, USPP, UNTIL_T, UNTIL_FLOOR)
    print("oracle above per layer:", [s["above"] for s in seq], "max_err:", [s["max_err"] for s in seq])
    stop = first_stop(seq, UNTIL_ABOVE)
    assert 2 < stop < 5, "the constants must make the oracle stop strictly between layers 2 and 5"
    p = ca.render_params(UX, UY, USPP, K, SEED, layer=1)
    g, st = pair.dev.render_until(pair.camera(ca, UX, UY), p, 1, UMAX, 1, UNTIL_T, UNTIL_FLOOR, UNTIL_ABOVE)
    assert st["layers"] == stop
    assert_stats(st, seq[stop - 1], "stop layer")
    assert_bitwise(g, ref(ca, pairs, "cornell", UX, UY, USPP, UMAX)[stop - 1][0], "frame at the stop layer")
    # the ctx's accumulators are what was evaluated
    st2, err = pair.dev.noise(UX, UY, stop, USPP, UNTIL_T, UNTIL_FLOOR)
    f, m = ref(ca, pairs, "cornell", UX, UY, USPP, UMAX)[stop - 1]
    assert_bitwise(err, noise_ref(f, m, stop, USPP, UNTIL_T, UNTIL_FLOOR)[0], "error map at the stop layer")
    assert_stats(st2, seq[stop - 1], "cr_noise after cr_render_until")


def test_render_until_check_every_2(ca, pairs):
    """Pass groups of two layers (the lean build: the counting build renders one layer per pass): the stop
    layer is the first even layer that meets the target."""
    pair = pairs("cornell")
    seq = until_sequence(ca, pairs, "cornell", UX, UY, USPP, UNTIL_T, UNTIL_FLOOR)
    stop = first_stop(seq, UNTIL_ABOVE, check_every=2)
    assert stop % 2 == 0 and stop >= first_stop(seq, UNTIL_ABOVE)
    p = ca.render_params(UX, UY, USPP, K, SEED, layer=1)
    pair.dev.set_option("counters", 0)
    try:
        assert pair.dev.layers_per_group(p, 2) == 2
        g, st = pair.dev.render_until(pair.camera(ca, UX, UY), p, 1, UMAX, 2, UNTIL_T, UNTIL_FLOOR, UNTIL_ABOVE)
    finally:
        pair.dev.set_option("counters", 1)
    assert st["layers"] == stop
    assert_stats(st, seq[stop - 1], "check_every 2")
    assert_bitwise(g, ref(ca, pairs, "cornell", UX, UY, USPP, UMAX)[stop - 1][0], "frame, check_every 2")


def test_render_until_no_convergence_and_min_layers(ca, pairs):
    pair = pairs("cornell")
    cam = pair.camera(ca, UX, UY)
    frames = ref(ca, pairs, "cornell", UX, UY, USPP, UMAX)
    p = ca.render_params(UX, UY, USPP, K, SEED, layer=1)
    # a threshold no frame of 24 samples meets: max_layers is reached with pixels still above
    tiny = until_sequence(ca, pairs, "cornell", UX, UY, USPP, 1e-6, UNTIL_FLOOR)
    assert all(s["above"] > 0 for s in tiny)
    g, st = pair.dev.render_until(cam, p, 1, UMAX, 1, 1e-6, UNTIL_FLOOR, 0)
    assert st["layers"] == UMAX and st["above"] > 0
    assert_stats(st, tiny[UMAX - 1], "no convergence")
    assert_bitwise(g, frames[UMAX - 1][0], "frame at max_layers")
    # a threshold every frame meets: min_layers alone decides
    huge = until_sequence(ca, pairs, "cornell", UX, UY, USPP, 1e9, UNTIL_FLOOR)
    assert all(s["above"] == 0 for s in huge)
    g, st = pair.dev.render_until(cam, p, 3, UMAX, 1, 1e9, UNTIL_FLOOR, 0)
    assert st["layers"] == 3
    assert_stats(st, huge[2], "min_layers")
    assert_bitwise(g, frames[2][0], "frame at min_layers")


# --- 7. isolation ------------------------------------------------------------------------------------------

def test_plain_renders_are_untouched(ca, pairs):
    import torch
    x, y, spp = 24, 16, 4
    pair = pairs("cornell")
    dev, cam = pair.dev, pair.camera(ca, x, y)
    want = ref(ca, pairs, "cornell", x, y, spp, 3)
    got = render_single_layers(ca, dev, cam, x, y, spp, 2)  # a noise render first (guard bands checked inside)
    assert_bitwise(got[1][1], want[1][1], "m2")
    # the plain host render of layers 1-2 afterwards
    g = None
    for layer in (1, 2):
        g = dev.render(cam, ca.render_params(x, y, spp, K, SEED, layer=layer), g)
    assert_bitwise(g, want[1][0], "plain render after a noise render")
    # the plain device call next to a poisoned moment buffer: the buffer of the last noise render stays as it is
    fr, mo = Guarded(y, x), Guarded(y, x)
    dev.render_layers_noise_device(cam, ca.render_params(x, y, spp, K, SEED, layer=1), 1, fr.ptr, mo.ptr, 0)
    torch.cuda.synchronize()
    mo.body.view(torch.int32).fill_(POISON)
    dev.render_layers_device(cam, ca.render_params(x, y, spp, K, SEED, layer=2), 1, fr.ptr, 0)
    torch.cuda.synchronize()
    assert (mo.t.view(torch.int32) == POISON).all(), "cr_render_layers_device wrote a moment buffer"
    fr.assert_guards("frame")
    assert_bitwise(fr.numpy(), want[1][0], "plain device layer 2 over a noise render's layer 1")


# --- 8. API mirrors ----------------------------------------------------------------------------------------

def test_raytracer_raytrace_until(ca, pairs, scenes):
    """RayTracer::rayTraceUntil through libchiaroscuro: test 6's layer, statistic and pixels (the RayTracer's
    ctx runs the counting build, one layer per pass group, so the noise is checked after every layer)."""
    seq = until_sequence(ca, pairs, "cornell", UX, UY, USPP, UNTIL_T, UNTIL_FLOOR)
    stop = first_stop(seq, UNTIL_ABOVE)
    frames = ref(ca, pairs, "cornell", UX, UY, USPP, UMAX)
    scene = ca.Scene(scenes.config_rtc("cornell"), "xres", str(UX), "yres", str(UY), "samples", str(USPP))
    i = scene.info
    assert (i["k"], i["seed"]) == (K, SEED)
    rt = ca.RayTracer(ca.Model(scene), scene)
    view = (i["VP"], i["LA"], i["UP"], i["yview"])
    reached = rt.rayTraceUntil(UNTIL_T, UMAX, *view, floor=UNTIL_FLOOR, checkEvery=1, maxAbove=UNTIL_ABOVE)
    assert reached == stop == rt.layers
    assert_stats(rt.lastNoise(), seq[stop - 1], "RayTracer.lastNoise")
    assert_bitwise(rt.pixels, frames[stop - 1][0], "RayTracer.rayTraceUntil pixels")
    f, m = frames[stop - 1]
    assert_bitwise(rt.noiseMap(), noise_ref(f, m, stop, USPP, UNTIL_T, UNTIL_FLOOR)[0], "RayTracer.noiseMap")
    # the same view again: the frame already meets the target at the next check, one more layer
    assert rt.rayTraceUntil(1e9, UMAX, *view, floor=UNTIL_FLOOR, checkEvery=1) == stop + 1
    assert_bitwise(rt.pixels, frames[stop][0], "continued accumulation")


def read_pfm(path):
    """PFM (little-endian, rows bottom-to-top) -> [H][W][3] float32, row 0 = top."""
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    assert parts[0] == b"PF"
    w, h = (int(v) for v in parts[1].split())
    assert float(parts[2]) < 0
    return np.frombuffer(parts[3], dtype="<f4", count=w * h * 3).reshape(h, w, 3)[::-1]


def test_cli_noise_token(ca, pairs, scenes, tmp_path):
    """bin/chiaroscuro ... layers 6 noise T: the PFM is the oracle's frame at the layer where the oracle's own
    max_err first falls to T (the CLI's max_above is 0, its floor 1e-3), checked after every layer."""
    seq = until_sequence(ca, pairs, "cornell", CLI_X, CLI_Y, CLI_SPP, CLI_T, FLOOR)
    print("oracle max_err per layer:", [s["max_err"] for s in seq])
    stop = first_stop(seq, 0)
    assert 1 < stop < UMAX, "CLI_T must make the oracle stop inside 2..5"
    out = tmp_path / "until.pfm"
    exe = scenes.default_dir().parent.parent / "bin" / "chiaroscuro"
    r = subprocess.run([str(exe), str(scenes.config_rtc("cornell")), "xres", str(CLI_X), "yres", str(CLI_Y),
                        "samples", str(CLI_SPP), "output", str(out), "layers", str(UMAX), "noise", repr(CLI_T)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "layer %d of at most %d" % (stop, UMAX) in r.stderr, r.stderr
    assert_bitwise(read_pfm(out), ref(ca, pairs, "cornell", CLI_X, CLI_Y, CLI_SPP, UMAX)[stop - 1][0],
                   "cli noise, PFM")
