"""Adaptive sampling on the GPU (include/chiaro_hip.h "adaptive sampling"), bit for bit:

1. cr_noise_select_device against a numpy restatement: the stable compaction, the statistic, the guard bands;
2. cr_render_layers_list_device against the oracle: listed pixels hold the later layer, the others are untouched;
3. cr_render_adaptive against the adaptive steps run on the oracle's own sequence of frames;
4. isolation (plain renders around an adaptive one) and the RayTracer / CLI mirrors.

The oracle's frames and moment frames are test_gpu_noise's references (computed once per shape and shared with it).

Fixtures, from the oracle at seed 0xC41A05C0, k 6, max_layers 6 (recomputed and asserted below):
cornell 32x32 x 4 spp, threshold 0.25, floor 0.25
  min_layers  check_every  checks at  active after each check  pixels per final layer count 1..6  pixel-layers / 6144
  1           1            1..5(,6)   108, 58, 36, 25, 17      916, 50, 22, 11, 8, 17             1268
  2           1            2..5(,6)   99, 57, 39, 28           0, 925, 42, 18, 11, 28             2271
  1 or 2      2            2, 4(,6)   99, 40                   0, 925, 0, 59, 0, 40               2326
cornell 12x12 x 64 spp, threshold 0.3, floor 1e-3, min_layers 1, check_every 1 (the CLI and RayTracer case):
  active 57, 35, 23, 14, 13; pixels per final layer count 87, 22, 12, 9, 1, 13; 286 pixel-layers of 864.
(The check at max_layers serves the statistic only; the table's counts stop before it.)
"""
import subprocess

import numpy as np
import pytest

from helpers import assert_bitwise
from test_gpu_noise import (CLI_SPP, CLI_X, CLI_Y, EVAL_FLOOR, EVAL_LAYERS, EVAL_SPP, EVAL_T, FLOOR, K, POISON, SEED,
                            UMAX, UNTIL_FLOOR, UNTIL_T, USPP, UX, UY, Guarded, crafted, noise_ref, pairs, read_pfm,
                            ref)

pytestmark = pytest.mark.gpu

F32 = np.float32
SKIP = 0xFFFFFFFF
AD_CLI_T = 0.3


# --- 1. selection ------------------------------------------------------------------------------------------

def select_ref(frame, m2, layers, spp, threshold, floor, lst):
    """(output list, statistic) of a selection, restated in numpy on noise_ref's error map."""
    err = noise_ref(frame, m2, layers, spp, threshold, floor)[0].reshape(-1)
    lst = np.asarray(lst, np.uint32)
    ev = lst[lst != SKIP]
    e = err[ev]
    pos = e[e > 0]
    return ev[e > F32(threshold)], {"evaluated": int(ev.size), "above": int((e > F32(threshold)).sum()),
                                    "max_err": float(pos.max()) if pos.size else 0.0, "layers": int(layers)}


def select_lists(err, n):
    """The input lists of one frame: name -> uint32 array."""
    hot = np.flatnonzero(err > F32(EVAL_T)).astype(np.uint32)
    cold = np.flatnonzero(~(err > F32(EVAL_T))).astype(np.uint32)
    mixed = np.arange(n, dtype=np.uint32)[::-1].copy()  # descending: the output keeps the INPUT order, not the pixels'
    mixed[1::3] = SKIP
    return {
        "whole": np.arange(n, dtype=np.uint32),
        "every_other": np.arange(0, n, 2, dtype=np.uint32),
        "one": np.array([min(11, n - 1)], np.uint32),
        "threshold_pixel": np.array([0], np.uint32),
        "empty": np.zeros(0, np.uint32),
        "all_selected": hot,
        "none_selected": cold,
        "skipped": np.concatenate([np.full(3, SKIP, np.uint32), mixed, np.full(70, SKIP, np.uint32)]),
    }


# (513 x 512 = 262,656 pixels: past one grid of 1024 blocks x 256 entries, so blocks walk more than one chunk)
@pytest.mark.parametrize("x,y", [(1, 1), (9, 7), (8, 8), (65, 1), (16, 16), (257, 1), (70, 45), (513, 512)])
def test_select_matches_numpy(ca, pairs, x, y):
    import torch
    dev = pairs("cornell").dev
    f, m = crafted(x, y)
    err = noise_ref(f, m, EVAL_LAYERS, EVAL_SPP, EVAL_T, EVAL_FLOOR)[0].reshape(-1)
    assert err[0] == F32(EVAL_T)  # the crafted pixel sits exactly on the threshold: it must not be selected
    df, dm = torch.from_numpy(f).cuda(), torch.from_numpy(m).cuda()
    guard = 1024
    for name, lst in select_lists(err, x * y).items():
        want, wst = select_ref(f, m, EVAL_LAYERS, EVAL_SPP, EVAL_T, EVAL_FLOOR, lst)
        if name == "all_selected":
            assert len(want) == len(lst)
        if name in ("none_selected", "threshold_pixel", "empty"):
            assert len(want) == 0
        if name == "whole" and x * y > 11:
            assert 0 < len(want) < x * y
        n = len(lst)
        din = torch.from_numpy(lst.view(np.int32).copy()).cuda() if n else None
        dout = torch.full((n + 2 * guard,), POISON, dtype=torch.int32, device="cuda")
        dst = torch.full((6,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")  # (the call writes it whole)
        dev.noise_select(x, y, EVAL_LAYERS, EVAL_SPP, EVAL_T, EVAL_FLOOR, df.data_ptr(), dm.data_ptr(),
                         din.data_ptr() if n else 0, n, dout[guard:].data_ptr() if n else 0, dst.data_ptr(), 0)
        torch.cuda.synchronize()
        st = ca.CrSelectStats.from_buffer_copy(dst.cpu().numpy().tobytes()).as_dict()
        what = "%dx%d %s" % (x, y, name)
        assert {k: st[k] for k in ("evaluated", "above", "layers")} == \
               {k: wst[k] for k in ("evaluated", "above", "layers")}, (what, st, wst)
        assert F32(st["max_err"]).view(np.uint32) == F32(wst["max_err"]).view(np.uint32), (what, st, wst)
        out = dout.cpu().numpy()
        got = out[guard:guard + st["above"]].view(np.uint32)
        assert np.array_equal(got, want), (what, got[:8], want[:8])
        # nothing before the output, nothing from entry `above` to its end, nothing after
        assert (out[:guard] == POISON).all() and (out[guard + st["above"]:] == POISON).all(), what + ": guard band"
        if n:
            assert np.array_equal(din.cpu().numpy().view(np.uint32), lst), what + ": input list"
    assert_bitwise(df.cpu().numpy(), f, "frame untouched")
    assert_bitwise(dm.cpu().numpy(), m, "m2 untouched")


# --- 2. list render ----------------------------------------------------------------------------------------

def oracle_counters(ca, pair, x, y, spp, pix, layers):
    """The oracle's counters of rendering the listed pixels at each of `layers`, summed."""
    pix = np.asarray(pix, np.uint32)
    total = {}
    for layer in layers:
        _, c = pair.oracle.render_pixels(pair.camera(ca, x, y).as_array(), x, y, spp, K, SEED, pix % x, pix // x,
                                         layer=layer)
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    return total


def list_render(ca, pair, x, y, spp, lst, calls=((2, 2),), tile=0):
    """A full layer 1, then for each (first layer, nlayers) of `calls` a list render of lst; -> (frame, m2, dev
    counters after the last call, camera launches of the last call)."""
    import torch
    dev, cam = pair.dev, pair.camera(ca, x, y)
    fr, mo = Guarded(y, x), Guarded(y, x)
    dev.render_layers_noise_device(cam, ca.render_params(x, y, spp, K, SEED, layer=1, tile=tile), 1, fr.ptr, mo.ptr, 0)
    lst = np.asarray(lst, np.uint32)
    dl = torch.from_numpy(lst.view(np.int32).copy()).cuda()
    for first, nl in calls:
        p = ca.render_params(x, y, spp, K, SEED, layer=first, tile=tile)
        dev.render_layers_list(cam, p, nl, dl.data_ptr(), len(lst), fr.ptr, mo.ptr, 0)
    torch.cuda.synchronize()
    fr.assert_guards("frame")
    mo.assert_guards("m2")
    assert np.array_equal(dl.cpu().numpy().view(np.uint32), lst), "the list is an input"
    return fr.numpy(), mo.numpy(), dev.counters(), dev.trace_stats()["camera"]["launches"]


def assert_listed(got_f, got_m, want, lst, x, y, what, after=3, before=1):
    """Listed pixels equal the oracle after `after` layers, the others after `before`, frame and m2, bitwise."""
    listed = np.zeros(x * y, bool)
    lst = np.asarray(lst, np.uint32)
    listed[lst[lst != SKIP]] = True
    listed = listed.reshape(y, x)
    for got, k, label in ((got_f, 0, "frame"), (got_m, 1, "m2")):
        assert_bitwise(got[listed], want[after - 1][k][listed], "%s: listed pixels' %s" % (what, label))
        assert_bitwise(got[~listed], want[before - 1][k][~listed], "%s: other pixels' %s" % (what, label))
    assert listed.any() and not np.array_equal(want[after - 1][0][listed], want[before - 1][0][listed])


def hand_list(x, y):
    """The first pixel, the last pixel and a few scattered ones -- seven entries, not in pixel order."""
    n = x * y
    return np.array([n - 1, 0, n // 2 + 3, x + 1, n // 3, n - x, 5 % n], np.uint32)


@pytest.mark.parametrize("spp", [4, 5])          # sum_samples_lds (s_count % 4 == 0) and the thread-per-pixel kernel
@pytest.mark.parametrize("tail", [0, 1 << 20])   # the per-generation kernels; the whole pass in wf_tail
def test_list_render_cornell(ca, pairs, spp, tail):
    """Cornell 12x12 on the counting build (one layer per pass, so layers 2-3 are two passes whose counters sum):
    the image, the moments, and every counter against the oracle's render_pixels of the same pixels and layers."""
    x, y = 12, 12
    pair = pairs("cornell")
    want = ref(ca, pairs, "cornell", x, y, spp, 3)
    lst = hand_list(x, y)
    assert len(set(lst.tolist())) == len(lst) and len(lst) % 64
    pair.dev.set_option("wf_tail_min", tail)
    try:
        f, m, gc, _ = list_render(ca, pair, x, y, spp, lst)
    finally:
        pair.dev.set_option("wf_tail_min", 0)
    assert_listed(f, m, want, lst, x, y, "cornell 12x12x%d tail %d" % (spp, tail))
    oc = oracle_counters(ca, pair, x, y, spp, lst, (2, 3))
    assert oc["paths"] == 2 * len(lst) * spp and gc["pixels"] == 2 * len(lst)
    assert all(gc[k] == oc[k] for k in oc), (gc, oc)


def test_list_render_partial_tiles(ca, pairs):
    """70x45 with tile 32 (3 x 2 tiles, the right and bottom ones partial): pixels of the partial tiles, a list of
    one pixel, and a caller-padded list with skipped entries between and after the pixels."""
    x, y, spp = 70, 45, 2
    pair = pairs("sponza")
    want = ref(ca, pairs, "sponza", x, y, spp, 3)
    edge = np.array([y * x - 1, 0, 69, 44 * x, 44 * x + 64, 33 * x + 65, 31 * x + 31, 32 * x + 32, 10 * x + 68], np.uint32)
    for what, lst in (("partial tiles", edge), ("one pixel", edge[:1]),
                      ("padded", np.concatenate([[SKIP], edge[:4], [SKIP, SKIP], edge[4:], np.full(55, SKIP)]).astype(np.uint32))):
        f, m, gc, _ = list_render(ca, pair, x, y, spp, lst, tile=32)
        assert_listed(f, m, want, lst, x, y, "70x45 " + what)
        npx = int((lst != SKIP).sum())
        assert gc["paths"] == 2 * npx * spp and gc["pixels"] == 2 * npx, (what, gc)


def test_list_render_layers_per_pass(ca, pairs):
    """The lean build: layers 2-3 of the list in one pass (one camera trace) and as one pass each -- the same bits."""
    x, y, spp = 24, 16, 4
    pair = pairs("cornell")
    want = ref(ca, pairs, "cornell", x, y, spp, 3)
    lst = np.arange(0, x * y, 3, dtype=np.uint32)[::-1].copy()
    pair.dev.set_option("counters", 0)
    try:
        f2, m2, _, launches2 = list_render(ca, pair, x, y, spp, lst, calls=((2, 2),))
        f1, m1, _, launches1 = list_render(ca, pair, x, y, spp, lst, calls=((2, 1), (3, 1)))
    finally:
        pair.dev.set_option("counters", 1)
    assert launches2 == 1 and launches1 == 1  # (launches1: of the last call alone)
    assert_listed(f2, m2, want, lst, x, y, "two layers in one pass")
    assert_listed(f1, m1, want, lst, x, y, "one layer per pass")


@pytest.mark.parametrize("spp", [4, 5])
def test_list_render_without_moments(ca, pairs, spp):
    """No moment frame: the frame alone, through the list forms of the plain sum kernels."""
    import torch
    x, y = 24, 16
    pair = pairs("cornell")
    dev, cam = pair.dev, pair.camera(ca, x, y)
    want = ref(ca, pairs, "cornell", x, y, spp, 3)
    lst = hand_list(x, y)
    fr = Guarded(y, x)
    dev.render_layers_device(cam, ca.render_params(x, y, spp, K, SEED, layer=1), 1, fr.ptr, 0)
    dl = torch.from_numpy(lst.view(np.int32).copy()).cuda()
    dev.render_layers_list(cam, ca.render_params(x, y, spp, K, SEED, layer=2), 2, dl.data_ptr(), len(lst), fr.ptr, 0, 0)
    torch.cuda.synchronize()
    fr.assert_guards("frame")
    listed = np.zeros(x * y, bool)
    listed[lst] = True
    listed = listed.reshape(y, x)
    assert_bitwise(fr.numpy()[listed], want[2][0][listed], "listed pixels, no m2")
    assert_bitwise(fr.numpy()[~listed], want[0][0][~listed], "other pixels, no m2")


def test_list_render_sample_chunks(ca, pairs):
    """A sample buffer of 8 samples per work item: each layer of the list (one tile of entries) runs as sample chunks
    8 + 8 + 4 whose running sums carry across the launches."""
    x, y, spp = 20, 12, 20
    pair = pairs("nanobox")
    want = ref(ca, pairs, "nanobox", x, y, spp, 3)
    lst = np.arange(1, x * y, 2, dtype=np.uint32)
    pair.dev.set_option("sample_buf_bytes", 1024 * 12 * 8)
    try:
        f, m, gc, launches = list_render(ca, pair, x, y, spp, lst)
    finally:
        pair.dev.set_option("sample_buf_bytes", 4 << 30)
    assert launches == 2 * 3, "two layers x three sample chunks, %d camera traces" % launches
    assert_listed(f, m, want, lst, x, y, "sample chunks")
    assert gc["paths"] == 2 * len(lst) * spp


def test_list_render_split_over_passes(ca, pairs):
    """wf_paths 5000 against a list of the whole 70x45 frame (3150 entries, 4096 work items, 2 spp): a pass holds two
    tiles of entries and one layer, so layers 2-3 are 2 ranges x 2 layers = 4 passes."""
    x, y, spp = 70, 45, 2
    pair = pairs("sponza")
    want = ref(ca, pairs, "sponza", x, y, spp, 3)
    lst = np.arange(x * y, dtype=np.uint32)
    lst = np.concatenate([lst[1::2], lst[0::2]])  # every pixel, not in pixel order
    pair.dev.set_option("counters", 0)
    pair.dev.set_option("wf_paths", 5000)
    try:
        f, m, _, launches = list_render(ca, pair, x, y, spp, lst, tile=32)
    finally:
        pair.dev.set_option("wf_paths", 256 << 20)
        pair.dev.set_option("counters", 1)
    assert launches == 4, launches
    assert_bitwise(f, want[2][0], "whole frame listed, frame")
    assert_bitwise(m, want[2][1], "whole frame listed, m2")


def test_list_render_large_scene_sorted_queues(ca, pairs):
    """The sponza stand-in (>= 65,536 triangles: trace build 59, leaf keys, sorted queues from wf_sort_min on)."""
    x, y, spp = 24, 16, 8
    pair = pairs("sponza")
    assert pair.dev.scene_triangles() >= 65536
    want = ref(ca, pairs, "sponza", x, y, spp, 3)
    lst = np.arange(2, x * y, 3, dtype=np.uint32)
    pair.dev.set_option("counters", 0)
    pair.dev.set_option("wf_sort_min", 16)
    try:
        f, m, _, _ = list_render(ca, pair, x, y, spp, lst)
        build = pair.dev.last_trace_build()
    finally:
        pair.dev.set_option("wf_sort_min", 1 << 16)
        pair.dev.set_option("counters", 1)
    assert build == 59
    assert_listed(f, m, want, lst, x, y, "sponza stand-in, build 59")


# --- 3. the adaptive render --------------------------------------------------------------------------------

def adaptive_ref(frames, spp, min_layers, max_layers, check_every, threshold, floor):
    """cr_render_adaptive's steps on the oracle's sequence frames[L - 1] = (frame, m2) after L layers."""
    y, x, _ = frames[0][0].shape
    active = np.ones((y, x), bool)
    lmap = np.zeros((y, x), np.uint32)
    st = {"pixels": x * y, "pixel_layers": 0, "active": 0, "layers": 0, "checks": 0, "max_err": 0.0}
    actives = []
    L = 0
    while L < max_layers and active.any():
        L += min(check_every, max_layers - L)
        lmap[active] = L
        st["layers"] = L
        if L < min_layers:
            continue
        err = noise_ref(frames[L - 1][0], frames[L - 1][1], L, spp, threshold, floor)[0]
        above = active & (err > F32(threshold))
        pos = err[active & (err > 0)]
        st["checks"] += 1
        st["active"] = int(above.sum())
        st["max_err"] = float(pos.max()) if pos.size else 0.0
        if L == max_layers:
            break
        actives.append(st["active"])
        active = above
    st["pixel_layers"] = int(lmap.sum(dtype=np.uint64))
    frame = np.zeros((y, x, 3), F32)
    m2 = np.zeros((y, x, 3), F32)
    for L in np.unique(lmap):
        sel = lmap == L
        frame[sel], m2[sel] = frames[L - 1][0][sel], frames[L - 1][1][sel]
    return frame, m2, lmap, st, actives


def assert_adaptive(got, want, what):
    gf, gm, gmap, gst = got
    wf, wm, wmap, wst, _ = want
    assert np.array_equal(gmap, wmap), (what, np.argwhere(gmap != wmap)[:5].tolist())
    assert_bitwise(gf, wf, what + ": frame")
    assert_bitwise(gm, wm, what + ": m2")
    assert {k: gst[k] for k in gst if k != "max_err"} == {k: wst[k] for k in wst if k != "max_err"}, (what, gst, wst)
    assert F32(gst["max_err"]).view(np.uint32) == F32(wst["max_err"]).view(np.uint32), (what, gst, wst)


# (min_layers, check_every) -> active after each check before max_layers, pixels per final layer count, pixel-layers
AD_TABLE = {
    (1, 1): ([108, 58, 36, 25, 17], [916, 50, 22, 11, 8, 17], 1268),
    (2, 1): ([99, 57, 39, 28], [0, 925, 42, 18, 11, 28], 2271),
    (1, 2): ([99, 40], [0, 925, 0, 59, 0, 40], 2326),
    (2, 2): ([99, 40], [0, 925, 0, 59, 0, 40], 2326),
}


@pytest.mark.parametrize("min_layers,check_every", sorted(AD_TABLE))
@pytest.mark.parametrize("counting", [1, 0])
def test_render_adaptive(ca, pairs, min_layers, check_every, counting):
    pair = pairs("cornell")
    frames = ref(ca, pairs, "cornell", UX, UY, USPP, UMAX)
    want = adaptive_ref(frames, USPP, min_layers, UMAX, check_every, UNTIL_T, UNTIL_FLOOR)
    wmap, wst, actives = want[2], want[3], want[4]
    per_count = [int((wmap == L).sum()) for L in range(1, UMAX + 1)]
    print("oracle: active", actives, "pixels per layer count", per_count, "pixel-layers", wst["pixel_layers"])
    # before the GPU is touched: the map is a real mixture, and it is the fixture's
    values = set(np.unique(wmap).tolist())
    assert len(values) >= 3 and UMAX in values and min(values) < UMAX
    assert (actives, per_count, wst["pixel_layers"]) == AD_TABLE[(min_layers, check_every)]
    p = ca.render_params(UX, UY, USPP, K, SEED, layer=1)
    pair.dev.set_option("counters", counting)
    try:
        got = pair.dev.render_adaptive(pair.camera(ca, UX, UY), p, min_layers, UMAX, check_every, UNTIL_T, UNTIL_FLOOR)
        gc = pair.dev.counters()
    finally:
        pair.dev.set_option("counters", 1)
    assert_adaptive(got, want, "adaptive min %d every %d counting %d" % (min_layers, check_every, counting))
    assert gc["pixels"] == wst["pixel_layers"]
    if counting:
        assert gc["paths"] == wst["pixel_layers"] * USPP


def test_render_adaptive_extreme_thresholds(ca, pairs):
    pair = pairs("cornell")
    dev, cam = pair.dev, pair.camera(ca, UX, UY)
    frames = ref(ca, pairs, "cornell", UX, UY, USPP, UMAX)
    p = ca.render_params(UX, UY, USPP, K, SEED, layer=1)
    # a threshold nothing meets: every pixel takes max_layers, and the frame is cr_render_layers'.  On the 12x12 x 64 spp
    # fixture, where every pixel has a positive variance from the first layer on (a pixel whose four samples of the
    # 32x32 x 4 spp fixture agree has err 0, which no threshold >= 0 is below)
    cam12, p12 = pair.camera(ca, CLI_X, CLI_Y), ca.render_params(CLI_X, CLI_Y, CLI_SPP, K, SEED, layer=1)
    want = adaptive_ref(ref(ca, pairs, "cornell", CLI_X, CLI_Y, CLI_SPP, UMAX), CLI_SPP, 1, UMAX, 1, 1e-6, FLOOR)
    assert (want[2] == UMAX).all() and want[3]["checks"] == UMAX and want[4] == [CLI_X * CLI_Y] * (UMAX - 1)
    got = dev.render_adaptive(cam12, p12, 1, UMAX, 1, 1e-6, FLOOR)
    assert_adaptive(got, want, "nothing converges")
    assert_bitwise(got[0], dev.render_layers(cam12, p12, UMAX), "adaptive with no drop vs cr_render_layers")
    # a threshold everything meets: every pixel stops at the first check -- the first multiple of check_every that
    # is >= min_layers
    for min_layers, check_every, first in ((1, 1, 1), (3, 1, 3), (3, 2, 4), (1, 4, 4), (6, 4, 6), (1, 7, 6)):
        want = adaptive_ref(frames, USPP, min_layers, UMAX, check_every, 1e9, UNTIL_FLOOR)
        assert (want[2] == first).all() and want[3]["checks"] == 1
        got = dev.render_adaptive(cam, p, min_layers, UMAX, check_every, 1e9, UNTIL_FLOOR)
        assert_adaptive(got, want, "everything converges, min %d every %d" % (min_layers, check_every))
    # without the optional outputs
    f, m, lmap, st = dev.render_adaptive(cam, p, 1, UMAX, 1, UNTIL_T, UNTIL_FLOOR, want_m2=False)
    assert m is None
    assert_bitwise(f, adaptive_ref(frames, USPP, 1, UMAX, 1, UNTIL_T, UNTIL_FLOOR)[0], "no m2 out")


def test_render_adaptive_groups_that_do_not_fit_a_pass(ca, pairs):
    """wf_paths holds one layer of the frame, check_every is 2: the two layers before the first check run as two
    passes with no check between them, and with tile 8 the lists are padded to whole 8x8 tiles -- the layer map, and
    every pixel, are what the schedule alone gives."""
    pair = pairs("cornell")
    frames = ref(ca, pairs, "cornell", UX, UY, USPP, UMAX)
    want = adaptive_ref(frames, USPP, 1, UMAX, 2, UNTIL_T, UNTIL_FLOOR)
    p = ca.render_params(UX, UY, USPP, K, SEED, layer=1, tile=8)
    pair.dev.set_option("counters", 0)
    pair.dev.set_option("wf_paths", 4096)  # (the frame is 1024 x 4 = 4096 paths per layer: one layer per pass)
    try:
        got = pair.dev.render_adaptive(pair.camera(ca, UX, UY), p, 1, UMAX, 2, UNTIL_T, UNTIL_FLOOR)
    finally:
        pair.dev.set_option("wf_paths", 256 << 20)
        pair.dev.set_option("counters", 1)
    assert_adaptive(got, want, "tile 8, one layer per pass")


# --- 4. isolation and the mirrors --------------------------------------------------------------------------

def test_plain_renders_around_an_adaptive_one(ca, pairs):
    pair = pairs("cornell")
    dev, cam = pair.dev, pair.camera(ca, UX, UY)
    frames = ref(ca, pairs, "cornell", UX, UY, USPP, UMAX)
    p = ca.render_params(UX, UY, USPP, K, SEED, layer=1)
    before = dev.render_layers(cam, p, 3)
    until_before = dev.render_until(cam, p, 1, UMAX, 1, UNTIL_T, UNTIL_FLOOR, 80)
    dev.render_adaptive(cam, p, 1, UMAX, 1, UNTIL_T, UNTIL_FLOOR)
    after = dev.render_layers(cam, p, 3)
    until_after = dev.render_until(cam, p, 1, UMAX, 1, UNTIL_T, UNTIL_FLOOR, 80)
    assert_bitwise(before, frames[2][0], "cr_render_layers before")
    assert_bitwise(after, before, "cr_render_layers after an adaptive render")
    assert until_before[1] == until_after[1]
    assert_bitwise(until_after[0], until_before[0], "cr_render_until after an adaptive render")
    assert_bitwise(until_after[0], frames[until_after[1]["layers"] - 1][0], "cr_render_until vs oracle")


def cli_reference(ca, pairs):
    frames = ref(ca, pairs, "cornell", CLI_X, CLI_Y, CLI_SPP, UMAX)
    want = adaptive_ref(frames, CLI_SPP, 1, UMAX, 1, AD_CLI_T, FLOOR)
    per_count = [int((want[2] == L).sum()) for L in range(1, UMAX + 1)]
    assert (want[4], per_count, want[3]["pixel_layers"]) == ([57, 35, 23, 14, 13], [87, 22, 12, 9, 1, 13], 286)
    return want


def test_raytracer_raytrace_adaptive(ca, pairs, scenes):
    want = cli_reference(ca, pairs)
    scene = ca.Scene(scenes.config_rtc("cornell"), "xres", str(CLI_X), "yres", str(CLI_Y), "samples", str(CLI_SPP))
    i = scene.info
    assert (i["k"], i["seed"]) == (K, SEED)
    rt = ca.RayTracer(ca.Model(scene), scene)
    view = (i["VP"], i["LA"], i["UP"], i["yview"])
    done = rt.rayTraceAdaptive(AD_CLI_T, UMAX, *view, floor=FLOOR, minLayers=1, checkEvery=1)
    assert done == want[3]["pixel_layers"] == 286
    assert np.array_equal(rt.layerMap(), want[2])
    st = rt.lastAdaptive()
    assert {k: st[k] for k in st if k != "max_err"} == {k: want[3][k] for k in st if k != "max_err"}
    assert_bitwise(rt.pixels, want[0], "RayTracer.rayTraceAdaptive pixels")
    assert rt.counters()["paths"] == 286 * CLI_SPP
    # the frame is no progressive state: the next rayTrace is layer 1 again
    rt.rayTrace(*view)
    assert rt.layers == 1
    assert_bitwise(rt.pixels, ref(ca, pairs, "cornell", CLI_X, CLI_Y, CLI_SPP, UMAX)[0][0], "rayTrace after adaptive")


def test_cli_adaptive_token(ca, pairs, scenes, tmp_path):
    want = cli_reference(ca, pairs)
    out = tmp_path / "adaptive.pfm"
    exe = scenes.default_dir().parent.parent / "bin" / "chiaroscuro"
    r = subprocess.run([str(exe), str(scenes.config_rtc("cornell")), "xres", str(CLI_X), "yres", str(CLI_Y),
                        "samples", str(CLI_SPP), "output", str(out), "layers", str(UMAX), "adaptive", repr(AD_CLI_T)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "286 of 864 pixel-layers" in r.stderr, r.stderr
    assert_bitwise(read_pfm(out), want[0], "cli adaptive, PFM")
