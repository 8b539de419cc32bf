"""Temporal reprojection on the GPU (include/chiaro_hip.h "temporal reprojection") against its numpy
restatement (tests/temporal_model.py), bit for bit:

1. cr_reproject_device on crafted inputs (tests/temporal_cases.py): frames from one pixel to several blocks, six
   camera pairs, the edge cases from pixel 0 on, with and without a layer map, other parameters, a non-default
   stream, guard bands; the packed history layout writes the same bits as the planar one;
2. cr_render_temporal over three cameras equals the model chained on the oracle's frames, moments and guides; the
   stored history after each step; the ctx's progressive accumulators stay untouched;
3. the same with the denoiser set; cr_temporal_reset;
4. RayTracer.rayTraceTemporal and the preview session.

NaNs are compared as NaNs (denoise_model.canon); everything else bit for bit."""
import math

import numpy as np
import pytest

import denoise_model as dm
import temporal_cases as tc
from helpers import assert_bitwise
from test_gpu_denoise import Band, same
from test_gpu_noise import pairs, read_pfm, ref  # noqa: F401  (pairs: the module's fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
INPUTS = ("frame", "m2", "normal", "depth", "hist_frame", "hist_m2", "hist_count", "hist_normal", "hist_depth")


def upload(c, use_map):
    import torch
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k]).view(np.int32 if c[k].dtype == U32 else F32).copy()).cuda()
         for k in INPUTS}
    t["lmap"] = torch.from_numpy(c["lmap"].view(np.int32).copy()).cuda() if use_map else None
    return t


def check_inputs(t, c):
    for k in INPUTS:
        got = t[k].cpu().numpy()
        assert np.array_equal(got.view(U32), np.ascontiguousarray(c[k]).view(U32)), k + " is an input"


def run_reproject(ca, dev, c, x, y, layers, spp, tp, use_map, stream=0):
    import torch
    t = upload(c, use_map)
    out, m2o, cnt = Band(y, x, 3), Band(y, x, 3), Band(y, x)
    torch.cuda.synchronize()
    dev.reproject_device(camera_of(ca, c["cam_cur"]), camera_of(ca, c["cam_prev"]), x, y, layers, spp, tp,
                         t["frame"].data_ptr(),
                         t["m2"].data_ptr(), t["lmap"].data_ptr() if use_map else 0, t["normal"].data_ptr(),
                         t["depth"].data_ptr(), t["hist_frame"].data_ptr(), t["hist_m2"].data_ptr(),
                         t["hist_count"].data_ptr(), t["hist_normal"].data_ptr(), t["hist_depth"].data_ptr(), out.ptr,
                         m2o.ptr, cnt.ptr, stream)
    torch.cuda.synchronize()
    for b, what in ((out, "frame"), (m2o, "moments"), (cnt, "count")):
        b.assert_guards("merged " + what)
    check_inputs(t, c)
    return out.numpy(), m2o.numpy(), cnt.numpy().view(U32)


def camera_of(ca, arr):
    cam = ca.CrCamera()
    a = np.asarray(arr, F32)
    for i, f in enumerate(("eye", "left_upper", "dx", "dy")):
        for k in range(3):
            getattr(cam, f)[k] = float(a[3 * i + k])
    assert np.array_equal(cam.as_array().view(U32), a.view(U32))
    return cam


def compare(got, want, what):
    same(got[0], want[0], what + ": frame")
    same(got[1], want[1], what + ": moments")
    assert np.array_equal(got[2], want[2]), what + ": count"


# --- 1. cr_reproject_device on crafted inputs ----------------------------------------------------------------

PARAMS = (dict(), dict(max_history=1), dict(depth_tol=0.5, normal_min=-1.0, max_history=0xFFFFFFFF))


@pytest.mark.parametrize("x,y", [(1, 1), (7, 5), (33, 20), (70, 45)])
def test_reproject_device_matches_the_model(ca, pairs, x, y):
    import torch
    dev = pairs("cornell").dev
    layers, spp = 3, 2
    side = torch.cuda.Stream()
    before = dev.counters()
    found = 0
    for name in tc.PAIRS:
        c = tc.crafted(ca, x, y, name)
        for pi, params in enumerate(PARAMS):
            for use_map in (False, True):
                want = tc.crafted_ref(c, layers, spp, use_map, **params)
                got = run_reproject(ca, dev, c, x, y, layers, spp, ca.temporal_params(**params), use_map,
                                    stream=side.cuda_stream if (pi + use_map) % 2 else 0)
                compare(got, want, "%dx%d %s %r map %d" % (x, y, name, params, use_map))
                found += int(want[3].astype(bool).sum())
                if pi == 2 and x >= 33 and name == "identical":
                    assert want[2].max() == 0xFFFFFFFF, "the count saturates on this fixture"
    # (a one-pixel frame is the first edge case alone -- a NaN history pixel, so nothing is found there)
    assert found > 0 or x * y == 1, "no pixel of any pair found history"
    assert dev.counters() == before, "cr_reproject_device touched cr_get_counters"
    # layers * spp == 0 without a map: the history alone, or nothing
    c = tc.crafted(ca, x, y, "translated")
    want = tc.crafted_ref(c, 0, spp, False)
    compare(run_reproject(ca, dev, c, x, y, 0, spp, ca.temporal_params(), False), want, "%dx%d no current samples" % (x, y))
    assert (want[2] == want[3]).all()


@pytest.mark.parametrize("x,y", [(7, 5), (70, 45)])
def test_both_history_layouts_write_the_same_bits(ca, pairs, x, y):
    """The library's launcher on the planar arrays and on the packed record built from them by temporal_pack; the
    record the kernel writes beside its planar outputs holds those outputs and the current guides."""
    import ctypes as C
    import torch
    pairs("cornell")  # (a device context)
    launch, pack = tc.launchers(ca)
    npix = x * y
    for name in ("translated", "rotated", "identical"):
        c = tc.crafted(ca, x, y, name)
        want = tc.crafted_ref(c, 3, 2, True)
        t = upload(c, True)
        rec = Band(npix, 12)
        results = []
        for packed in (False, True):
            out, m2o, cnt, rec_out = Band(y, x, 3), Band(y, x, 3), Band(y, x), Band(npix, 12)
            torch.cuda.synchronize()
            if packed:
                assert pack(npix, t["hist_frame"].data_ptr(), t["hist_m2"].data_ptr(), t["hist_count"].data_ptr(),
                            t["hist_normal"].data_ptr(), t["hist_depth"].data_ptr(), rec.ptr, None) == 0
            ptrs = dict(layer_map=t["lmap"].data_ptr(), frame=t["frame"].data_ptr(), m2=t["m2"].data_ptr(),
                        normal=t["normal"].data_ptr(), depth=t["depth"].data_ptr(), out=out.ptr, m2_out=m2o.ptr,
                        count_out=cnt.ptr, rec_out=rec_out.ptr)
            if packed:
                ptrs["hist_rec"] = rec.ptr
            else:
                ptrs.update(hist_frame=t["hist_frame"].data_ptr(), hist_m2=t["hist_m2"].data_ptr(),
                            hist_count=t["hist_count"].data_ptr(), hist_normal=t["hist_normal"].data_ptr(),
                            hist_depth=t["hist_depth"].data_ptr())
            args = tc.tp_args(c["cam_cur"], c["cam_prev"], x, y, 3, 2, **ptrs)
            assert launch(C.byref(args), packed, None) == 0
            torch.cuda.synchronize()
            for b in (out, m2o, cnt, rec_out, rec):
                b.assert_guards("%s packed %d" % (name, packed))
            got = (out.numpy(), m2o.numpy(), cnt.numpy().view(U32))
            compare(got, want, "%dx%d %s packed %d" % (x, y, name, packed))
            r = rec_out.numpy().reshape(npix, 3, 4)
            same(r[:, 0, :3], got[0].reshape(npix, 3), "record: frame")
            assert np.array_equal(r[:, 0, 3].view(U32), got[2].reshape(-1)), "record: count bits"
            same(r[:, 1, :3], got[1].reshape(npix, 3), "record: moments")
            same(r[:, 1, 3], c["depth"].reshape(-1), "record: depth")
            same(r[:, 2, :3], c["normal"].reshape(npix, 3), "record: normal")
            assert not r[:, 2, 3].any()
            results.append(got)
        compare(results[1], results[0], "%dx%d %s packed against planar" % (x, y, name))


# --- 2. cr_render_temporal over three cameras ----------------------------------------------------------------

def render_chain(ca, dev, steps, dp=None, **params):
    """Each step through cr_render_temporal -> [(frame, count, history)]."""
    out = []
    for k, s in enumerate(steps):
        p = ca.render_params(tc.CX, tc.CY, tc.CSPP, tc.K, tc.SEED + k, layer=1)
        frame, count = dev.render_temporal(camera_of(ca, s["cam"]), p, 1, ca.temporal_params(**params), dp)
        out.append((frame, count, dev.temporal_history(tc.CX, tc.CY)))
    return out


def test_render_temporal_over_three_cameras(ca, pairs):
    pair = pairs("cornell")
    dev = pair.dev
    steps = tc.chain(ca, pair, tc.CX, tc.CY, tc.CSPP, 3)
    # the coverage conditions, on the model's own result
    for k in (1, 2):
        hit, carried, bare = tc.coverage(steps[k], tc.CSPP)
        assert carried * 2 >= hit and bare >= 1, (k, hit, carried, bare)
    # a progressive render first: its accumulators must survive the temporal frames
    cam0 = pair.camera(ca, tc.CX, tc.CY)
    frames = ref(ca, pairs, "cornell", tc.CX, tc.CY, tc.CSPP, 2)
    gf, gm = dev.render_layers_noise(cam0, ca.render_params(tc.CX, tc.CY, tc.CSPP, tc.K, tc.SEED, layer=1), 1)
    assert_bitwise(gf, frames[0][0], "layer 1")
    dev.temporal_reset()
    with pytest.raises(RuntimeError, match="CR_E_INVALID"):
        dev.temporal_history(tc.CX, tc.CY)
    for k, (frame, count, hist) in enumerate(render_chain(ca, dev, steps)):
        s = steps[k]
        same(frame, s["out"], "cr_render_temporal frame %d" % k)
        assert np.array_equal(count, s["count"]), "cr_render_temporal count %d" % k
        same(hist[0], s["out"], "history frame %d" % k)
        same(hist[1], s["m2_out"], "history moments %d" % k)
        assert np.array_equal(hist[2], s["count"]), "history count %d" % k
        if k == 0:
            assert_bitwise(frame, s["frame"], "the first frame is the plain frame")
        else:
            assert not np.array_equal(frame, s["frame"])
    gf, gm = dev.render_layers_noise(cam0, ca.render_params(tc.CX, tc.CY, tc.CSPP, tc.K, tc.SEED, layer=2), 1)
    assert_bitwise(gf, frames[1][0], "layer 2 after cr_render_temporal, frame")
    assert_bitwise(gm, frames[1][1], "layer 2 after cr_render_temporal, m2")
    # a frame of another size starts a new history
    p = ca.render_params(tc.CX - 1, tc.CY, tc.CSPP, tc.K, tc.SEED, layer=1)
    frame, count = dev.render_temporal(ca.camera(*steps[0]["view"], tc.CX - 1, tc.CY), p)
    assert (count == tc.CSPP).all()
    # other parameters through the mirror: max_history 1
    dev.temporal_reset()
    short = tc.chain(ca, pair, tc.CX, tc.CY, tc.CSPP, 3, max_history=1)
    got = render_chain(ca, dev, short, max_history=1)
    same(got[2][0], short[2]["out"], "max_history 1, frame 2")
    assert got[2][1].max() == tc.CSPP + 1 and not np.array_equal(short[2]["out"], steps[2]["out"])


# --- 3. with the denoiser; reset -------------------------------------------------------------------------------

def test_render_temporal_with_the_denoiser_and_reset(ca, pairs):
    pair = pairs("cornell")
    dev = pair.dev
    steps = tc.chain(ca, pair, tc.CX, tc.CY, tc.CSPP, 3)
    dev.temporal_reset()
    dp = ca.denoise_params(levels=2)
    for k, (frame, count, hist) in enumerate(render_chain(ca, dev, steps, dp=dp)):
        s, g = steps[k], steps[k]["guides"]
        want = dm.denoise_ref(s["out"], s["m2_out"], 1, 1, g["albedo"], g["normal"], g["depth"], layer_map=s["count"],
                              **dict(dm.DEFAULTS, levels=2))[0]
        same(frame, want, "denoised merged frame %d" % k)
        assert not np.array_equal(dm.canon(want), dm.canon(s["out"]))
        same(hist[0], s["out"], "the stored history stays unfiltered, frame %d" % k)
        same(hist[1], s["m2_out"], "... moments %d" % k)
        assert np.array_equal(count, s["count"]) and np.array_equal(hist[2], s["count"])
    # levels 0 through the same path: the merged frame itself
    dev.temporal_reset()
    got = render_chain(ca, dev, steps[:2], dp=ca.denoise_params(levels=0))
    same(got[1][0], steps[1]["out"], "levels 0")
    # reset: the next frame is the plain frame
    dev.temporal_reset()
    p = ca.render_params(tc.CX, tc.CY, tc.CSPP, tc.K, tc.SEED + 2, layer=1)
    frame, count = dev.render_temporal(camera_of(ca, steps[2]["cam"]), p)
    assert_bitwise(frame, steps[2]["frame"], "after cr_temporal_reset")
    assert (count == tc.CSPP).all()


# --- 4. the mirrors ----------------------------------------------------------------------------------------------

def small_scene(ca, scenes):
    return ca.Scene(scenes.config_rtc("cornell"), "xres", str(tc.CX), "yres", str(tc.CY), "samples", str(tc.CSPP))


def test_raytracer_raytrace_temporal(ca, pairs, scenes, tmp_path):
    import torch
    pair = pairs("cornell")
    steps = tc.chain(ca, pair, tc.CX, tc.CY, tc.CSPP, 3)
    scene = small_scene(ca, scenes)
    assert scene.info["seed"] == tc.SEED and scene.info["k"] == tc.K
    rt = ca.RayTracer(ca.Model(scene), scene)
    with pytest.raises(RuntimeError):
        rt.countMap()
    for k, s in enumerate(steps):
        least = rt.rayTraceTemporal(*s["view"])
        same(rt.denoisedData(), s["out"], "RayTracer.rayTraceTemporal frame %d" % k)
        assert np.array_equal(rt.countMap(), s["count"])
        assert least == int(s["count"][s["count"] > 0].min())
    out = tmp_path / "temporal.pfm"
    rt.exportImage(str(out))
    same(read_pfm(out), steps[2]["out"], "exportImage writes the temporal frame")
    rt.normalizeImage()
    t = ca.tonemap_params(scene.info["exposure"])
    d_rgb = torch.from_numpy(np.ascontiguousarray(steps[2]["out"])).cuda()
    d_bytes = torch.zeros(tc.CY * tc.CX * 3, dtype=torch.uint8, device="cuda")
    pair.dev.tonemap_device(t, tc.CX, tc.CY, d_rgb.data_ptr(), d_bytes.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(rt.getData().reshape(-1), d_bytes.cpu().numpy())
    # the next plain render starts at layer 1 and shows the rendered frame again
    rt.rayTrace(*steps[0]["view"])
    assert rt.layers == 1 and rt.denoisedData() is None
    assert_bitwise(rt.pixels, steps[0]["frame"], "rayTrace after rayTraceTemporal")
    # reset: a new history, the seed back at the scene's; with the filter on
    rt.resetTemporal()
    rt.rayTraceTemporal(*steps[0]["view"], denoiseLevels=2)
    s, g = steps[0], steps[0]["guides"]
    want = dm.denoise_ref(s["out"], s["m2_out"], 1, 1, g["albedo"], g["normal"], g["depth"], layer_map=s["count"],
                          **dict(dm.DEFAULTS, levels=2))[0]
    same(rt.denoisedData(), want, "rayTraceTemporal with denoiseLevels 2")
    rt.rayTraceTemporal(*steps[1]["view"])
    same(rt.denoisedData(), steps[1]["out"], "... and the history it left is unfiltered")


def preview_view(st):
    """PreviewSession::pressRender's arguments from the camera state."""
    pos, front = st["position"].astype(F32), st["front"].astype(F32)
    yview = float(F32(2 * math.tan(float(F32(st["zoom"])) * math.pi / 360.)))
    return (tuple(float(v) for v in pos), tuple(float(v) for v in (front + pos).astype(F32)),
            tuple(float(v) for v in st["up"]), yview)


def drive(pv, k):
    """Step k of the session: R, then back to the model view and a move / a look / a scroll."""
    if k == 0:
        pv.mouse(-900.0, 0.0)  # (the reference camera starts looking along +x, out of the box: test_gpu_preview.py)
    elif k == 1:
        pv.key("TAB")
        pv.key("D", 0.05)
        pv.key("W", 0.04)
    elif k == 2:
        pv.key("TAB")
        pv.mouse(12.0, -6.0)
        pv.scroll(1.5)
    pv.key("R")


def test_preview_session_temporal_on_and_off(ca, pairs, scenes):
    pair = pairs("cornell")
    # off (the default, and set explicitly): every press is what it is today -- a plain layer at the camera
    textures = []
    for explicit in (False, True):
        scene = small_scene(ca, scenes)
        rt = ca.RayTracer(ca.Model(scene), scene)
        pv = ca.Preview(scene, rt)
        if explicit:
            pv.set_temporal(False)
        tex = []
        for k in range(3):
            drive(pv, k)
            view = preview_view(pv.state())
            other = small_scene(ca, scenes)  # (a scene of its own: building a RayTracer adds to its scene's lights)
            plain = ca.RayTracer(ca.Model(other), other)
            plain.rayTrace(*view)
            plain.normalizeImage()
            assert np.array_equal(pv.texture(), plain.getData()), "temporal off, press %d" % k
            assert rt.denoisedData() is None and rt.layers == 1
            tex.append(pv.texture())
        textures.append(tex)
    assert all(np.array_equal(a, b) for a, b in zip(*textures))
    # on: the presses reproduce the chain of the model over the oracle's frames at the session's cameras
    scene = small_scene(ca, scenes)
    rt = ca.RayTracer(ca.Model(scene), scene)
    pv = ca.Preview(scene, rt)
    pv.set_temporal(True)
    hist = tc.tm.History()
    moved = 0
    for k in range(3):
        drive(pv, k)
        cam = ca.camera(*preview_view(pv.state()), tc.CX, tc.CY).as_array()
        frame, m2 = tc.oracle_frame(pair, cam, tc.CX, tc.CY, tc.CSPP, tc.SEED + k)
        g = dm.guides_ref(pair.oracle, pair.tris, cam, tc.CX, tc.CY)
        assert g["hit"].sum() > 100, "the session should look into the box"
        out, _, count, h = hist.step(cam, frame, m2, 1, tc.CSPP, g["normal"], g["depth"])
        same(rt.denoisedData(), out, "temporal on, press %d" % k)
        assert np.array_equal(rt.countMap(), count)
        moved += int(h.astype(bool).sum())
        assert np.array_equal(pv.texture(), rt.getData())
        assert k == 0 or (h.any() and not np.array_equal(out, frame)), "press %d should find history" % k
    assert moved > 0, "the session's moves should leave history to find"
    assert pv.state()["renders"] == 3
