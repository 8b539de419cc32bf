"""The guide buffers and the a-trous filter on the GPU (include/chiaro_hip.h "guide buffers and denoiser", DESIGN.md
§3.25) against their numpy restatement (tests/denoise_model.py), bit for bit:

1. cr_guides_device / cr_guides against the restatement on the oracle's hits: hits and misses, textured triangles,
   each nullable output omitted, a non-default stream, guard bands;
2. cr_denoise_device on crafted inputs: every level count 0..5 at sizes from one pixel up (a step of 16 exceeds the
   small frames; 70x45 and 130x66 are several tiles with partial ones), with and without a layer map;
3. cr_denoise after a noise render equals the restatement on the oracle's frame, moments and guides, and the
   accumulators are untouched: the next layer is the oracle's;
4. cr_denoise after cr_render_adaptive, with its layer map;
5. RayTracer.denoise and the CLI's `denoise N`.

NaNs are compared as NaNs (denoise_model.canon): an invalid operation's default NaN has another sign on the host
than on the GPU; everything else is compared bit for bit.  The oracle's frames are test_gpu_noise's references
(computed once per shape and shared with it and test_gpu_adaptive)."""
import subprocess

import numpy as np
import pytest

import denoise_model as dm
from helpers import assert_bitwise
from test_gpu_adaptive import AD_CLI_T, adaptive_ref
from test_gpu_noise import (CLI_SPP, CLI_T, CLI_X, CLI_Y, FLOOR, K, POISON, SEED, UMAX, UNTIL_ABOVE, UNTIL_FLOOR,
                            UNTIL_T, USPP, UX, UY, first_stop, pairs, read_pfm, ref, until_sequence)

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 4096


class Band:
    """A device float buffer of `shape` between two poisoned guard bands."""

    def __init__(self, *shape):
        import torch
        self.shape, self.n = shape, int(np.prod(shape))
        self.t = torch.full((self.n + 2 * GUARD,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        self.ptr = self.t[GUARD:].data_ptr()

    def numpy(self):
        return self.t[GUARD:GUARD + self.n].cpu().numpy().reshape(self.shape)

    def untouched(self):
        import torch
        return bool((self.t.view(torch.int32) == POISON).all())

    def assert_guards(self, what):
        import torch
        bits = self.t.view(torch.int32).cpu().numpy()
        assert (bits[:GUARD] == POISON).all() and (bits[GUARD + self.n:] == POISON).all(), what + ": guard band"


def same(got, want, what):
    assert_bitwise(dm.canon(got), dm.canon(want), what)


# --- 1. guides ---------------------------------------------------------------------------------------------

_GUIDES = {}


def guides_of(ca, pairs, name, x, y):
    if (name, x, y) not in _GUIDES:
        pair = pairs(name)
        _GUIDES[(name, x, y)] = dm.guides_ref(pair.oracle, pair.tris, pair.camera(ca, x, y).as_array(), x, y)
    return _GUIDES[(name, x, y)]


@pytest.mark.parametrize("name,x,y", [("cornell", 33, 20), ("nanobox", 40, 30)])
def test_guides_match_the_restatement(ca, pairs, name, x, y):
    import torch
    pair = pairs(name)
    dev, cam = pair.dev, pair.camera(ca, x, y)
    want = guides_of(ca, pairs, name, x, y)
    if name == "cornell":
        assert want["hit"].any() and (~want["hit"]).any()
    else:
        assert want["textured"].any()
    before = dev.counters()
    stream = torch.cuda.Stream()
    shapes = {"albedo": (y, x, 3), "normal": (y, x, 3), "depth": (y, x)}
    for omit in (None, "albedo", "normal", "depth"):
        for st in (0, stream.cuda_stream):
            bands = {k: Band(*s) for k, s in shapes.items()}
            torch.cuda.synchronize()
            ptr = {k: 0 if k == omit else b.ptr for k, b in bands.items()}
            dev.guides_device(cam, x, y, ptr["albedo"], ptr["normal"], ptr["depth"], st)
            torch.cuda.synchronize()
            for k, b in bands.items():
                what = "%s %dx%d %s (omitted: %s, stream %d)" % (name, x, y, k, omit, st)
                if k == omit:
                    assert b.untouched(), what
                else:
                    b.assert_guards(what)
                    same(b.numpy(), want[k], what)
    assert dev.counters() == before, "cr_guides_device touched cr_get_counters"
    # the host-array form, whole and with two outputs omitted
    got = dev.guides(cam, x, y)
    for k in shapes:
        same(got[k], want[k], "cr_guides " + k)
    only = dev.guides(cam, x, y, want=("depth",))
    assert set(only) == {"depth"}
    same(only["depth"], want["depth"], "cr_guides, depth alone")


# --- 2. the filter on crafted inputs -------------------------------------------------------------------------

def crafted(x, y, variant="mixed"):
    """frame, m2 [y][x][3], albedo, normal [y][x][3], depth [y][x], layer map [y][x]: plausible random pixels over a
    few flat regions (equal albedo and normal, so weights near 1 occur), a band of misses, and from pixel 0 on (as
    far as the frame reaches) the edge cases."""
    rng = np.random.default_rng(1000 * x + y)
    n = x * y
    base = rng.random((n, 3), dtype=F32) * F32(2)
    region = (np.arange(n) // max(1, n // 5)) % 4                      # flat regions in row-major bands
    f = (base * F32(0.1) + (region[:, None].astype(F32) + F32(1)) * F32(0.3)).astype(F32)
    m = (f * f) * (F32(1) + rng.random((n, 3), dtype=F32) * F32(0.6))
    pal_a = np.array([[0.8, 0.8, 0.8], [0.8, 0.1, 0.1], [0.1, 0.8, 0.1], [0.5, 0.5, 0.9]], F32)
    pal_n = dm.normalize(np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1], [1, 1, 0]], F32))
    a, nr = pal_a[region].copy(), pal_n[region].copy()
    odd = rng.random(n) < 0.2                                           # some pixels off their region's values
    a[odd] = rng.random((int(odd.sum()), 3), dtype=F32)
    nr[odd] = dm.normalize(rng.random((int(odd.sum()), 3), dtype=F32) - F32(0.5))
    z = (F32(2) + region.astype(F32) + rng.random(n, dtype=F32) * F32(0.05)).astype(F32)
    miss = (np.arange(n) % x) >= (x * 3) // 4                           # the right quarter: hit / miss borders
    a[miss], nr[miss], z[miss] = 0, 0, F32(-1)
    lmap = rng.integers(1, 7, n).astype(np.uint32)
    nan, inf, sub = F32(np.nan), F32(np.inf), F32(1e-40)
    hitpix = dict(a=(0.8, 0.8, 0.8), n=(0, 1, 0), z=2.0)
    special = [
        dict(f=(0, 0, 0), m=(0, 0, 0), **hitpix),                       # zeros
        dict(f=(1.0, 2.0, 3.0), m=(0.5, 1.0, 2.0), **hitpix),           # m2 < mean^2 in every channel
        dict(f=(nan, 1.0, 1.0), m=(2.0, 2.0, 2.0), **hitpix),           # a NaN pixel
        dict(f=(inf, 1.0, 1.0), m=(inf, 2.0, 2.0), **hitpix),           # +inf
        dict(f=(1.0, -inf, 1.0), m=(2.0, inf, 2.0), **hitpix),          # -inf
        dict(f=(1.0, 1.0, 1.0), m=(nan, 2.0, 2.0), **hitpix),           # a NaN moment: that channel's variance is 0
        dict(f=(0.5, 0.5, 0.5), m=(0.3, 0.3, 0.3), a=(0.8, 0.8, 0.8), n=(0, 0, 0), z=2.0),      # a zero normal
        dict(f=(0.5, 0.5, 0.5), m=(0.3, 0.3, 0.3), a=(0.8, 0.8, 0.8), n=(nan, nan, nan), z=2.0),  # ... normalised
        dict(f=(0.5, 0.5, 0.5), m=(0.3, 0.3, 0.3), a=(0.8, 0.8, 0.8), n=(0, 1, 0), z=0.0),      # depth 0
        dict(f=(0.5, 0.5, 0.5), m=(0.3, 0.3, 0.3), a=(0.8, 0.8, 0.8), n=(0, 1, 0), z=0.0),      # ... beside another
        dict(f=(sub, sub, sub), m=(sub, sub, sub), **hitpix),           # subnormal mean and moment
        dict(f=(0, 0, 0), m=(sub, 0, 0), a=(sub, 0, 0), n=(0, 1, 0), z=sub),  # subnormal variance, albedo, depth
        dict(f=(1e30, 1.0, 1.0), m=(3e38, 2.0, 2.0), **hitpix),         # mean^2 overflows
        dict(f=(0.5, 0.5, 0.5), m=(0.3, 0.3, 0.3), a=(0, 0, 0), n=(0, 0, 0), z=-1.0),           # a miss among hits
    ]
    for i, sp in enumerate(special[:n]):
        f[i], m[i], a[i], nr[i], z[i] = (np.array(sp[k], F32) for k in ("f", "m", "a", "n", "z"))
    if variant == "zero_var":
        f = np.where(np.isfinite(f) & (np.abs(f) < 1e18), f, F32(1)).astype(F32)
        m = (f * f).astype(F32)                                         # v = 0 everywhere: den = 1e-8
    if variant == "all_miss":
        a[:], nr[:], z[:] = 0, 0, F32(-1)
    return (f.reshape(y, x, 3), m.reshape(y, x, 3), a.reshape(y, x, 3), nr.reshape(y, x, 3), z.reshape(y, x),
            lmap.reshape(y, x))


def run_denoise_device(ca, dev, x, y, layers, spp, dp, f, m, a, nr, z, lmap=None, want_var=True, stream=0):
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (f, m, a, nr, z)]
    dmap = torch.from_numpy(lmap.view(np.int32).copy()).cuda() if lmap is not None else None
    out, var = Band(y, x, 3), Band(y, x)
    torch.cuda.synchronize()
    dev.denoise_device(x, y, layers, spp, dp, t[0].data_ptr(), t[1].data_ptr(), dmap.data_ptr() if lmap is not None else 0,
                       t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), out.ptr, var.ptr if want_var else 0, stream)
    torch.cuda.synchronize()
    out.assert_guards("denoised frame")
    if want_var:
        var.assert_guards("variance")
    else:
        assert var.untouched(), "a null d_var_out was written"
    for got, src, what in zip(t, (f, m, a, nr, z), ("frame", "m2", "albedo", "normal", "depth")):
        same(got.cpu().numpy(), src, what + " is an input")
    return out.numpy(), var.numpy() if want_var else None


@pytest.mark.parametrize("x,y", [(1, 1), (3, 2), (17, 5), (70, 45), (130, 66)])
def test_denoise_device_matches_the_restatement(ca, pairs, x, y):
    import torch
    dev = pairs("cornell").dev
    layers, spp = 3, 4
    f, m, a, nr, z, lmap = crafted(x, y)
    if x * y > 14:
        assert np.isnan(f).any() and np.isinf(f).any() and (z == 0).any() and (z < 0).any() and (z > 0).any()
        assert (lmap.min(), lmap.max()) == (1, 6)
    side = torch.cuda.Stream()
    for levels in range(6):
        for use_map in (False, True):
            dp = ca.denoise_params(levels=levels)
            kw = dict(dm.DEFAULTS, levels=levels)
            want = dm.denoise_ref(f, m, layers, spp, a, nr, z, layer_map=lmap if use_map else None, **kw)
            got = run_denoise_device(ca, dev, x, y, layers, spp, dp, f, m, a, nr, z, lmap if use_map else None,
                                     stream=side.cuda_stream if levels == 3 else 0)
            what = "%dx%d levels %d map %d" % (x, y, levels, use_map)
            same(got[0], want[0], what + ": frame")
            same(got[1], want[1], what + ": variance")
            if levels == 0:
                same(got[0], f, what + ": the identity")
    # without the variance output; other parameters (no normal squaring, wide and narrow sigmas)
    dp = ca.denoise_params(levels=2, sigma_l=0.5, sigma_z=1.5, sigma_a=2.0, normal_squarings=0)
    want = dm.denoise_ref(f, m, layers, spp, a, nr, z, levels=2, sigma_l=0.5, sigma_z=1.5, sigma_a=2.0,
                          normal_squarings=0)
    got = run_denoise_device(ca, dev, x, y, layers, spp, dp, f, m, a, nr, z, want_var=False)
    same(got[0], want[0], "%dx%d other parameters, no variance output" % (x, y))
    dp = ca.denoise_params(levels=3, normal_squarings=8)
    want = dm.denoise_ref(f, m, layers, spp, a, nr, z, **dict(dm.DEFAULTS, levels=3, normal_squarings=8))
    got = run_denoise_device(ca, dev, x, y, layers, spp, dp, f, m, a, nr, z)
    same(got[0], want[0], "%dx%d 8 squarings: frame" % (x, y))
    same(got[1], want[1], "%dx%d 8 squarings: variance" % (x, y))
    # zero variance everywhere (den = 1e-8) and an all-miss guide set
    for variant in ("zero_var", "all_miss"):
        f2, m2, a2, n2, z2, _ = crafted(x, y, variant)
        if variant == "zero_var":
            assert not dm.initial_variance(f2, m2, layers, spp).any()
        for levels in (1, 4):
            want = dm.denoise_ref(f2, m2, layers, spp, a2, n2, z2, **dict(dm.DEFAULTS, levels=levels))
            got = run_denoise_device(ca, dev, x, y, layers, spp, ca.denoise_params(levels=levels), f2, m2, a2, n2, z2)
            same(got[0], want[0], "%dx%d %s levels %d: frame" % (x, y, variant, levels))
            same(got[1], want[1], "%dx%d %s levels %d: variance" % (x, y, variant, levels))


def test_a_nan_pixel_does_not_spread_on_the_gpu(ca, pairs):
    x, y = 70, 45
    f, m, a, nr, z, _ = crafted(x, y)
    got, _ = run_denoise_device(ca, pairs("cornell").dev, x, y, 3, 4, ca.denoise_params(), f, m, a, nr, z)
    assert np.array_equal(np.isnan(got).any(axis=2), np.isnan(f).any(axis=2))


# --- 3. cr_denoise after a noise render ----------------------------------------------------------------------

def test_denoise_of_the_accumulators_and_the_next_layer(ca, pairs):
    pair = pairs("cornell")
    dev, cam = pair.dev, pair.camera(ca, UX, UY)
    frames = ref(ca, pairs, "cornell", UX, UY, USPP, 3)
    g = guides_of(ca, pairs, "cornell", UX, UY)
    gf, gm = dev.render_layers_noise(cam, ca.render_params(UX, UY, USPP, K, SEED, layer=1), 2)
    assert_bitwise(gf, frames[1][0], "frame after 2 layers")
    for levels in (4, 0, 1):
        want = dm.denoise_ref(frames[1][0], frames[1][1], 2, USPP, g["albedo"], g["normal"], g["depth"],
                              **dict(dm.DEFAULTS, levels=levels))
        out, var = dev.denoise(cam, UX, UY, 2, USPP, ca.denoise_params(levels=levels))
        same(out, want[0], "cr_denoise levels %d: frame" % levels)
        same(var, want[1], "cr_denoise levels %d: variance" % levels)
    out, var = dev.denoise(cam, UX, UY, 2, USPP, want_var=False)
    assert var is None
    same(out, dm.denoise_ref(frames[1][0], frames[1][1], 2, USPP, g["albedo"], g["normal"], g["depth"])[0], "defaults")
    assert not np.array_equal(out, frames[1][0])
    # the accumulators were left alone: layer 3 on the same ctx is the oracle's, frame and moments
    gf, gm = dev.render_layers_noise(cam, ca.render_params(UX, UY, USPP, K, SEED, layer=3), 1)
    assert_bitwise(gf, frames[2][0], "layer 3 after cr_denoise, frame")
    assert_bitwise(gm, frames[2][1], "layer 3 after cr_denoise, m2")
    # accumulators of another size
    with pytest.raises(RuntimeError, match="CR_E_INVALID"):
        dev.denoise(cam, UX + 1, UY, 2, USPP)


# --- 4. cr_denoise after cr_render_adaptive ------------------------------------------------------------------

def test_denoise_of_an_adaptive_frame_uses_its_layer_map(ca, pairs):
    pair = pairs("cornell")
    dev, cam = pair.dev, pair.camera(ca, UX, UY)
    frames = ref(ca, pairs, "cornell", UX, UY, USPP, UMAX)
    wf, wm, wmap, wst, _ = adaptive_ref(frames, USPP, 1, UMAX, 1, UNTIL_T, UNTIL_FLOOR)
    assert len(np.unique(wmap)) >= 3
    g = guides_of(ca, pairs, "cornell", UX, UY)
    gf, gm, gmap, gst = dev.render_adaptive(cam, ca.render_params(UX, UY, USPP, K, SEED, layer=1), 1, UMAX, 1, UNTIL_T,
                                            UNTIL_FLOOR)
    assert np.array_equal(gmap, wmap)
    want = dm.denoise_ref(wf, wm, gst["layers"], USPP, g["albedo"], g["normal"], g["depth"], layer_map=wmap)
    out, var = dev.denoise(cam, UX, UY, gst["layers"], USPP, layer_map=gmap)
    same(out, want[0], "adaptive frame denoised with its layer map: frame")
    same(var, want[1], "adaptive frame denoised with its layer map: variance")
    flat = dm.denoise_ref(wf, wm, gst["layers"], USPP, g["albedo"], g["normal"], g["depth"])
    assert not np.array_equal(want[0], flat[0]), "the layer map must matter on this fixture"


# --- 5. the mirrors ------------------------------------------------------------------------------------------

def test_raytracer_denoise(ca, pairs, scenes, tmp_path):
    import torch
    seq = until_sequence(ca, pairs, "cornell", UX, UY, USPP, UNTIL_T, UNTIL_FLOOR)
    stop = first_stop(seq, UNTIL_ABOVE)
    frames = ref(ca, pairs, "cornell", UX, UY, USPP, UMAX)
    g = guides_of(ca, pairs, "cornell", UX, UY)
    scene = ca.Scene(scenes.config_rtc("cornell"), "xres", str(UX), "yres", str(UY), "samples", str(USPP))
    i = scene.info
    rt = ca.RayTracer(ca.Model(scene), scene)
    view = (i["VP"], i["LA"], i["UP"], i["yview"])
    # a frame without complete moments: denoise throws and nothing is shown
    rt.rayTrace(*view)
    with pytest.raises(RuntimeError, match="moments"):
        rt.denoise()
    assert rt.denoisedData() is None
    # a rayTraceUntil frame
    assert rt.rayTraceUntil(UNTIL_T, UMAX, *view, floor=UNTIL_FLOOR, checkEvery=1, maxAbove=UNTIL_ABOVE) == stop
    want = dm.denoise_ref(frames[stop - 1][0], frames[stop - 1][1], stop, USPP, g["albedo"], g["normal"], g["depth"])[0]
    same(rt.denoise(), want, "RayTracer.denoise")
    same(rt.denoisedData(), want, "RayTracer.denoisedData")
    assert_bitwise(rt.pixels, frames[stop - 1][0], "the rendered frame stays")
    out = tmp_path / "denoised.pfm"
    rt.exportImage(str(out))
    same(read_pfm(out), want, "exportImage writes the denoised frame")
    # normalizeImage / getData act on the denoised frame: the device tonemap of exactly that frame
    rt.normalizeImage()
    t = ca.tonemap_params(i["exposure"])
    d_rgb = torch.from_numpy(np.ascontiguousarray(want)).cuda()
    d_bytes = torch.zeros(UY * UX * 3, dtype=torch.uint8, device="cuda")
    pairs("cornell").dev.tonemap_device(t, UX, UY, d_rgb.data_ptr(), d_bytes.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(rt.getData().reshape(-1), d_bytes.cpu().numpy())
    # other parameters through the mirror
    want2 = dm.denoise_ref(frames[stop - 1][0], frames[stop - 1][1], stop, USPP, g["albedo"], g["normal"], g["depth"],
                           levels=2, sigma_l=2.0, sigma_z=0.5, sigma_a=0.3, normal_squarings=1)[0]
    same(rt.denoise(2, 2.0, 0.5, 0.3, 1), want2, "RayTracer.denoise, other parameters")
    # the progressive state is untouched, and the next render shows the rendered frame again
    assert rt.rayTraceUntil(1e9, UMAX, *view, floor=UNTIL_FLOOR, checkEvery=1) == stop + 1
    assert_bitwise(rt.pixels, frames[stop][0], "continued accumulation after denoise")
    assert rt.denoisedData() is None


def test_raytracer_denoise_of_an_adaptive_frame(ca, pairs, scenes):
    frames = ref(ca, pairs, "cornell", CLI_X, CLI_Y, CLI_SPP, UMAX)
    wf, wm, wmap, wst, _ = adaptive_ref(frames, CLI_SPP, 1, UMAX, 1, AD_CLI_T, FLOOR)
    g = guides_of(ca, pairs, "cornell", CLI_X, CLI_Y)
    scene = ca.Scene(scenes.config_rtc("cornell"), "xres", str(CLI_X), "yres", str(CLI_Y), "samples", str(CLI_SPP))
    i = scene.info
    rt = ca.RayTracer(ca.Model(scene), scene)
    rt.rayTraceAdaptive(AD_CLI_T, UMAX, i["VP"], i["LA"], i["UP"], i["yview"], floor=FLOOR, minLayers=1, checkEvery=1)
    want = dm.denoise_ref(wf, wm, wst["layers"], CLI_SPP, g["albedo"], g["normal"], g["depth"], layer_map=wmap,
                          **dict(dm.DEFAULTS, levels=3))[0]
    same(rt.denoise(3), want, "RayTracer.denoise of an adaptive frame")


def test_cli_denoise_token(ca, pairs, scenes, tmp_path):
    seq = until_sequence(ca, pairs, "cornell", CLI_X, CLI_Y, CLI_SPP, CLI_T, FLOOR)
    stop = first_stop(seq, 0)
    f, m = ref(ca, pairs, "cornell", CLI_X, CLI_Y, CLI_SPP, UMAX)[stop - 1]
    g = guides_of(ca, pairs, "cornell", CLI_X, CLI_Y)
    want = dm.denoise_ref(f, m, stop, CLI_SPP, g["albedo"], g["normal"], g["depth"], **dict(dm.DEFAULTS, levels=3))[0]
    out = tmp_path / "denoised.pfm"
    exe = scenes.default_dir().parent.parent / "bin" / "chiaroscuro"
    base = [str(exe), str(scenes.config_rtc("cornell")), "xres", str(CLI_X), "yres", str(CLI_Y), "samples",
            str(CLI_SPP), "output", str(out), "layers", str(UMAX)]
    r = subprocess.run(base + ["noise", repr(CLI_T), "denoise", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "denoise 3: 3 a-trous level(s) over %d layer(s)" % stop in r.stderr, r.stderr
    same(read_pfm(out), want, "cli noise T denoise 3, PFM")
    # denoise alone has no moments to work with: one line, exit 1, nothing rendered
    out2 = tmp_path / "none.pfm"
    base[base.index(str(out))] = str(out2)
    r = subprocess.run(base + ["denoise", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and len(r.stderr.strip().splitlines()) == 1 and "denoise" in r.stderr, r.stderr
    assert not out2.exists()
