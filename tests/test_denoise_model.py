"""The definition of the guide buffers and the a-trous filter (tests/denoise_model.py) on the CPU: that it is sound
-- on the oracle's own noisy frame it more than halves the error against a high-spp render of another seed -- and
that its corner cases are what include/chiaro_hip.h promises.  No GPU.

Measured here (cornell 64x64, 4 spp, one layer, default parameters; truth 512 spp, seed + 1): MSE denoised / noisy
= 0.244.  The bound below, 0.5, is a condition with a 2x margin, not a tuned number."""
import numpy as np
import pytest

import denoise_model as dm
from helpers import Pair, assert_bitwise
from test_gpu_noise import K, SEED, oracle_moments

F32 = np.float32
X, Y, SPP = 64, 64, 4
_PAIRS = {}


@pytest.fixture(scope="module")
def pairs(ca, po, scenes):
    def get(name):
        if name not in _PAIRS:
            _PAIRS[name] = Pair(ca, po, scenes.config_rtc(name), device=False)
        return _PAIRS[name]
    yield get
    _PAIRS.clear()


@pytest.fixture(scope="module")
def cornell(ca, pairs):
    """The noisy frame and moments, the guides and the truth, computed once."""
    pair = pairs("cornell")
    cam = pair.camera(ca, X, Y).as_array()
    frame, m2 = oracle_moments(ca, pair, X, Y, SPP, 1)[0]
    truth, _ = pair.oracle.render(cam, X, Y, 512, K, SEED + 1)
    return {"frame": frame, "m2": m2, "truth": truth, "guides": dm.guides_ref(pair.oracle, pair.tris, cam, X, Y)}


def test_default_parameters_more_than_halve_the_error(cornell):
    g = cornell["guides"]
    out, var = dm.denoise_ref(cornell["frame"], cornell["m2"], 1, SPP, g["albedo"], g["normal"], g["depth"],
                              **dm.DEFAULTS)
    assert np.isfinite(out).all() and np.isfinite(var).all() and (var >= 0).all()
    truth = cornell["truth"].astype(np.float64)
    noisy = float(np.mean((cornell["frame"].astype(np.float64) - truth) ** 2))
    den = float(np.mean((out.astype(np.float64) - truth) ** 2))
    print("MSE noisy %.6g denoised %.6g ratio %.4f" % (noisy, den, den / noisy))
    assert noisy > 0 and den < 0.5 * noisy, (den, noisy, den / noisy)


def test_guide_reference_covers_hits_misses_and_textures(ca, po, pairs, cornell):
    g = cornell["guides"]
    assert g["hit"].any() and (~g["hit"]).any(), "cornell 64x64 must have hits and misses"
    miss = ~g["hit"]
    assert (g["depth"][miss] == F32(-1)).all() and not g["albedo"][miss].any() and not g["normal"][miss].any()
    assert (g["depth"][g["hit"]] >= 0).all()
    n = g["normal"][g["hit"]].astype(np.float64)
    assert np.allclose((n * n).sum(axis=1), 1.0, atol=1e-5)
    # the model's material normal and normalisation are the oracle's, bit for bit, on the scene's own triangles
    pair = pairs("cornell")
    L = po.lib()
    for vn in np.asarray(pair.tris["vnrm"], F32)[:12]:
        vn = np.ascontiguousarray(vn, F32)
        mn, nn = np.zeros(3, F32), np.zeros(3, F32)
        L.or_material_normal(po._p(vn), po._p(mn))
        L.or_glm_normalize(po._p(mn), po._p(nn))
        assert_bitwise(dm.material_normal(vn[None])[0], mn, "material normal")
        assert_bitwise(dm.normalize(mn), nn, "normalize")
    # nanobox 40x30: at least one textured first hit, whose albedo is the texel and not the plain Kd
    nb = pairs("nanobox")
    gn = dm.guides_ref(nb.oracle, nb.tris, nb.camera(ca, 40, 30).as_array(), 40, 30)
    assert gn["textured"].any() and (gn["hit"] & ~gn["textured"]).any()


def test_levels_0_is_the_identity(cornell):
    g = cornell["guides"]
    out, var = dm.denoise_ref(cornell["frame"], cornell["m2"], 1, SPP, g["albedo"], g["normal"], g["depth"],
                              **dict(dm.DEFAULTS, levels=0))
    assert_bitwise(out, cornell["frame"], "levels 0: the frame")
    assert_bitwise(var, dm.initial_variance(cornell["frame"], cornell["m2"], 1, SPP), "levels 0: the variance")
    assert (var > 0).any()


def test_a_planted_nan_pixel_stays_single(cornell):
    g = cornell["guides"]
    frame = cornell["frame"].copy()
    py, px = 31, 29
    assert g["hit"][py, px]
    frame[py, px, 1] = np.nan
    out, var = dm.denoise_ref(frame, cornell["m2"], 1, SPP, g["albedo"], g["normal"], g["depth"], **dm.DEFAULTS)
    bad = ~np.isfinite(out).all(axis=2)
    assert bad[py, px] and int(bad.sum()) == 1, np.argwhere(bad)[:8].tolist()
    assert np.isfinite(var[~bad]).all()
    # and the other pixels are what they are without that pixel's taps: finite, close to the clean result nearby
    clean, _ = dm.denoise_ref(cornell["frame"], cornell["m2"], 1, SPP, g["albedo"], g["normal"], g["depth"],
                              **dm.DEFAULTS)
    far = np.ones((Y, X), bool)
    far[max(0, py - 31):py + 32, max(0, px - 31):px + 32] = False  # 4 levels reach 2 * (1 + 2 + 4 + 8) = 30 pixels
    assert far.any()
    assert_bitwise(out[far], clean[far], "pixels out of the NaN pixel's reach")
