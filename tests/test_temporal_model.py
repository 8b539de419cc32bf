"""The numpy restatement of temporal reprojection (tests/temporal_model.py; include/chiaro_hip.h "temporal
reprojection") on the CPU: the projector against a float64 solve, the unmoved camera, the merge's
cases, the coverage the GPU tests rely on, and what the history is worth against a converged render."""
import numpy as np
import pytest

import denoise_model as dm
import temporal_cases as tc
import temporal_model as tm
from helpers import Pair

F32 = np.float32
U32 = np.uint32


@pytest.fixture(scope="module")
def cornell(ca, po, scenes):
    return Pair(ca, po, scenes.config_rtc("cornell"), device=False)


def test_projector_matches_a_float64_solve(ca):
    """P = eye + t (lu + u dx + v dy): (t, t u, t v) solve the 3x3 system [lu dx dy] s = q.  The projector's Cramer
    form in float32 -- six products and three differences per cross product, five operations per dot product, one
    division -- is compared with numpy's float64 solve on points in front of each camera."""
    rng = np.random.default_rng(5)
    views = (((0, 0, 2), (0, 0, 0), (0, 1, 0), 1.0, 4, 4), ((278, 273, -800), (278, 273, 0), (0, 1, 0), 0.7, 64, 64),
             ((1.5, -2.25, 7.125), (0.3, 0.1, -0.2), (0.1, 1, 0.05), 0.3, 640, 360), ((0, 1, 2.95), (0, 1, 0), (0, 1, 0), 1.0, 24, 18))
    for e, c, u, yv, x, y in views:
        cam = ca.camera(e, c, u, yv, x, y).as_array()
        ra, rb, rc, det = tm.projector(cam)
        A = np.stack([cam[3:6], cam[6:9], cam[9:12]], axis=1).astype(np.float64)
        assert abs(float(det) - np.linalg.det(A)) <= 8 * np.spacing(F32(abs(np.linalg.det(A))))
        for _ in range(50):
            t, uu, vv = rng.uniform(0.5, 4.0), rng.uniform(0, x), rng.uniform(0, y)
            q64 = A @ np.array([t, t * uu, t * vv])
            q = q64.astype(F32)
            s = np.linalg.solve(A, q.astype(np.float64))
            a, b, cc = tm.dot(q, ra), tm.dot(q, rb), tm.dot(q, rc)
            got = np.array([a / det, b / a, cc / a], np.float64)
            want = np.array([s[0], s[1] / s[0], s[2] / s[0]])
            # a few ulps of the result's size, plus the cancellation in the dot products: their terms are up to
            # |q| |r| each, so the error is a few ulps of that over the size of a
            scale = float(np.linalg.norm(q64)) * max(float(np.linalg.norm(r)) for r in (ra, rb, rc)) / abs(float(a))
            tol = 8 * np.finfo(F32).eps * np.maximum(np.abs(want), scale)
            assert (np.abs(got - want) <= tol).all(), (e, got, want, tol)


def _flat_history(x, y, rng, cam):
    """A history without holes over the plane z = 0 as cam sees it."""
    z = tc._plane_depth(cam, x, y)
    nrm = np.broadcast_to(np.array([0, 0, 1], F32), (y, x, 3)).copy()
    h = rng.random((y, x, 3), dtype=F32)
    return h, (h * h * F32(1.5)).astype(F32), np.full((y, x), 8, U32), nrm, z


def test_unmoved_camera_finds_history_everywhere(ca):
    rng = np.random.default_rng(11)
    x, y = 33, 20
    cam = ca.camera((0.2, 0.1, 3.0), (0.2, 0.1, 0.0), (0, 1, 0), 1.0, x, y).as_array()
    H, H2, K, N, Z = _flat_history(x, y, rng, cam)
    Z[:3] = F32(-1)   # three rows of misses
    N[:3] = 0
    f = rng.random((y, x, 3), dtype=F32)
    m = (f * f * F32(2)).astype(F32)
    out, m2o, cnt, h = tm.reproject_ref(cam, cam, f, m, 1, 4, N, Z, H, H2, K, N, Z)
    hit = Z >= 0
    assert (h[hit] == 8).all() and (h[~hit] == 0).all()
    assert (cnt[hit] == 12).all() and (cnt[~hit] == 4).all()
    # a miss is the current pixel bit for bit; a hit the 8 : 4 blend of (about) its own history pixel
    assert np.array_equal(out[~hit].view(U32), f[~hit].view(U32)) and np.array_equal(m2o[~hit].view(U32), m[~hit].view(U32))
    want = (H.astype(np.float64) * 8 + f * 4) / 12
    assert np.abs(out[hit] - want[hit]).max() < 1e-4


def test_merge_cases_and_count_saturation(ca):
    rng = np.random.default_rng(12)
    x, y = 6, 4
    cam = ca.camera((0.2, 0.1, 3.0), (0.2, 0.1, 0.0), (0, 1, 0), 1.0, x, y).as_array()
    H, H2, K, N, Z = _flat_history(x, y, rng, cam)
    f = rng.random((y, x, 3), dtype=F32)
    m = (f * f * F32(2)).astype(F32)
    lmap = np.ones((y, x), U32)
    lmap[0, :2] = 0          # no current samples: the history alone
    K[1, :] = 0              # no history in row 1 ...
    lmap[1, 0] = 0           # ... and at (1, 0) nothing at all
    K[2, 0] = 0xFFFFFFFF
    out, m2o, cnt, h = tm.reproject_ref(cam, cam, f, m, 7, 3, N, Z, H, H2, K, N, Z, layer_map=lmap,
                                        max_history=0xFFFFFFFF)
    assert (h[0, :2] > 0).all() and (cnt[0, :2] == h[0, :2]).all()
    assert (cnt[1, 1:] == 3).all() and np.array_equal(out[1, 1:].view(U32), f[1, 1:].view(U32))
    assert cnt[1, 0] == 0 and not out[1, 0].any() and not m2o[1, 0].any()
    assert h[2, 0] == 0xFFFFFFFF and cnt[2, 0] == 0xFFFFFFFF    # saturates, does not wrap
    # max_history bounds the weight of the past
    out1, _, cnt1, h1 = tm.reproject_ref(cam, cam, f, m, 1, 3, N, Z, H, H2, K, N, Z, max_history=1)
    assert set(np.unique(h1)) == {0, 1} and cnt1.max() == 4
    # layers * spp wraps as a uint32
    assert tm.sample_counts(1, 1, 1 << 16, 1 << 16)[0, 0] == 0 and tm.sample_counts(1, 1, 65537, 65537)[0, 0] == 131073


@pytest.mark.parametrize("name", sorted(tc.PAIRS))
def test_crafted_pairs_exercise_what_they_name(ca, name):
    c = tc.crafted(ca, 33, 20, name)
    out, m2o, cnt, h = tc.crafted_ref(c, 1, 4, False)
    live = c["depth"] >= 0
    if name in ("behind", "far_outside"):
        assert not h.any()
        assert np.array_equal(dm.canon(out).view(U32), dm.canon(c["frame"]).view(U32))
    else:
        # history is found at a good share of the live pixels, and refused at some (depth gate, normals, holes)
        assert h[live].astype(bool).mean() > 0.2, name
        assert (h[live] == 0).any(), name
    assert np.isnan(c["hist_frame"]).any() and (c["hist_count"] == 0).any() and (c["hist_count"] > 0xFFFFFF00).any()
    # a NaN of the history never reaches a pixel that has current samples except through the current pixel itself
    assert np.array_equal(np.isnan(out).any(axis=2), np.isnan(c["frame"]).any(axis=2) | (np.isnan(out).any(axis=2) & (h > 0)))


def test_chain_meets_the_coverage_the_gpu_test_relies_on(ca, cornell):
    """cr_render_temporal's GPU test compares three frames of this chain (cornell 24x18, 1 layer x 2 spp): at the
    second and third cameras at least half of the hit pixels must carry history and at least one must carry none."""
    steps = tc.chain(ca, cornell, tc.CX, tc.CY, tc.CSPP, 3)
    hit0, carried0, _ = tc.coverage(steps[0], tc.CSPP)
    assert hit0 and carried0 == 0 and (steps[0]["count"] == tc.CSPP).all()
    assert (~steps[0]["guides"]["hit"]).any(), "the frame should hold misses too"
    for k in (1, 2):
        hit, carried, bare = tc.coverage(steps[k], tc.CSPP)
        assert carried * 2 >= hit and bare >= 1, (k, hit, carried, bare)
        assert not np.array_equal(steps[k]["cam"], steps[k - 1]["cam"])
    assert steps[2]["count"].max() == 3 * tc.CSPP


# Measured with this test (cornell 64x64, four frames of 4 spp along camera_path, seeds SEED .. SEED + 3, against a
# 512-spp render of seed QREF_SEED at the last camera; MSE over the hit pixels): merged 0.004384, the last frame alone
# 0.028498, 3878 of the 3904 hit pixels carry history, their mean count is 15.6 of 16
R_MEASURED = 0.154


def test_history_is_worth_its_samples(ca, cornell):
    """Four frames of 4 spp merged by the model against the last 4-spp frame alone, both measured against a 512-spp
    oracle render of another seed at the last camera: ratio = MSE(merged) / MSE(last frame) over the hit pixels.
    Four equal frames would ideally give 0.25; disocclusion costs some of that, and the bilinear taps give some back
    -- each averages up to four history pixels, which on the box's smooth walls removes more variance than it adds
    bias.  Measured: r = 0.154 (R_MEASURED).  The bound is sqrt(r) = 0.392, the geometric midpoint
    between what was measured and no gain at all: the test fails when history stops contributing without being
    pinned to the last digit."""
    steps = tc.chain(ca, cornell, tc.QX, tc.QY, tc.QSPP, tc.QFRAMES)
    last = steps[-1]
    ref, _ = cornell.oracle.render(last["cam"], tc.QX, tc.QY, tc.QREF_SPP, tc.K, tc.QREF_SEED, layer=1)
    hit = last["guides"]["hit"]
    mse = lambda a: float(np.mean((a[hit].astype(np.float64) - ref[hit]) ** 2))
    merged, alone = mse(last["out"]), mse(last["frame"])
    ratio = merged / alone
    print("temporal quality: MSE merged %.6g, last frame alone %.6g, ratio %.4f; carried %d of %d hit pixels, mean count %.2f"
          % (merged, alone, ratio, tc.coverage(last, tc.QSPP)[1], int(hit.sum()), float(last["count"][hit].mean())))
    assert ratio < np.sqrt(R_MEASURED)
