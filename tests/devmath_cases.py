"""Case generators and host-side expected values of the device known-answer tests (tests/native/devmath_check.hip,
tests/test_gpu_devmath.py) -- the inputs as the flat uint32 records the harness reads, the expected output words
from the oracle (pyoracle) or from a numpy float32 restatement in the reference's operation order, and the coverage
facts tests/test_rng_distributions.py asserts on the CPU, so that an edit here cannot hollow the GPU tests out.

Nothing here touches a GPU or the code under test (csrc/device_math.hpp, csrc/render_common.hpp).
"""
from __future__ import annotations

import functools
import json
from pathlib import Path

import numpy as np

import pyoracle as po

ROOT = Path(__file__).resolve().parents[1]
U32 = np.uint32
F32 = np.float32
M32 = 0xFFFFFFFF
GOLDEN_RATIO = 0x9E3779B9
NAN = 0x7FC00000
SENTINEL = 0xDEADBEEF  # devmath_check.hip WAVE_SENTINEL


def f32(bits):
    return np.asarray(bits, U32).view(F32)


def bits(x):
    return np.ascontiguousarray(x, F32).view(U32)


def b1(x):
    """The bit pattern of one float32, as a Python int."""
    return int(np.array(x, F32).view(U32))


def same_words(got, exp, float_cols=None):
    """Bit for bit, NaN compared as NaN in the float columns (all columns when float_cols is None): the mask of
    mismatching words."""
    got, exp = np.asarray(got, U32), np.asarray(exp, U32)
    bad = got != exp
    both_nan = np.isnan(got.view(F32)) & np.isnan(exp.view(F32))
    if float_cols is not None:
        keep = np.zeros(got.shape[-1], bool)
        keep[list(float_cols)] = True
        both_nan = both_nan & keep
    return bad & ~both_nan


# ---------------------------------------------------------------- RNG --
def mix32(x):
    """oracle.c / device_math.hpp mix32 on Python ints or uint32 arrays."""
    if isinstance(x, np.ndarray):
        x = x.astype(np.uint64)
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
        x ^= x >> np.uint64(15)
        x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
        x ^= x >> np.uint64(16)
        return x.astype(U32)
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


_INV1, _INV2 = pow(0x7FEB352D, -1, 1 << 32), pow(0x846CA68B, -1, 1 << 32)


def unmix32(y):
    """mix32 is a bijection (xorshifts and odd multiplies); its inverse, step by step from the end."""
    y &= M32
    y ^= y >> 16
    y = (y * _INV2) & M32
    y ^= (y >> 15) ^ (y >> 30)
    y = (y * _INV1) & M32
    y ^= y >> 16
    return y


def rng_key(seed, layer, pixel, sample):
    return mix32(mix32(mix32(mix32(seed) ^ layer) ^ pixel) ^ sample)


def raw_draws(key, ctr, n):
    return [mix32((key + (ctr + i) * GOLDEN_RATIO) & M32) for i in range(n)]


EDGE_DRAWS = (0, 1, 0x7F, 0x80, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFF81, 0xFFFFFFFF)
INDEX_N = (1, 2, 3, 5, 7, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 3 * 2 ** 30, 2 ** 32 - 1)
N_STREAMS = 4096


def lemire_threshold(n):
    return ((1 << 32) - n) % n


def clamps(draw):
    """rng_uniform's c >= 1.0f branch: the draw rounds to 2^32 as a float."""
    return bool(F32(draw) / F32(4294967296.0) >= F32(1.0))


@functools.lru_cache(maxsize=None)
def rng_streams():
    """(seed, layer, pixel, sample) of the random streams: small fields as the renderer's, and full 32-bit ones."""
    r = np.random.default_rng(0xD17A)
    s = r.integers(0, 1 << 32, size=(N_STREAMS, 4), dtype=np.uint64).astype(U32)
    small = np.arange(N_STREAMS) % 2 == 0
    s[small, 1] = r.integers(1, 64, small.sum())
    s[small, 2] = r.integers(0, 3840 * 2160, small.sum())
    s[small, 3] = r.integers(0, 64, small.sum())
    return s


@functools.lru_cache(maxsize=None)
def rng_draw_cases():
    """Pass 1 of the rng stage: raw draws and rng_uniform (which cannot loop).  Returns (records [n][8], expected
    [n][14], facts)."""
    rec, exp = [], []
    n_clamp = 0

    def uniform_case(kind, w, key, ctr, a, b):
        nonlocal n_clamp
        val, c1 = po.rng_uniform_kat(key, ctr, a, b)
        rec.append([kind, *w, 1, b1(a), b1(b)])
        d = raw_draws(key, ctr, 8)
        exp.append([key, *d, (ctr + 8) & M32, b1(val), c1, 0, 0])
        n_clamp += clamps(d[0])

    for seed, layer, pixel, sample in rng_streams().tolist():
        key = rng_key(seed, layer, pixel, sample)
        w = (seed, layer, pixel, sample)
        uniform_case(0, w, key, 0, 0.0, 1.0)
        uniform_case(0, w, key, 0, -1.0, 1.0)
        # the third call shape: v1 = rng_uniform(0, 1 - v0) right after v0 = rng_uniform(0, 1)
        v0, c1 = po.rng_uniform_kat(key, 0, 0.0, 1.0)
        uniform_case(1, (key, c1, 0, 0), key, c1, 0.0, F32(1.0) - v0)
    # crafted first draws, with every 1 - v0 the crafted draws themselves give
    v0s = [po.rng_uniform_kat(unmix32(d), 0, 0.0, 1.0)[0] for d in EDGE_DRAWS]
    for d in EDGE_DRAWS:
        key = unmix32(d)
        assert raw_draws(key, 0, 1)[0] == d
        for ctr0 in (0, 5, M32):  # the same draw reached at another counter (and across its wrap)
            k = (key - ctr0 * GOLDEN_RATIO) & M32
            w = (k, ctr0, 0, 0)
            uniform_case(1, w, k, ctr0, 0.0, 1.0)
            uniform_case(1, w, k, ctr0, -1.0, 1.0)
            for v0 in v0s:
                uniform_case(1, w, k, ctr0, 0.0, F32(1.0) - v0)
    return np.array(rec, U32), np.array(exp, U32), {"clamp": n_clamp}


def _index_case(rec, exp, rej, key, ctr, n):
    val, c1 = po.rng_index_kat(key, ctr, n)
    rec.append([1, key, ctr, 0, 0, 2, n, 0])
    exp.append([key, *raw_draws(key, ctr, 8), (ctr + 8) & M32, 0, 0, val, c1])
    rej.append(((c1 - ctr) & M32) - 1)


def crafted_index_streams():
    """(key, n, k, low): streams whose first k draws reject (low word below the threshold) and whose draw k has the
    low word `low` = thr - 1 (one more rejection, at the boundary) or thr (the first accepted value).  The stream
    has one free word, so the draw k is solved for (n odd: u -> u * n mod 2^32 is a bijection) and odd n upward
    from 2^31 + 1 (thr = 2^32 - n, about half of all draws reject) are searched until the k draws before it reject."""
    out = []
    for k in (0, 1, 2, 3):
        for which in (-1, 0):
            n = 2 ** 31 + 1
            while True:
                thr = lemire_threshold(n)
                low = thr + which
                u = (low * pow(n, -1, 1 << 32)) & M32
                key = (unmix32(u) - k * GOLDEN_RATIO) & M32
                d = raw_draws(key, 0, k + 1)
                assert d[k] == u and (u * n) & M32 == low
                if all(((x * n) & M32) < thr for x in d[:k]):
                    out.append((key, n, k, low))
                    break
                n += 2
    # every n of the list with a non-empty rejection range: the first draw on thr - 1 and on thr
    for n in INDEX_N:
        thr = lemire_threshold(n)
        if thr == 0:
            continue
        for low in (thr - 1, thr):
            if n % 2:
                us = [(low * pow(n, -1, 1 << 32)) & M32]
            else:  # 3 * 2^30: the low word takes four values only
                us = [u for u in range(8) if (u * n) & M32 == low]
            for u in us:
                out.append((unmix32(u), n, 0, low))
    return out


@functools.lru_cache(maxsize=None)
def rng_index_cases():
    """Pass 2 of the rng stage, run only after pass 1 passed (rng_index's loop ends exactly when the draws are the
    CPU's).  Returns (records, expected, facts): facts["rejections"] = how many cases reject 0, 1, 2, >= 3 times."""
    rec, exp, rej = [], [], []
    keys = [rng_key(*s) for s in rng_streams().tolist()]
    for n in INDEX_N:
        for i, key in enumerate(keys):
            _index_case(rec, exp, rej, key, i % 3, n)
    crafted = crafted_index_streams()
    for key, n, k, low in crafted:
        at = len(rej)
        _index_case(rec, exp, rej, key, 0, n)
        thr = lemire_threshold(n)
        assert rej[at] >= k + (1 if low < thr else 0), (key, n, k, low, rej[at])
        if low >= thr:
            assert rej[at] == k
    rej = np.array(rej)
    facts = {"rejections": [int((rej == 0).sum()), int((rej == 1).sum()), int((rej == 2).sum()),
                            int((rej >= 3).sum())],
             "crafted": len(crafted),
             "crafted_boundary": sorted({(k, low - lemire_threshold(n)) for _, n, k, low in crafted if n > 2 ** 31}),
             "rejecting_small_n": int(sum(1 for r, c in zip(rej, rec) if r > 0 and c[6] <= 7))}
    return np.array(rec, U32), np.array(exp, U32), facts


# ------------------------------------------------------------- minmax --
MINMAX_VALUES = (NAN, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x3F800000)  # NaN, +0, -0, +inf, -inf, 1


def minmax_cases():
    rec = np.array([[a, b] for a in MINMAX_VALUES for b in MINMAX_VALUES], U32)
    exp = []
    for ab, bb in rec.tolist():
        a, b = f32(ab)[()], f32(bb)[()]
        std_min = bb if b < a else ab  # (b < a) ? b : a
        std_max = bb if a < b else ab  # (a < b) ? b : a
        glm_max = ab if a > b else bb  # x > y ? x : y
        exp.append([std_min, std_max, glm_max])
    return rec, np.array(exp, U32)


# --------------------------------------------------------------- BRDF --
def brdf_edge_values():
    mags = [2.0 ** -149, 2.0 ** -126, 2.0 ** -24, 0.25, 0.5, 1.0 - 2.0 ** -23, 1.0 - 2.0 ** -24, 1.0]
    v = [0.0, -0.0]
    for m in mags:
        v += [m, -m]
    v = np.array(v, F32)
    assert len(set(bits(v).tolist())) == 18
    return v


@functools.lru_cache(maxsize=None)
def brdf_normals():
    r = np.random.default_rng(0xB2DF)
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    c = F32(0.70710677)
    ties = [(0.5, 0.5, c), (0.5, -0.5, c), (-0.5, 0.5, c), (-0.5, -0.5, -c), (c, c, 0.0), (-c, c, 0.0)]
    rnd = r.standard_normal((64, 3))
    rnd = (rnd / np.linalg.norm(rnd, axis=1, keepdims=True)).astype(F32)
    odd = [(3.0, 4.0, 12.0), (1e-3, 2e-3, -1e-3), (2.0 ** -140, 2.0 ** -141, 0.0), (0.0, 2.0 ** -149, 2.0 ** -130),
           (2.0 ** 70, 2.0 ** 70, 1.0)]
    zero = [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)]
    return np.concatenate([np.array(axes, F32), np.array(ties, F32), rnd, np.array(odd, F32), np.array(zero, F32)])


N_BRDF_RANDOM = 1 << 15


@functools.lru_cache(maxsize=None)
def brdf_pairs():
    """(sx, sy): the full edge grid, then 2^15 pairs that are real rng_uniform(-1, 1) outputs of one stream."""
    e = brdf_edge_values()
    grid = np.array([(a, b) for a in e for b in e], F32)
    key = rng_key(0xC41A05C0, 1, 12345, 0)
    rnd = np.array([po.rng_uniform_kat(key, i, -1.0, 1.0)[0] for i in range(2 * N_BRDF_RANDOM)], F32).reshape(-1, 2)
    return grid, rnd


def concentric_branch(sx, sy):
    """Which assignment of concentric() (src/brdf.cpp:18-54) the pair takes: 0 the (0, 0) return, 1..5 the five
    (r, theta) assignments in source order."""
    sx, sy = F32(sx), F32(sy)
    if sx == 0 and sy == 0:
        return 0
    if sx >= -sy:
        if sx > sy:
            return 1 if sy > 0 else 2
        return 3
    return 4 if sx <= sy else 5


def perpendicular(n):
    """src/brdf.cpp:10-15 on [k][3] float32."""
    n = np.asarray(n, F32)
    first = (np.abs(n[:, 0]) < np.abs(n[:, 1]))[:, None]
    z = np.zeros(len(n), F32)
    return np.where(first, np.stack([z, -n[:, 2], n[:, 1]], 1), np.stack([-n[:, 2], z, n[:, 0]], 1)).astype(F32)


@functools.lru_cache(maxsize=None)
def brdf_cases():
    """Records [n][5] and expected [n][9].  The edge grid is crossed with every normal; the random pairs, which
    sit on no branch boundary, take the normals in turn (the stage stays at a few times 10^4 cases)."""
    grid, rnd = brdf_pairs()
    normals = brdf_normals()
    nn = np.concatenate([np.repeat(normals, len(grid), 0), normals[np.arange(len(rnd)) % len(normals)]])
    pairs = np.concatenate([np.tile(grid, (len(normals), 1)), rnd])
    rec = np.concatenate([bits(nn), bits(pairs)], 1)
    exp = np.zeros((len(rec), 9), U32)
    exp[:, 0:3] = bits(perpendicular(nn))
    conc = {}
    branches = np.zeros(6, np.int64)
    n_pdf0 = n_hz0 = n_nan = 0
    with np.errstate(all="ignore"):
        for i in range(len(rec)):
            sx, sy = pairs[i]
            k = (int(rec[i, 3]), int(rec[i, 4]))
            if k not in conc:
                conc[k] = po.concentric(sx, sy)
                branches[concentric_branch(sx, sy)] += 1
            hx, hy = F32(conc[k][0]), F32(conc[k][1])
            exp[i, 3:5] = bits(np.array([hx, hy], F32))
            wi, pdf = po.sample_wi(nn[i], sx, sy)
            exp[i, 5:8] = bits(wi)
            exp[i, 8] = b1(pdf)
            n_pdf0 += pdf == 0.0
            n_nan += pdf != pdf
            n_hz0 += bool(F32(F32(F32(1.0) - hx * hx) - hy * hy) < 0)  # std_max(0.f, 1.f - hx * hx - hy * hy)
    facts = {"branches": branches.tolist(), "pdf_zero": int(n_pdf0), "hz_clamped": int(n_hz0),
             "pdf_nan": int(n_nan), "pairs": len(conc)}
    return rec, exp, facts


# --------------------------------------------------------------- wave --
MASKS = {"full": M32 | (M32 << 32), "low32": M32, "alternate": 0xAAAAAAAAAAAAAAAA, "single": None}
LANE_PATTERNS = (("0", ()), ("1@0", (0,)), ("1@31", (31,)), ("1@32", (32,)), ("1@63", (63,)), ("32", None),
                 ("63", None), ("64", tuple(range(64))))
WAVE_REPEATS = 4
EPS = F32(1.19209290e-7)


def _rand_f32(r, n, emin, emax):
    """Random sign and mantissa, exponent uniform in [emin, emax]."""
    e = r.integers(emin + 127, emax + 128, n).astype(U32)
    return f32((r.integers(0, 2, n).astype(U32) << U32(31)) | (e << U32(23)) | r.integers(0, 1 << 23, n).astype(U32))


def _rcp_out_of_range(r, n):
    """Zeros, denormals, infinities, NaN and normals outside [2^-100, 2^100], both signs."""
    pool = np.concatenate([
        f32([0, 0x80000000, 1, 0x80000001, 0x007FFFFF, 0x00400000, 0x7F800000, 0xFF800000, NAN, 0xFFC00001]),
        np.array([2.0 ** 101, -2.0 ** 101, 2.0 ** -101, -2.0 ** -126, 2.0 ** 127], F32),
        np.nextafter(F32(2.0 ** -100), F32(0), dtype=F32)[None], np.nextafter(F32(2.0 ** 100), F32(np.inf))[None],
        _rand_f32(r, 4, 101, 127), _rand_f32(r, 4, -126, -101)]).astype(F32)
    return pool[r.integers(0, len(pool), n)]


def rcp_in_range(a):
    a = np.abs(np.asarray(a, F32))
    return (a >= F32(2.0 ** -100)) & (a <= F32(2.0 ** 100))


def div_in_range(a, b):
    """div_by_rcp_wave's `in` with y = rcp_for_div(b): NaN outside 2^-40 <= |b| <= 2^40."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(all="ignore"):
        ab = np.abs(b)
        y = np.where((ab >= F32(2.0 ** -40)) & (ab <= F32(2.0 ** 40)), F32(1) / b, F32(np.nan)).astype(F32)
        q0 = np.abs(a * y)
    return (q0 >= F32(2.0 ** -60)) & (q0 <= F32(2.0 ** 60))


def _cross(x, y):
    # func_geometric.inl:77-83
    return np.stack([x[:, 1] * y[:, 2] - y[:, 1] * x[:, 2], x[:, 2] * y[:, 0] - y[:, 2] * x[:, 0],
                     x[:, 0] * y[:, 1] - y[:, 0] * x[:, 1]], 1)


def _dot(a, b):
    t = a * b
    return t[:, 0] + t[:, 1] + t[:, 2]


def tri_model(o, d, v0, e1, e2, tmax):
    """kdtree.cpp:219-246 on float32 arrays, in the oracle's operation order (oracle.c tri_test, with the caller's
    t < tmax): accept, ux, uy, t.  Every operation is one float32 numpy operation, so nothing is contracted."""
    o, d, v0, e1, e2 = (np.asarray(x, F32) for x in (o, d, v0, e1, e2))
    with np.errstate(all="ignore"):
        p = _cross(d, e2)
        aa = _dot(e1, p)
        ok = ~((aa < EPS) & (aa > -EPS))
        f = F32(1.0) / aa
        sv = o - v0
        ux = f * _dot(sv, p)
        ok &= ~((ux < 0) | (ux > 1))
        q = _cross(sv, e1)
        uy = f * _dot(d, q)
        ok &= ~((uy < 0) | (uy + ux > 1))
        t = f * _dot(e2, q)
        ok &= (t >= 0) & (t < np.asarray(tmax, F32))
    return ok, ux.astype(F32), uy.astype(F32), t.astype(F32), aa.astype(F32)


def _std_min(a, b):
    return np.where(b < a, b, a)


def _std_max(a, b):
    return np.where(a < b, b, a)


def box_model(o, d, mn, mx):
    """kdtree.cpp:196-208 (oracle.c ray_box) on float32 arrays."""
    with np.errstate(all="ignore"):
        di = F32(1.0) / d
        t0, t1 = (mn - o) * di, (mx - o) * di
        first = _std_max(_std_max(_std_min(t0[:, 0], t1[:, 0]), _std_min(t0[:, 1], t1[:, 1])),
                         _std_min(t0[:, 2], t1[:, 2]))
        second = _std_min(_std_min(_std_max(t0[:, 0], t1[:, 0]), _std_max(t0[:, 1], t1[:, 1])),
                          _std_max(t0[:, 2], t1[:, 2]))
    return first.astype(F32), second.astype(F32)


UNIT_UV = [(0.0, 0.0), (0.0, 0.5), (0.5, 0.0), (0.5, 0.5), (1.0, 0.0), (0.0, 1.0), (0.25, 0.75), (-0.0, 0.5),
           (0.5, -0.0), (float(np.nextafter(F32(1), F32(2))), 0.0), (0.5, float(np.nextafter(F32(0.5), F32(1)))),
           (-2.0 ** -149, 0.5), (0.5, -2.0 ** -149), (0.75, 0.5), (0.3, 0.3)]
TMAX_EDGE = [1.0, float(np.nextafter(F32(1), F32(2))), float(np.nextafter(F32(1), F32(0))), np.inf, 0.0]


def _tri_lanes(r, big):
    """64 triangle tests: o, d, A, e1, e2, tmax.  big[l]: a lane whose |aa| exceeds 2^100 (rcp_rn_wave's blend
    inside tri_test_wave); the others mix random triangles, exact-aa slivers around FLT_EPSILON, the unit
    triangle hit on its edges and vertices, t == tmax and t == 0."""
    o, d, A, e1, e2 = (np.zeros((64, 3), F32) for _ in range(5))
    tmax = np.zeros(64, F32)
    kind = r.integers(0, 4, 64)
    for l in range(64):
        u, v = UNIT_UV[r.integers(0, len(UNIT_UV))]
        if big[l]:
            # e1 = (s, 0, 0), e2 = (0, 1, 0), d = (0, 0, -1): aa = s exactly, ux = u, uy = v, t = 1
            s = F32(2.0) ** F32(r.integers(101, 120)) * F32(r.choice([-1.0, 1.0]))
            e1[l], e2[l], d[l] = (s, 0, 0), (0, 1, 0), (0, 0, -1)
            o[l] = (s * F32(u), v, 1.0)
            tmax[l] = TMAX_EDGE[r.integers(0, len(TMAX_EDGE))]
        elif kind[l] == 0:  # random triangle, ray aimed at a random (sometimes outside) barycentric point
            A[l], e1[l], e2[l] = r.uniform(-1, 1, 3), r.uniform(-1, 1, 3), r.uniform(-1, 1, 3)
            bu, bv = r.uniform(-0.2, 1.0, 2)
            target = A[l] + F32(bu) * e1[l] + F32(bv) * e2[l]
            o[l] = r.uniform(-3, 3, 3)
            d[l] = (target - o[l]) * F32(r.choice([1.0, 0.5, 4.0]))
            tmax[l] = r.choice([np.inf, 1e30, 0.1, 3.0])
        elif kind[l] == 1:  # sliver: aa = s exactly, on both sides of +-FLT_EPSILON
            s = r.choice([EPS, np.nextafter(EPS, F32(0)), np.nextafter(EPS, F32(1)), EPS * F32(2), EPS / F32(2),
                          F32(0), F32(2.0 ** -110)]) * F32(r.choice([-1.0, 1.0]))
            e1[l], e2[l], d[l] = (s, 0, 0), (0, 1, 0), (0, 0, -1)
            o[l] = (F32(s) * F32(0.25), 0.25, 1.0)
            tmax[l] = np.inf
        elif kind[l] == 2:  # the unit triangle from above: ux = u, uy = v, t = 1 exactly
            e1[l], e2[l], d[l] = (1, 0, 0), (0, 1, 0), (0, 0, -1)
            o[l] = (u, v, 1.0)
            tmax[l] = TMAX_EDGE[r.integers(0, len(TMAX_EDGE))]
        else:  # ... started on the triangle's plane: t == 0
            e1[l], e2[l], d[l] = (1, 0, 0), (0, 1, 0), (0, 0, -1)
            o[l] = (u, v, 0.0)
            tmax[l] = r.choice([np.inf, 0.0, 2.0 ** -149])
    return o, d, A, e1, e2, tmax


def _box_lanes(r, bad):
    """64 root-box slab tests: direction components with zeros, negative zeros, denormals and infinities;
    origins on the box faces, inside and outside.  bad[l]: d.x out of rcp_rn_wave's range."""
    mn = np.tile(np.array([-1.0, -2.0, -0.5], F32), (64, 1)) + r.integers(0, 2, (64, 1)).astype(F32)
    mx = mn + np.array([2.0, 3.5, 1.25], F32)
    special = np.concatenate([f32([0, 0x80000000, 1, 0x80000001, 0x7F800000, 0xFF800000, 0x007FFFFF]),
                              np.array([1.0, -1.0, 0.5, 2.0 ** -100, -2.0 ** 100, 3.0], F32)])
    d = _rand_f32(r, 64 * 3, -6, 3).reshape(64, 3)
    pick = r.random((64, 3)) < 0.4
    d[pick] = special[r.integers(0, len(special), pick.sum())]
    good = _rand_f32(r, 64, -6, 3)
    d[:, 0] = np.where(bad, _rcp_out_of_range(r, 64), np.where(rcp_in_range(d[:, 0]), d[:, 0], good))
    for ax in (1, 2):  # (the other components stay in range: the x component alone decides the lane mix)
        d[:, ax] = np.where(rcp_in_range(d[:, ax]) | (r.random(64) < 0.5), d[:, ax], good)
    o = r.uniform(-3, 3, (64, 3)).astype(F32)
    face = r.random((64, 3))
    o = np.where(face < 0.25, mn, np.where(face < 0.5, mx, o)).astype(F32)
    return o, d.astype(F32), mn.astype(F32), mx.astype(F32)


@functools.lru_cache(maxsize=None)
def wave_cases():
    """Returns (lanes [g][64][32], masks [g] uint64, expected [g][64][16], facts).  Per lane pattern (how many
    lanes fail the helpers' range tests, and where), active mask and repeat one group; the same lanes fail
    rcp_rn_wave's test (a, the triangle's aa, the box ray's d.x) and div_by_rcp_wave's."""
    r = np.random.default_rng(0x3A7E)
    lanes, masks, exp, facts = [], [], [], []
    for rep in range(WAVE_REPEATS):
        for pname, pos in LANE_PATTERNS:
            for mname, mask in MASKS.items():
                if pos is None:
                    bad = np.zeros(64, bool)
                    bad[r.permutation(64)[:int(pname)]] = True
                else:
                    bad = np.isin(np.arange(64), pos)
                if mask is None:  # one lane: a failing one on even repeats where there is one, else any
                    cand = np.flatnonzero(bad) if (rep % 2 == 0 and bad.any()) else np.arange(64)
                    mask = 1 << int(cand[r.integers(0, len(cand))])
                a = np.where(bad, _rcp_out_of_range(r, 64), _rand_f32(r, 64, -100, 99))
                edge = r.random(64) < 0.1
                a = np.where(~bad & edge, F32(2.0) ** F32(r.choice([-100, 100])), a).astype(F32)
                # divisions: in range b in [2^-40, 2^40] and the quotient in [2^-55, 2^55]; the failing lanes
                # take b out of its range, or a quotient that is zero, huge, tiny, infinite or NaN
                db = _rand_f32(r, 64, -40, 39)
                da = (db * _rand_f32(r, 64, -55, 55)).astype(F32)
                bad_b = _rcp_out_of_range(r, 64)
                bad_b = np.where(np.abs(bad_b) == F32(2.0 ** -101), F32(2.0 ** -41), bad_b)
                way = r.integers(0, 2, 64)
                bad_a = np.array([0.0, -0.0, np.inf, np.nan, 2.0 ** 100, 2.0 ** -110, 2.0 ** -149], F32)[
                    r.integers(0, 7, 64)]
                db = np.where(bad & (way == 0), bad_b, db).astype(F32)
                da = np.where(bad & (way != 0), bad_a, da).astype(F32)
                to, td, tA, te1, te2, tmax = _tri_lanes(r, bad)
                live = (r.random(64) < 0.8).astype(U32)
                bo, bd, mn, mx = _box_lanes(r, bad)
                rec = np.concatenate([bits(a)[:, None], bits(da)[:, None], bits(db)[:, None], bits(to), bits(td),
                                      bits(tA), bits(te1), bits(te2), bits(tmax)[:, None], live[:, None], bits(bo),
                                      bits(bd), bits(mn), bits(mx)], 1)
                assert rec.shape == (64, 32)
                with np.errstate(all="ignore"):
                    rcp = (F32(1.0) / a).astype(F32)
                    quo = (da / db).astype(F32)
                ok, ux, uy, t, aa = tri_model(to, td, tA, te1, te2, tmax)
                first, second = box_model(bo, bd, mn, mx)
                e = np.zeros((64, 16), U32)
                e[:, 0] = e[:, 1] = bits(rcp)
                e[:, 2] = e[:, 3] = bits(quo)
                e[:, 4], e[:, 8] = ok & (live != 0), ok
                e[:, 5], e[:, 6], e[:, 7] = bits(ux), bits(uy), bits(t)
                e[:, 9], e[:, 10], e[:, 11] = bits(ux), bits(uy), bits(t)
                e[:, 12] = e[:, 14] = bits(first)
                e[:, 13] = e[:, 15] = bits(second)
                lanes.append(rec), masks.append(mask), exp.append(e)
                act = np.array([(mask >> l) & 1 for l in range(64)], bool)
                facts.append({"pattern": pname, "mask": mname, "active": int(act.sum()),
                              "rcp_fail": int((~rcp_in_range(a)).sum()), "div_fail": int((~div_in_range(da, db)).sum()),
                              "tri_fail": int((~rcp_in_range(aa)).sum()),
                              "tri_big": int((np.abs(aa) > F32(2.0 ** 100)).sum()),
                              "box_fail": int((~rcp_in_range(bd[:, 0])).sum()),
                              "rcp_fail_active": int((~rcp_in_range(a) & act).sum()),
                              "div_fail_active": int((~div_in_range(da, db) & act).sum()),
                              "tri_accept": int((ok & (live != 0)).sum()),
                              "tri_big_accept": int((ok & (live != 0) & (np.abs(aa) > F32(2.0 ** 100))).sum()),
                              "edge_hits": int((ok & ((ux == 0) | (uy == 0) | (ux + uy == 1))).sum()),
                              "t_zero": int((ok & (t == 0)).sum()), "t_at_tmax": int((t == tmax).sum()),
                              "aa_near_eps": int(((np.abs(aa) >= EPS / 2) & (np.abs(aa) <= EPS * 2)).sum())})
    return np.array(lanes, U32), np.array(masks, np.uint64), np.array(exp, U32), facts


def wave_input_words(lanes, masks):
    m = np.stack([masks & np.uint64(M32), masks >> np.uint64(32)], 1).astype(U32)
    return np.concatenate([lanes.reshape(-1), m.reshape(-1)])


def wave_expected_runs(masks, exp):
    """[2][g][64][16]: run 0 whole wave, run 1 the mask's lanes (the others hold the sentinel)."""
    act = ((masks[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    return np.stack([exp, np.where(act[:, :, None], exp, U32(SENTINEL))])


# Which of the 16 output words of a lane are compared when tri_test_wave (words 4..7) / tri_test (8..11) rejects:
# ux, uy, t of a rejecting lane are unspecified.
def wave_compare_mask(exp_runs):
    keep = np.ones(exp_runs.shape, bool)
    sentinel = (exp_runs == U32(SENTINEL)).all(-1)
    for flag in (4, 8):
        rej = (exp_runs[..., flag] == 0) & ~sentinel
        keep[..., flag + 1:flag + 4] &= ~rej[..., None]
    return keep


# ------------------------------------------------------------ texture --
def texture_cases():
    """The four textures and 4 x 144 (u, v) -> rgb vectors of tests/golden/ref_texture.json (the reference's own
    Texture::getColorAt), as one atlas of four textures; then NaN coordinates, which have no expected value.
    Returns (input words, texture list [(w, h, nc, bytes)], cases [n][3], expected rgb [n_ref][3], n_ref)."""
    data = json.loads((ROOT / "tests" / "golden" / "ref_texture.json").read_text())
    words, texs, cases, exp = [], [], [], []
    for ti, t in enumerate(data["textures"]):
        w, h, nc, salt = t["w"], t["h"], t["nc"], t["salt"]
        i = np.arange(w * h * nc, dtype=np.uint64)
        img = ((i * 2654435761 + salt) >> np.uint64(7)).astype(np.uint8)  # tests/test_oracle_golden.py
        texs.append((w, h, nc, img))
        for c in t["cases"]:
            cases.append([ti, c["u"], c["v"]])
            exp.append(c["rgb"])
    n_ref = len(cases)
    half = b1(0.5)
    for ti in range(len(texs)):
        cases += [[ti, NAN, half], [ti, half, NAN], [ti, NAN, NAN], [ti, 0xFFC00000, half]]
    words = [len(texs), len(cases)]
    for w, h, nc, img in texs:
        padded = np.zeros((len(img) + 3) // 4 * 4, np.uint8)
        padded[:len(img)] = img
        words += [w, h, nc] + padded.view(U32).tolist()
    cases = np.array(cases, U32)
    return np.concatenate([np.array(words, U32), cases.reshape(-1)]), texs, cases, np.array(exp, U32), n_ref
