"""The numpy float32 statement of the SH irradiance probes (include/chiaro_hip.h "probes"): the sphere
direction, the L2 basis, the projection's fold and blend, the evaluation and the grid lookup.  Every step is one
correctly rounded float32 operation in the order the header gives, the two marked double in float64; csrc/probe.hpp is
the C++ statement and tests/test_probe_model.py compares the two bit for bit.  The sine and cosine are libm's sinf and
cosf, called through ctypes (numpy's own float32 sine is another function)."""
import ctypes as C
import ctypes.util

import numpy as np

F32 = np.float32
K0, K1, K2, K3, K4 = F32(0.28209479), F32(0.48860251), F32(1.0925484), F32(0.31539157), F32(0.54627422)
BAND = np.array([1.0] + [2.0 / 3.0] * 3 + [0.25] * 5, np.float64).astype(F32)  # A_l / pi per coefficient
FOURPI = F32(12.566371)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.sinf, _libm.cosf):
    _f.restype, _f.argtypes = C.c_float, [C.c_float]


def sincos(phi):
    phi = np.ascontiguousarray(phi, F32)
    sn = np.array([_libm.sinf(float(v)) for v in phi.ravel()], F32).reshape(phi.shape)
    cs = np.array([_libm.cosf(float(v)) for v in phi.ravel()], F32).reshape(phi.shape)
    return sn, cs


def max0(v):
    return np.where(v > F32(0), v, F32(0)).astype(F32)


def uniform(raw):
    """rng_uniform(rng, 0, 1) of raw 32-bit draws."""
    c = np.asarray(raw, np.uint32).astype(F32) / F32(4294967296.0)
    c = np.where(c >= F32(1), F32(float.fromhex("0x1.fffffep-1")), c).astype(F32)
    return (c * (F32(1) - F32(0)) + F32(0)).astype(F32)


def direction_u(u0, u1):
    """[..., 3] from the two uniforms."""
    u0, u1 = np.asarray(u0, F32), np.asarray(u1, F32)
    z = (u0 * F32(2) + F32(-1)).astype(F32)
    r = np.sqrt(max0(F32(1) - z * z)).astype(F32)
    phi = (u1.astype(np.float64) * 6.283185307179586).astype(F32)
    sn, cs = sincos(phi)
    return np.stack([r * cs, r * sn, z], axis=-1).astype(F32)


def direction(raw0, raw1):
    return direction_u(uniform(raw0), uniform(raw1))


def basis(d):
    """[..., 9] of directions [..., 3] (used as given)."""
    d = np.asarray(d, F32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    Y = [np.full(x.shape, K0, F32), K1 * y, K1 * z, K1 * x, K2 * (x * y), K2 * (y * z),
         K3 * (F32(3) * (z * z) - F32(1)), K2 * (x * z), K4 * (x * x - y * y)]
    return np.stack(Y, axis=-1).astype(F32)


def fold(dirs, rad, first_layer=1, sh=None, m2=None):
    """dirs, rad [layers][n][spp][3] -> (sh, m2) [n][9][3] after the last layer, blended onto sh / m2 (zeros)."""
    dirs, rad = np.asarray(dirs, F32), np.asarray(rad, F32)
    nl, n, spp, _ = rad.shape
    sh = np.zeros((n, 9, 3), F32) if sh is None else np.array(sh, F32).reshape(n, 9, 3)
    m2 = np.zeros((n, 9, 3), F32) if m2 is None else np.array(m2, F32).reshape(n, 9, 3)
    inv = F32(1) / F32(spp)
    for j in range(nl):
        L = first_layer + j
        t, q = np.zeros((n, 9, 3), F32), np.zeros((n, 9, 3), F32)
        Y = basis(dirs[j])  # [n][spp][9]
        for s in range(spp):
            p = (Y[:, s, :, None] * rad[j, :, s, None, :]).astype(F32)
            t = t + p
            q = q + p * p
        old, old2 = (sh, m2) if L > 1 else (np.zeros_like(sh), np.zeros_like(m2))
        sh = ((old * F32(L - 1) + t * inv) / F32(L)).astype(F32)
        m2 = ((old2 * F32(L - 1) + q * inv) / F32(L)).astype(F32)
    return sh, m2


def evaluate(sh, nrm):
    """sh [m][9][3], nrm [m][3] -> [m][3]: the mean incoming radiance under the cosine density about nrm."""
    sh, Y = np.asarray(sh, F32).reshape(-1, 9, 3), basis(nrm)
    e = np.zeros((len(sh), 3), F32)
    for k in range(9):
        w = (BAND[k] * Y[:, k]).astype(F32)
        e = e + w[:, None] * sh[:, k, :]
    return max0(FOURPI * e)


def grid_positions(origin, step, dims):
    origin, step = np.asarray(origin, F32), np.asarray(step, F32)
    nx, ny, nz = (int(v) for v in dims)
    out = np.zeros((nz, ny, nx, 3), F32)
    out[..., 0] = (origin[0] + np.arange(nx, dtype=np.uint32).astype(F32) * step[0])[None, None, :]
    out[..., 1] = (origin[1] + np.arange(ny, dtype=np.uint32).astype(F32) * step[1])[None, :, None]
    out[..., 2] = (origin[2] + np.arange(nz, dtype=np.uint32).astype(F32) * step[2])[:, None, None]
    return out.reshape(-1, 3)


def axis(p, origin, step, dim, clamp=True):
    """(i0, i1, t) of coordinates p on one axis."""
    p = np.asarray(p, F32)
    if dim == 1:
        z = np.zeros(p.shape, np.int64)
        return z, z, np.zeros(p.shape, F32)
    f = ((p - F32(origin)) / F32(step)).astype(F32)
    if clamp:
        hi = F32(dim - 1)
        f = np.where(f > F32(0), f, F32(0)).astype(F32)
        f = np.where(f < hi, f, hi).astype(F32)
    i0 = np.minimum(f.astype(np.int64), dim - 2)
    t = (f - i0.astype(F32)).astype(F32)
    return i0, i0 + 1, t


def lookup(origin, step, dims, sh, pos, nrm):
    """The grid lookup: sh [count][9][3] -> [m][3]."""
    sh, pos = np.asarray(sh, F32).reshape(-1, 9, 3), np.asarray(pos, F32).reshape(-1, 3)
    ax = [axis(pos[:, a], origin[a], step[a], int(dims[a])) for a in range(3)]
    coef = np.zeros((len(pos), 9, 3), F32)
    for uz in (0, 1):
        for uy in (0, 1):
            for ux in (0, 1):
                w = []
                for a, u in ((0, ux), (1, uy), (2, uz)):
                    t = ax[a][2]
                    w.append(t if u else (F32(1) - t).astype(F32))
                wt = ((w[0] * w[1]) * w[2]).astype(F32)
                ix, iy, iz = ax[0][ux], ax[1][uy], ax[2][uz]
                idx = (iz * int(dims[1]) + iy) * int(dims[0]) + ix
                coef = coef + wt[:, None, None] * sh[idx]
    return evaluate(coef, nrm)
