"""The guide buffers and the a-trous filter of include/chiaro_hip.h "guide buffers and denoiser", restated in numpy
float32 -- the definition the GPU kernels (csrc/denoise.hip) are compared with bit for bit.

Every operation is a float32 numpy operation on float32 operands, in the order the header writes it; nothing is
promoted to float64 and nothing is reassociated.  The oracle supplies what the header takes from the render:
or_intersect (the hits), or_tex_lookup (textured albedo); the material normal and its normalisation are restated
here and pinned against or_material_normal / or_glm_normalize by tests/test_denoise_model.py.
"""
import numpy as np

F32 = np.float32
DEFAULTS = dict(levels=4, sigma_l=4.0, sigma_z=0.1, sigma_a=0.1, normal_squarings=5)
G = (F32(0.25), F32(0.5), F32(0.25))
H = (F32(0.0625), F32(0.25), F32(0.375), F32(0.25), F32(0.0625))


# --- guides --------------------------------------------------------------------------------------------------

def guide_rays(cam, x, y):
    """(orig, dir) [y*x][3]: eye, and (left_upper + dx * sx) + dy * sy at the pixel centres."""
    cam = np.asarray(cam, F32)
    eye, lu, dx, dy = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    sx = (np.arange(x, dtype=np.uint32).astype(F32) + F32(0.5))[None, :, None]
    sy = (np.arange(y, dtype=np.uint32).astype(F32) + F32(0.5))[:, None, None]
    d = (lu[None, None, :] + dx[None, None, :] * sx) + dy[None, None, :] * sy
    o = np.broadcast_to(eye, (y, x, 3))
    return np.ascontiguousarray(o, F32).reshape(-1, 3), np.ascontiguousarray(d, F32).reshape(-1, 3)


def material_normal(vnrm):
    """[n][9] vertex normals -> Material::normal ((n0 + n1) + n2) / 3."""
    v = np.asarray(vnrm, F32).reshape(-1, 3, 3)
    return ((v[:, 0] + v[:, 1]) + v[:, 2]) / F32(3)


def normalize(v):
    """glm::normalize: v * (1 / sqrt((x * x + y * y) + z * z))."""
    with np.errstate(all="ignore"):
        v = np.asarray(v, F32)
        d = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        return v * (F32(1) / np.sqrt(d))[..., None]


def guides_ref(oracle, tris, cam, x, y):
    """{"albedo", "normal" [y][x][3], "depth" [y][x], "hit", "textured" [y][x] bool} of the header's definition."""
    o, d = guide_rays(cam, x, y)
    h = oracle.intersect(o, d)
    hit = h["hit"].astype(bool)
    n = x * y
    albedo, normal, depth = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.full(n, F32(-1))
    textured = np.zeros(n, bool)
    t = h["tri"][hit]
    kd = np.asarray(tris["kd"], F32)[t].copy()
    tex = np.asarray(tris["tex"], np.int32)[t]
    uv = np.asarray(tris["uv"], F32)[t]
    bx, by = h["bary"][hit, 0], h["bary"][hit, 1]
    bz = (F32(1) - bx) - by
    u = (uv[:, 0] * bz + uv[:, 2] * bx) + uv[:, 4] * by
    v = (uv[:, 1] * bz + uv[:, 3] * bx) + uv[:, 5] * by
    for i in np.flatnonzero(tex >= 0):
        kd[i] = oracle.tex_lookup(int(tex[i]), u[i], v[i])
    albedo[hit] = kd
    normal[hit] = normalize(material_normal(np.asarray(tris["vnrm"], F32)[t]))
    depth[hit] = h["dist"][hit]
    textured[np.flatnonzero(hit)[tex >= 0]] = True
    return {"albedo": albedo.reshape(y, x, 3), "normal": normal.reshape(y, x, 3), "depth": depth.reshape(y, x),
            "hit": hit.reshape(y, x), "textured": textured.reshape(y, x)}


# --- the filter ----------------------------------------------------------------------------------------------

def initial_variance(frame, m2, layers, spp, layer_map=None):
    """The variance of each pixel's mean [y][x]."""
    with np.errstate(all="ignore"):
        c, q = np.asarray(frame, F32), np.asarray(m2, F32)
        if layer_map is None:
            n = F32(np.uint32((int(layers) * int(spp)) & 0xFFFFFFFF))
        else:
            n = (np.asarray(layer_map, np.uint32) * np.uint32(spp)).astype(F32)[..., None]
        v = q - c * c
        v = np.where(v > 0, v, F32(0)).astype(F32)
        v = v / n
        return ((v[..., 0] + v[..., 1]) + v[..., 2]).astype(F32)


def _shift(a, dx, dy):
    """(b, inside): b[y, x] = a[y + dy, x + dx] where that lies in the frame (else 0, inside False)."""
    yres, xres = a.shape[:2]
    b = np.zeros_like(a)
    inside = np.zeros((yres, xres), bool)
    y0, y1 = max(0, -dy), min(yres, yres - dy)
    x0, x1 = max(0, -dx), min(xres, xres - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        inside[y0:y1, x0:x1] = True
    return b, inside


def atrous_level(C, var, A, N, Z, step, sigma_l, sigma_z, sigma_a, squarings):
    """One level: (C', var')."""
    yres, xres = var.shape
    s = int(step)
    sl2 = F32(sigma_l) * F32(sigma_l)
    sz_step = F32(sigma_z) * F32(s)
    inv_sa2 = F32(1) / (F32(sigma_a) * F32(sigma_a))
    one = F32(1)
    with np.errstate(all="ignore"):
        ys, xs = np.arange(yres), np.arange(xres)
        vb = np.zeros((yres, xres), F32)
        for j in range(3):
            for i in range(3):
                qy, qx = np.clip(ys + j - 1, 0, yres - 1), np.clip(xs + i - 1, 0, xres - 1)
                vb = vb + (G[j] * G[i]) * var[qy][:, qx]
        den = sl2 * vb + F32(1e-8)
        bp = (C[..., 0] + C[..., 1]) + C[..., 2]
        hp = Z >= 0
        sw = np.zeros((yres, xres), F32)
        sc = np.zeros((yres, xres, 3), F32)
        sv = np.zeros((yres, xres), F32)
        for j in range(5):
            for i in range(5):
                w0 = H[j] * H[i]
                dx, dy = s * (i - 2), s * (j - 2)
                Cq, inside = _shift(C, dx, dy)
                vq, _ = _shift(var, dx, dy)
                if i == 2 and j == 2:
                    w = np.full((yres, xres), w0, F32)
                    use = inside
                else:
                    Aq, _ = _shift(A, dx, dy)
                    Nq, _ = _shift(N, dx, dy)
                    Zq, _ = _shift(Z, dx, dy)
                    bq = (Cq[..., 0] + Cq[..., 1]) + Cq[..., 2]
                    dl = bq - bp
                    t = one / (one + (dl * dl) / den)
                    w = w0 * (t * t)
                    da = Aq - A
                    d2 = ((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]) * inv_sa2
                    t = one / (one + d2)
                    w = w * (t * t)
                    hq = Zq >= 0
                    dn = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                    dn = np.where(dn > 0, dn, F32(0)).astype(F32)
                    for _ in range(int(squarings)):
                        dn = dn * dn
                    zm = np.where(Z > Zq, Z, Zq)
                    dz = (Zq - Z) / (sz_step * zm)
                    t = one / (one + dz * dz)
                    w = np.where(hp & hq, w * (dn * (t * t)), w).astype(F32)
                    use = inside & (hp == hq) & (w > 0)
                sw = np.where(use, sw + w, sw)
                sc = np.where(use[..., None], sc + w[..., None] * Cq, sc)
                sv = np.where(use, sv + (w * w) * vq, sv)
        return (sc / sw[..., None]).astype(F32), (sv / (sw * sw)).astype(F32)


def denoise_ref(frame, m2, layers, spp, albedo, normal, depth, layer_map=None, levels=4, sigma_l=4.0, sigma_z=0.1,
                sigma_a=0.1, normal_squarings=5):
    """(denoised frame [y][x][3], its variance [y][x]) of the header's definition."""
    C = np.ascontiguousarray(frame, F32).copy()
    var = initial_variance(frame, m2, layers, spp, layer_map)
    A, N, Z = (np.ascontiguousarray(a, F32) for a in (albedo, normal, depth))
    for it in range(int(levels)):
        C, var = atrous_level(C, var, A, N, Z, 1 << it, sigma_l, sigma_z, sigma_a, normal_squarings)
    return C, var


def canon(a):
    """a with every NaN replaced by one quiet NaN: a NaN's sign and payload are not part of the definition (an
    invalid operation yields another default NaN on x86 than on the GPU); that a value is a NaN is."""
    a = np.ascontiguousarray(a, F32).copy()
    a[np.isnan(a)] = F32(np.nan)
    return a
