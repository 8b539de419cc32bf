"""Temporal reprojection of include/chiaro_hip.h "temporal reprojection", restated in numpy float32 -- the definition
the GPU kernel (csrc/temporal.hip) is compared with bit for bit.

Every operation is a float32 numpy operation on float32 operands, in the order the header writes it; nothing is
promoted to float64 and nothing is reassociated.  Cameras are the 12 floats eye, left_upper, dx, dy."""
import numpy as np

from denoise_model import canon  # noqa: F401  (NaNs are compared through it)

F32 = np.float32
U32 = np.uint32
DEFAULTS = dict(depth_tol=0.05, normal_min=0.9, max_history=65536)


def cross(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F32)


def dot(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def projector(cam_prev):
    """(ra, rb, rc, det) of the previous camera, or None when det is 0 or not finite (CR_E_INVALID)."""
    with np.errstate(all="ignore"):
        cam = np.asarray(cam_prev, F32)
        lu, dx, dy = cam[3:6], cam[6:9], cam[9:12]
        ra, rb, rc = cross(dx, dy), cross(dy, lu), cross(lu, dx)
        det = F32(dot(lu, ra))
    if not np.isfinite(det) or det == 0:
        return None
    return ra, rb, rc, det


def sample_counts(yres, xres, layers, spp, layer_map=None):
    """n_u [y][x] uint32: layers * spp, with a layer map map * spp, wrapping."""
    if layer_map is None:
        return np.full((yres, xres), (int(layers) * int(spp)) & 0xFFFFFFFF, U32)
    return ((np.asarray(layer_map, np.uint64) * np.uint64(spp)) & np.uint64(0xFFFFFFFF)).astype(U32)


def reproject_ref(cam_cur, cam_prev, frame, m2, layers, spp, normal, depth, hist_frame, hist_m2, hist_count,
                  hist_normal, hist_depth, layer_map=None, depth_tol=0.05, normal_min=0.9, max_history=65536):
    """(out [y][x][3], m2_out [y][x][3], count_out [y][x] uint32, h [y][x] uint32 -- the history count each pixel
    found, 0: none) of the header's definition."""
    C, M, Nc, Zc = (np.ascontiguousarray(a, F32) for a in (frame, m2, normal, depth))
    H, H2, Np, Zp = (np.ascontiguousarray(a, F32) for a in (hist_frame, hist_m2, hist_normal, hist_depth))
    K = np.ascontiguousarray(hist_count, U32)
    yres, xres = Zc.shape
    cur, prev = np.asarray(cam_cur, F32), np.asarray(cam_prev, F32)
    eye_c, lu_c, dx_c, dy_c = cur[0:3], cur[3:6], cur[6:9], cur[9:12]
    eye_p = prev[0:3]
    ra, rb, rc, det = projector(prev)
    n_u = sample_counts(yres, xres, layers, spp, layer_map)
    tol, nmin = F32(depth_tol), F32(normal_min)
    half, one = F32(0.5), F32(1)
    with np.errstate(all="ignore"):
        sx = (np.arange(xres, dtype=U32).astype(F32) + half)[None, :, None]
        sy = (np.arange(yres, dtype=U32).astype(F32) + half)[:, None, None]
        d = (lu_c[None, None, :] + dx_c[None, None, :] * sx) + dy_c[None, None, :] * sy
        P = eye_c[None, None, :] + d * Zc[..., None]
        q = P - eye_p[None, None, :]
        a, b, c = dot(q, ra), dot(q, rb), dot(q, rc)
        u, v = b / a, c / a
        ze = a / det
        live = (Zc >= 0) & (ze > 0)
        fx, fy = u - half, v - half
        x0, y0 = np.floor(fx), np.floor(fy)
        wx, wy = fx - x0, fy - y0
        omx, omy = one - wx, one - wy
        ztol = tol * ze
        sw = np.zeros((yres, xres), F32)
        sr = np.zeros((yres, xres, 3), F32)
        s2 = np.zeros((yres, xres, 3), F32)
        kmin = np.full((yres, xres), 0xFFFFFFFF, U32)
        taps = np.zeros((yres, xres), bool)
        for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)):
            tx, ty = x0 + F32(i), y0 + F32(j)
            w = (wx if i else omx) * (wy if j else omy)
            inside = live & (tx >= 0) & (tx < F32(xres)) & (ty >= 0) & (ty < F32(yres))
            qx = np.where(inside, tx, F32(0)).astype(np.int64)
            qy = np.where(inside, ty, F32(0)).astype(np.int64)
            Hq, H2q, Kq, Npq, Zpq = H[qy, qx], H2[qy, qx], K[qy, qx], Np[qy, qx], Zp[qy, qx]
            use = inside & (Kq > 0) & (Zpq >= 0) & (np.abs(Zpq - ze) <= ztol) & (dot(Nc, Npq) >= nmin)
            use &= ~(np.isnan(Hq).any(axis=-1) | np.isnan(H2q).any(axis=-1)) & (w > 0)
            sw = np.where(use, sw + w, sw)
            sr = np.where(use[..., None], sr + w[..., None] * Hq, sr)
            s2 = np.where(use[..., None], s2 + w[..., None] * H2q, s2)
            kmin = np.where(use, np.minimum(kmin, Kq), kmin)
            taps |= use
        R, R2 = sr / sw[..., None], s2 / sw[..., None]
        h = np.where(taps, np.minimum(kmin, U32(max_history)), U32(0)).astype(U32)
        hf, nf = h.astype(F32), n_u.astype(F32)
        tot = hf + nf
        mo = (R * hf[..., None] + C * nf[..., None]) / tot[..., None]
        mo2 = (R2 * hf[..., None] + M * nf[..., None]) / tot[..., None]
        mc = np.minimum(h.astype(np.uint64) + n_u.astype(np.uint64), np.uint64(0xFFFFFFFF)).astype(U32)
    cur_only, hist_only, none = (h == 0) & (n_u > 0), (h > 0) & (n_u == 0), (h == 0) & (n_u == 0)
    zero3 = np.zeros_like(C)

    def pick(merged, current, history):
        o = np.where(cur_only[..., None], current, merged)
        o = np.where(hist_only[..., None], history, o)
        return np.where(none[..., None], zero3, o).astype(F32)

    out, m2_out = pick(mo, C, R), pick(mo2, M, R2)
    count = np.where(cur_only, n_u, np.where(hist_only, h, np.where(none, U32(0), mc))).astype(U32)
    return out, m2_out, count, h


class History:
    """cr_render_temporal's state: the chain of reproject_ref over successive frames."""

    def __init__(self, **params):
        self.params = dict(DEFAULTS, **params)
        self.reset()

    def reset(self):
        self.cam = None

    def step(self, cam, frame, m2, nlayers, spp, normal, depth):
        """The merged (frame, m2, count, h) for the frame of `nlayers * spp` samples at cam; becomes the history."""
        frame, m2 = np.ascontiguousarray(frame, F32), np.ascontiguousarray(m2, F32)
        normal, depth = np.ascontiguousarray(normal, F32), np.ascontiguousarray(depth, F32)
        if self.cam is None or self.frame.shape != frame.shape:
            out, m2_out = frame.copy(), m2.copy()
            count = sample_counts(depth.shape[0], depth.shape[1], nlayers, spp)
            h = np.zeros(depth.shape, U32)
        else:
            out, m2_out, count, h = reproject_ref(cam, self.cam, frame, m2, nlayers, spp, normal, depth, self.frame,
                                                  self.m2, self.count, self.normal, self.depth, **self.params)
        self.cam = np.asarray(cam, F32).copy()
        self.frame, self.m2, self.count, self.normal, self.depth = out, m2_out, count, normal, depth
        return out, m2_out, count, h
