"""The texture-space side of a lightmap bake restated in numpy float32 (include/chiaro_hip.h "lightmap baking",
DESIGN.md §3.29): coverage, owner, surface point, covered list, dilation and the grid atlas.  This file is the
definition's second statement, as denoise_model.py is the filter's: csrc/bake.hpp's host functions and the kernels of
csrc/texbake.hip are compared against it bit for bit.  Every operation is a float32 operation in the order the header
writes it; nothing here is fused or reassociated."""
import math

import numpy as np

F32 = np.float32
NONE = 0xFFFFFFFF
# the neighbours of a dilation pass, (dx, dy), in the order their values are summed
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))


def edge(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _weights(uv, W, H, inclusive=True):
    """(ys, xs, covered, w1, w2, A) of one triangle's six UVs over the W x H map: the rows and columns whose centres lie
    in the triangle's bounding box (part of the definition: exact, inclusive comparisons), and over that sub-grid the
    covered mask and the weights of q1 and q2, all negated for A < 0.  None when the triangle covers nothing."""
    uv = np.asarray(uv, F32)
    if not np.isfinite(uv).all():
        return None
    fW, fH = F32(W), F32(H)
    qx, qy = uv[0::2] * fW, uv[1::2] * fH
    A = edge(qx[0], qy[0], qx[1], qy[1], qx[2], qy[2])
    if A == 0:
        return None
    cx = np.arange(W, dtype=F32) + F32(0.5)
    cy = np.arange(H, dtype=F32) + F32(0.5)
    xs = np.flatnonzero((cx >= qx.min()) & (cx <= qx.max()))
    ys = np.flatnonzero((cy >= qy.min()) & (cy <= qy.max()))
    if not len(xs) or not len(ys):
        return None
    cx, cy = cx[xs][None, :], cy[ys][:, None]
    w0 = edge(qx[1], qy[1], qx[2], qy[2], cx, cy)
    w1 = edge(qx[2], qy[2], qx[0], qy[0], cx, cy)
    w2 = edge(qx[0], qy[0], qx[1], qy[1], cx, cy)
    if A < 0:
        w0, w1, w2, A = -w0, -w1, -w2, -A
    ge = (lambda w: w >= 0) if inclusive else (lambda w: w > 0)
    return ys, xs, ge(w0) & ge(w1) & ge(w2), w1.astype(F32), w2.astype(F32), F32(A)


def coverage(uv, W, H, inclusive=True):
    """[n_tris][H][W] bool: the texels each triangle covers."""
    uv = np.asarray(uv, F32).reshape(-1, 6)
    out = np.zeros((len(uv), H, W), bool)
    with np.errstate(all="ignore"):
        for t in range(len(uv)):
            r = _weights(uv[t], W, H, inclusive)
            if r is not None:
                out[t][np.ix_(r[0], r[1])] = r[2]
    return out


def surface(uv, tri_pos, tri_normal, W, H, offset=0.001, inclusive=True):
    """owner uint32 [H][W], pos, nrm float32 [H][W][3], list uint32 [count] (the owned texel indices ascending)."""
    uv = np.asarray(uv, F32).reshape(-1, 6)
    tri_pos = np.asarray(tri_pos, F32).reshape(-1, 3, 3)
    tri_normal = np.asarray(tri_normal, F32).reshape(-1, 3)
    owner = np.full((H, W), NONE, np.uint32)
    pos, nrm = np.zeros((H, W, 3), F32), np.zeros((H, W, 3), F32)
    off = F32(offset)
    with np.errstate(all="ignore"):
        for t in range(len(uv)):  # ascending: the first triangle to cover a texel is the lowest id
            r = _weights(uv[t], W, H, inclusive)
            if r is None:
                continue
            ys, xs, c, w1, w2, A = r
            box = np.ix_(ys, xs)
            mine = c & (owner[box] == NONE)
            if not mine.any():
                continue
            yy, xx = np.broadcast_to(ys[:, None], mine.shape)[mine], np.broadcast_to(xs[None, :], mine.shape)[mine]
            owner[yy, xx] = t
            b1, b2 = (w1[mine] / A)[:, None], (w2[mine] / A)[:, None]
            b0 = F32(1.0) - b1 - b2
            p = tri_pos[t]
            P = (p[0][None, :] * b0 + p[1][None, :] * b1) + p[2][None, :] * b2
            n = np.broadcast_to(tri_normal[t] + F32(0.0), P.shape).astype(F32)
            nrm[yy, xx] = n
            pos[yy, xx] = P + off * n
    return owner, pos.astype(F32), nrm.astype(F32), np.flatnonzero(owner.reshape(-1) != NONE).astype(np.uint32)


def dilate(owner, values, passes):
    """`passes` dilation passes of values [H][W][3] under the owner map."""
    owner = np.asarray(owner, np.uint32)
    H, W = owner.shape
    out = np.array(values, F32).reshape(H, W, 3)
    filled = owner != NONE
    with np.errstate(all="ignore"):
        for _ in range(min(int(passes), max(W, H))):
            s = np.zeros((H, W, 3), F32)
            cnt = np.zeros((H, W), np.uint32)
            for dx, dy in NEIGHBOURS:
                # the neighbour (x + dx, y + dy) of every texel, where it is inside the map and filled
                v = np.zeros((H, W, 3), F32)
                f = np.zeros((H, W), bool)
                ys, yd = (slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0)))
                xs, xd = (slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0)))
                v[yd, xd] = out[ys, xs]
                f[yd, xd] = filled[ys, xs]
                s = np.where(f[..., None], s + v, s)
                cnt += f
            new = ~filled & (cnt > 0)
            mean = s / cnt.astype(F32)[..., None]
            out = np.where(new[..., None], mean, out).astype(F32)
            filled = filled | new
    return out


def atlas_grid(n_tris, cell, gutter=0.25):
    """(W, H, uv float32 [n_tris][6]) of the grid atlas."""
    cols = math.isqrt(n_tris - 1) + 1 if n_tris > 1 else 1
    rows = (n_tris + cols - 1) // cols
    W, H = cols * cell, rows * cell
    fw, fh, lo, hi = F32(W), F32(H), F32(gutter), F32(cell) - F32(gutter)
    uv = np.zeros((n_tris, 6), F32)
    for t in range(n_tris):
        cx, cy = F32((t % cols) * cell), F32((t // cols) * cell)
        uv[t] = [(cx + lo) / fw, (cy + lo) / fh, (cx + hi) / fw, (cy + lo) / fh, (cx + lo) / fw, (cy + hi) / fh]
    return W, H, uv
