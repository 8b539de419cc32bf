"""Inputs shared by the temporal-reprojection tests (tests/test_temporal_model.py on the CPU, tests/test_gpu_temporal.py
on the GPU): the camera path through the cornell box, the oracle's frame and moment frame at a camera, the chain of
tests/temporal_model.py over them, and the crafted inputs of cr_reproject_device.  Computed once per key and shared;
nothing here changes them."""
import ctypes as C

import numpy as np

import denoise_model as dm
import temporal_model as tm

F32 = np.float32
U32 = np.uint32
SEED, K = 0xC41A05C0, 6
# cr_render_temporal's chain: cornell at 24x18, 1 layer x 2 spp, three cameras
CX, CY, CSPP = 24, 18, 2
# the quality check: cornell 64x64, four frames of 4 spp, a 512-spp reference of another seed
QX, QY, QSPP, QFRAMES, QREF_SPP, QREF_SEED = 64, 64, 4, 4, 512, 0x5EED1234


def camera_path(info, n):
    """n views (eye, center, up, yview) along a small path from the scene's own: the eye drifts right and up and
    comes closer, the target follows at half the pace (a translation plus a slight turn)."""
    vp, la = np.asarray(info["VP"], F32), np.asarray(info["LA"], F32)
    out = []
    for k in range(n):
        t = F32(k)
        eye = vp + np.array([0.12, 0.05, -0.08], F32) * t
        center = la + np.array([0.06, 0.025, 0.0], F32) * t
        out.append((tuple(float(v) for v in eye), tuple(float(v) for v in center), tuple(info["UP"]),
                    float(info["yview"])))
    return out


_FRAMES = {}


def oracle_frame(pair, cam, x, y, spp, seed):
    """(frame, m2) of one layer (layer 1) at cam: the oracle's frame, and the moment frame restated from or_path as
    tests/test_gpu_noise.py oracle_moments does -- q = (((0 + r_0 * r_0) + r_1 * r_1) + ...), m2 = (0 * 0 + q / spp) / 1."""
    cam = np.asarray(cam, F32)
    key = (id(pair), cam.tobytes(), x, y, spp, seed)
    if key not in _FRAMES:
        frame, _ = pair.oracle.render(cam, x, y, spp, K, seed, layer=1)
        q = np.zeros((y, x, 3), F32)
        r = np.zeros((y, x, 3), F32)
        for s in range(spp):
            for py in range(y):
                for px in range(x):
                    r[py, px] = pair.oracle.path(cam, x, y, K, (0.0, 0.0, 0.0), seed, 1, px, py, s)
            q = q + r * r
        m2 = (np.zeros((y, x, 3), F32) * F32(0) + q * (F32(1.0) / F32(spp))) / F32(1)
        _FRAMES[key] = (frame, m2)
    return _FRAMES[key]


_CHAINS = {}


def chain(ca, pair, x, y, spp, nframes, **params):
    """[{"view", "cam", "frame", "m2", "guides", "out", "m2_out", "count", "h"}] for the frames of camera_path:
    frame k has seed SEED + k; out / m2_out / count are the model's history after it."""
    key = (id(pair), x, y, spp, nframes, tuple(sorted(params.items())))
    if key not in _CHAINS:
        hist, steps = tm.History(**params), []
        for k, view in enumerate(camera_path(pair.info, nframes)):
            cam = ca.camera(*view, x, y).as_array()
            frame, m2 = oracle_frame(pair, cam, x, y, spp, SEED + k)
            g = dm.guides_ref(pair.oracle, pair.tris, cam, x, y)
            out, m2_out, count, h = hist.step(cam, frame, m2, 1, spp, g["normal"], g["depth"])
            steps.append(dict(view=view, cam=cam, frame=frame, m2=m2, guides=g, out=out, m2_out=m2_out, count=count, h=h))
        _CHAINS[key] = steps
    return _CHAINS[key]


def coverage(step, spp):
    """(hit pixels, hit pixels that carry history, hit pixels that carry none) of a chain step."""
    hit = step["guides"]["hit"]
    carried = hit & (step["count"] > spp)
    return int(hit.sum()), int(carried.sum()), int((hit & ~carried).sum())


# --- crafted inputs of cr_reproject_device -------------------------------------------------------------------

# the current camera looks down -z at the plane z = 0 from (0.2, 0.1, 3); the previous camera is one of:
PAIRS = {
    "identical": ((0.2, 0.1, 3.0), (0.2, 0.1, 0.0), 1.0),
    "translated": ((0.5, -0.1, 3.2), (0.5, -0.1, 0.0), 1.0),
    "rotated": ((0.2, 0.1, 3.0), (0.7, 0.4, 0.0), 1.0),
    "zoomed": ((0.2, 0.1, 3.0), (0.2, 0.1, 0.0), 1.5),
    "behind": ((0.2, 0.1, -1.0), (0.2, 0.1, -4.0), 1.0),     # the plane lies behind it: ze <= 0
    "far_outside": ((0.2, 0.1, 3.0), (40.0, 0.1, 2.9), 1.0),  # it looks along the plane: u / v far outside the frame
}
CUR = ((0.2, 0.1, 3.0), (0.2, 0.1, 0.0), 1.0)


def _plane_depth(cam, x, y):
    """The distance, in units of the pixel-centre direction, to the plane z = 0 [y][x] (float32; <= 0 or inf: none)."""
    _, d = dm.guide_rays(cam, x, y)
    with np.errstate(all="ignore"):
        t = (-F32(cam[2])) / d[:, 2]
    return t.astype(F32).reshape(y, x)


def crafted(ca, x, y, pair_name):
    """dict(cam_cur, cam_prev, frame, m2, normal, depth, lmap, hist_frame, hist_m2, hist_count, hist_normal,
    hist_depth): both cameras see the plane z = 0, so a pixel's expected depth is about what the history holds there;
    on top of that random depth errors around the tolerance, three normal regions, a band of misses in each frame,
    history holes and, from pixel 0 on (as far as the frame reaches), the edge cases."""
    rng = np.random.default_rng(7000 * x + 13 * y + len(pair_name))
    up = (0.0, 1.0, 0.0)
    cur = ca.camera(CUR[0], CUR[1], up, CUR[2], x, y).as_array()
    pe, pc, pyv = PAIRS[pair_name]
    prev = ca.camera(pe, pc, up, pyv, x, y).as_array()
    n = x * y
    pal_n = dm.normalize(np.array([[0, 0, 1], [0.2, 0, 1], [1, 0, 0.2]], F32))

    def side(cam, salt):
        z = _plane_depth(cam, x, y).reshape(-1)
        z = np.where(np.isfinite(z) & (z > 0), z, F32(5)).astype(F32)
        z = (z * (F32(1) + (rng.random(n, dtype=F32) - F32(0.5)) * F32(0.16))).astype(F32)  # +-8% around a 5% gate
        region = ((np.arange(n) % x) * 3 // max(x, 1) + salt) % 3 if x > 2 else np.zeros(n, np.int64)
        nr = pal_n[region].copy()
        f = (rng.random((n, 3), dtype=F32) * F32(2)).astype(F32)
        m = ((f * f) * (F32(1) + rng.random((n, 3), dtype=F32))).astype(F32)
        miss = (np.arange(n) // x) >= (y * 5) // 6 + (1 if y < 3 else 0)   # the bottom rows (none in a 1-row frame)
        nr[miss], z[miss] = 0, F32(-1)
        return f, m, nr, z

    f, m, nr, z = side(cur, 0)
    hf, hm, hn, hz = side(prev, 0 if pair_name == "identical" else 1)
    hk = rng.integers(1, 40, n).astype(U32)
    hk[rng.random(n) < 0.1] = 0                                             # holes
    lmap = rng.integers(1, 5, n).astype(U32)
    nan, inf = F32(np.nan), F32(np.inf)
    # (array, value) per edge case, at pixel i of the current frame and of the history alike
    special = [
        [(hf, (nan, 1.0, 1.0))],                     # a NaN history pixel
        [(hm, (1.0, nan, 1.0))],                     # a NaN history moment
        [(hk, 0)],                                   # a hole
        [(hz, -1.0), (hn, (0, 0, 0))],               # a miss in the history
        [(z, -1.0), (nr, (0, 0, 0))],                # a miss in the current frame
        [(z, nan)],                                  # a NaN depth
        [(nr, (nan, nan, nan))],                     # a NaN normal in the current frame
        [(hn, (nan, 0.0, 1.0))],                     # ... in the history
        [(hk, 0xFFFFFFFF)],                          # counts near 2^32
        [(hk, 0xFFFFFFF0)],
        [(lmap, 0)],                                 # a layer map holding 0
        [(lmap, 0), (hk, 0)],                        # ... over a hole: nothing at all
        [(f, (nan, 0.5, 0.5))],                      # a NaN current pixel
        [(hf, (inf, 1.0, 1.0)), (hm, (inf, 1.0, 1.0))],  # an infinite history pixel
        [(z, 0.0)],                                  # depth 0: the point is the eye
        [(hz, 0.0)],
        [(hk, 1)],
    ]
    for i, edits in enumerate(special[:n]):
        for arr, val in edits:
            arr[i] = val
    if x > len(special) and y > 1:
        hk[x + 8], hk[x + 9] = 0xFFFFFFFE, 0xFFFFFFFD    # ... and below them: every tap of pixel 8 that counts is one
    sh3, sh1 = (y, x, 3), (y, x)
    return dict(cam_cur=cur, cam_prev=prev, frame=f.reshape(sh3), m2=m.reshape(sh3), normal=nr.reshape(sh3),
                depth=z.reshape(sh1), lmap=lmap.reshape(sh1), hist_frame=hf.reshape(sh3), hist_m2=hm.reshape(sh3),
                hist_count=hk.reshape(sh1), hist_normal=hn.reshape(sh3), hist_depth=hz.reshape(sh1))


class TpArgs(C.Structure):  # cr::TpArgs, csrc/kernels.hpp
    _fields_ = ([(n, C.c_uint32) for n in ("xres", "yres", "spp", "n_u", "max_history")]
                + [("depth_tol", C.c_float), ("normal_min", C.c_float), ("cam", C.c_float * 12),
                   ("eye_p", C.c_float * 3), ("ra", C.c_float * 3), ("rb", C.c_float * 3), ("rc", C.c_float * 3),
                   ("det", C.c_float)]
                + [(n, C.c_void_p) for n in ("layer_map", "frame", "m2", "normal", "depth", "hist_frame", "hist_m2",
                                             "hist_count", "hist_normal", "hist_depth", "hist_rec", "out", "m2_out",
                                             "count_out", "rec_out")])


def tp_args(cam_cur, cam_prev, x, y, layers, spp, depth_tol=0.05, normal_min=0.9, max_history=65536, **ptrs):
    """cr::TpArgs as cabi.cpp's reproject_args fills it, with the device pointers given by name."""
    ra, rb, rc, det = tm.projector(cam_prev)
    f = lambda a: (C.c_float * len(a))(*[float(v) for v in a])
    return TpArgs(xres=x, yres=y, spp=spp, n_u=(layers * spp) & 0xFFFFFFFF, max_history=max_history,
                  depth_tol=depth_tol, normal_min=normal_min, cam=f(cam_cur), eye_p=f(cam_prev[0:3]), ra=f(ra), rb=f(rb),
                  rc=f(rc), det=float(det), **ptrs)


def launchers(ca):
    """(launch_reproject(TpArgs *, packed, stream), launch_temporal_pack(npix, frame, m2, count, normal, depth, rec,
    stream)): the library's own launchers, which take either history layout."""
    hip = ca.libs()[0]
    rep = getattr(hip, "_ZN2cr16launch_reprojectERKNS_6TpArgsEbP12ihipStream_t")
    rep.restype, rep.argtypes = C.c_int, [C.POINTER(TpArgs), C.c_bool, C.c_void_p]
    pack = getattr(hip, "_ZN2cr20launch_temporal_packEjPKfS1_PKjS1_S1_P15HIP_vector_typeIfLj4EEP12ihipStream_t")
    pack.restype, pack.argtypes = C.c_int, [C.c_uint32] + [C.c_void_p] * 7
    return rep, pack


def crafted_ref(c, layers, spp, use_map, **params):
    return tm.reproject_ref(c["cam_cur"], c["cam_prev"], c["frame"], c["m2"], layers, spp, c["normal"], c["depth"],
                            c["hist_frame"], c["hist_m2"], c["hist_count"], c["hist_normal"], c["hist_depth"],
                            layer_map=c["lmap"] if use_map else None, **params)
