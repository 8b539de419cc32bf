"""Cost of temporal reprojection at 1080p on the sponza stand-in: the time of cr_reproject_device
and of the reprojection kernel on both history layouts -- the five planar arrays, and the packed record of three
float4 per pixel, with and without the kernel writing the next frame's record -- each over N launches between two HIP
events on one stream, three interleaved rounds.  The layouts are launched through the library's own launcher
(cr::launch_reproject, by its mangled name) on a real history: the frame, moments and guides of the scene's camera,
reprojected to a camera a step aside.  Reports the kernel's compulsory traffic over the float4-copy rate §3.25
measured, and whether both layouts wrote the same bits.  Measurement only."""
import ctypes as C
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "chiaroscuro-raytracer_amd")]
os.environ.setdefault("CHIARO_QUIET", "1")
import numpy as np
import torch
import chiaroscuro_amd as ca
from chiaroscuro_amd import scenes

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200
SPP, LAYERS = 4, 2
HBM = 6.3e12  # achievable bytes / s (float4 copy)


class TpArgs(C.Structure):  # cr::TpArgs, csrc/kernels.hpp
    _fields_ = ([(n, C.c_uint32) for n in ("xres", "yres", "spp", "n_u", "max_history")]
                + [("depth_tol", C.c_float), ("normal_min", C.c_float), ("cam", C.c_float * 12),
                   ("eye_p", C.c_float * 3), ("ra", C.c_float * 3), ("rb", C.c_float * 3), ("rc", C.c_float * 3),
                   ("det", C.c_float)]
                + [(n, C.c_void_p) for n in ("layer_map", "frame", "m2", "normal", "depth", "hist_frame", "hist_m2",
                                             "hist_count", "hist_normal", "hist_depth", "hist_rec", "out", "m2_out",
                                             "count_out", "rec_out")])


scene = ca.Scene(scenes.config_rtc("sponza"), "samples", str(SPP))
info = scene.info
model = ca.Model(scene)
kd = ca.KDTree(model, scene)
dev = ca.Device(0)
dev.upload(kd.describe())
dev.set_option("counters", 0)
x, y = info["xres"], info["yres"]
npix = x * y
vp, la = np.asarray(info["VP"], np.float32), np.asarray(info["LA"], np.float32)
step = (la - vp) * np.float32(0.02) + np.float32(0.01) * np.linalg.norm(la - vp) * np.array([1, 0.5, 0], np.float32)
cams = [ca.camera(info["VP"], info["LA"], info["UP"], info["yview"], x, y),
        ca.camera(tuple(vp + step), tuple(la + step * np.float32(0.5)), info["UP"], info["yview"], x, y)]
out = {"shape": [x, y], "spp": SPP, "layers": LAYERS, "launches": N, "triangles": dev.scene_triangles()}
s = torch.cuda.current_stream().cuda_stream
side = []
for k, cam in enumerate(cams):
    f, m = dev.render_layers_noise(cam, ca.render_params(x, y, SPP, info["k"], info["seed"] + k, layer=1), LAYERS)
    g = dev.guides(cam, x, y, want=("normal", "depth"))
    side.append({n: torch.from_numpy(np.ascontiguousarray(a)).cuda()
                 for n, a in (("frame", f), ("m2", m), ("normal", g["normal"]), ("depth", g["depth"]))})
hist, cur = side
hcount = torch.full((y, x), LAYERS * SPP, dtype=torch.int32, device="cuda")
o_f, o_m = torch.zeros((y, x, 3), device="cuda"), torch.zeros((y, x, 3), device="cuda")
o_k = torch.zeros((y, x), dtype=torch.int32, device="cuda")
rec, rec_out = torch.zeros((npix, 3, 4), device="cuda"), torch.zeros((npix, 3, 4), device="cuda")
tp = ca.temporal_params()
hip = ca.libs()[0]
launch = getattr(hip, "_ZN2cr16launch_reprojectERKNS_6TpArgsEbP12ihipStream_t")
launch.restype, launch.argtypes = C.c_int, [C.POINTER(TpArgs), C.c_bool, C.c_void_p]
pack = getattr(hip, "_ZN2cr20launch_temporal_packEjPKfS1_PKjS1_S1_P15HIP_vector_typeIfLj4EEP12ihipStream_t")
pack.restype, pack.argtypes = C.c_int, [C.c_uint32] + [C.c_void_p] * 7


def cross(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float32)


def args(packed, write_rec):
    c, p = cams[1].as_array(), cams[0].as_array()
    lu, dx, dy = p[3:6], p[6:9], p[9:12]
    ra, rb, rc = cross(dx, dy), cross(dy, lu), cross(lu, dx)
    det = np.float32((lu[0] * ra[0] + lu[1] * ra[1]) + lu[2] * ra[2])
    f = lambda a: (C.c_float * len(a))(*[float(v) for v in a])
    a = TpArgs(xres=x, yres=y, spp=SPP, n_u=LAYERS * SPP, max_history=tp.max_history, depth_tol=tp.depth_tol,
               normal_min=tp.normal_min, cam=f(c), eye_p=f(p[0:3]), ra=f(ra), rb=f(rb), rc=f(rc), det=float(det),
               frame=cur["frame"].data_ptr(), m2=cur["m2"].data_ptr(), normal=cur["normal"].data_ptr(),
               depth=cur["depth"].data_ptr(), out=o_f.data_ptr(), m2_out=o_m.data_ptr(), count_out=o_k.data_ptr(),
               rec_out=rec_out.data_ptr() if write_rec else None)
    if packed:
        a.hist_rec = rec.data_ptr()
    else:
        a.hist_frame, a.hist_m2, a.hist_count = hist["frame"].data_ptr(), hist["m2"].data_ptr(), hcount.data_ptr()
        a.hist_normal, a.hist_depth = hist["normal"].data_ptr(), hist["depth"].data_ptr()
    return a


def kernel(packed, write_rec=False):
    a = args(packed, write_rec)
    def run():
        rc = launch(C.byref(a), bool(packed), s)
        assert rc == 0, rc
    return run


def timed(fn, n=N):
    """us per call of fn over n calls between two events (5 warm-up calls first)."""
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


api = lambda: dev.reproject_device(cams[1], cams[0], x, y, LAYERS, SPP, tp, cur["frame"].data_ptr(), cur["m2"].data_ptr(),
                                   0, cur["normal"].data_ptr(), cur["depth"].data_ptr(), hist["frame"].data_ptr(),
                                   hist["m2"].data_ptr(), hcount.data_ptr(), hist["normal"].data_ptr(),
                                   hist["depth"].data_ptr(), o_f.data_ptr(), o_m.data_ptr(), o_k.data_ptr(), s)
do_pack = lambda: pack(npix, hist["frame"].data_ptr(), hist["m2"].data_ptr(), hcount.data_ptr(), hist["normal"].data_ptr(),
                       hist["depth"].data_ptr(), rec.data_ptr(), s)
assert do_pack() == 0
# both layouts write the same bits, and those of the entry point
results = []
for fn in (api, kernel(False), kernel(True), kernel(True, True)):
    o_f.zero_(), o_m.zero_(), o_k.zero_()
    fn()
    torch.cuda.synchronize()
    results.append((o_f.clone(), o_m.clone(), o_k.clone()))
canon = lambda t: torch.where(torch.isnan(t), torch.zeros_like(t), t).view(torch.int32) if t.dtype == torch.float32 else t
out["layouts_bit_identical"] = all(bool((canon(a) == canon(b)).all()) for r in results[1:] for a, b in zip(results[0], r))
hit = cur["depth"] >= 0
out["hit_fraction"] = float(hit.float().mean())
out["history_found_fraction_of_hits"] = float((results[0][2][hit] > LAYERS * SPP).float().mean())
# compulsory traffic per pixel: the current frame, moments, normal and depth (40 B) and the outputs (28 B) once, and
# the history once -- 44 B in five planar arrays, 48 B as the record (+ 48 B when the next record is written too)
bytes_px = {"planar": 40 + 44 + 28, "packed": 40 + 48 + 28, "packed_rec_out": 40 + 48 + 28 + 48, "pack": 44 + 48}
out["bytes_per_pixel"] = bytes_px
out["floor_us"] = {k: npix * b / HBM * 1e6 for k, b in bytes_px.items()}
rows = {"reproject_device_us": [], "planar_us": [], "packed_us": [], "packed_rec_out_us": [], "pack_us": []}
for r in range(3):
    rows["reproject_device_us"].append(timed(api))
    rows["planar_us"].append(timed(kernel(False)))
    rows["packed_us"].append(timed(kernel(True)))
    rows["packed_rec_out_us"].append(timed(kernel(True, True)))
    rows["pack_us"].append(timed(do_pack))
    out.update(rows)
    print(json.dumps(out), flush=True)
out["fraction_of_floor"] = {k: out["floor_us"][k] / min(rows[k + "_us"]) for k in bytes_px}
print(json.dumps(out), flush=True)
