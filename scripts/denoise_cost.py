"""Cost of the guide buffers and the a-trous filter at 1080p on the sponza stand-in: the time of
cr_guides_device, of cr_denoise_device at the default parameters, and of one a-trous level at steps 1, 2, 4, 8 in
both forms (tile plus halo staged in LDS / every tap through L2), each over N launches between two HIP events on
one stream, three interleaved rounds.  The single levels are launched through the library's own launcher
(cr::launch_atrous, by its mangled name) on buffers packed here from a real frame, its moments and its guides, so
both forms can be timed at every step whatever the schedule picks.  Measurement only."""
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


class DnArgs(C.Structure):  # cr::DnArgs, csrc/kernels.hpp
    _fields_ = [("xres", C.c_uint32), ("yres", C.c_uint32), ("step", C.c_uint32), ("squarings", C.c_uint32),
                ("spp", C.c_uint32), ("n", C.c_float), ("sl2", C.c_float), ("sz_step", C.c_float),
                ("inv_sa2", C.c_float)] + [(k, C.c_void_p) for k in (
                    "layer_map", "frame", "m2", "albedo", "normal", "depth", "rec", "src", "dst", "out", "var_out")]


scene = ca.Scene(scenes.config_rtc("sponza"), "samples", str(SPP))
info = scene.info
model = ca.Model(scene)
kd = ca.KDTree(model, scene)
dev = ca.Device(0)
dev.upload(kd.describe())
dev.set_option("counters", 0)
x, y = info["xres"], info["yres"]
cam = ca.camera(info["VP"], info["LA"], info["UP"], info["yview"], x, y)
p = ca.render_params(x, y, SPP, info["k"], info["seed"], layer=1)
frame, m2 = dev.render_layers_noise(cam, p, LAYERS)
npix = x * y
out = {"shape": [x, y], "spp": SPP, "layers": LAYERS, "launches": N, "triangles": dev.scene_triangles()}
s = torch.cuda.current_stream().cuda_stream
df, dm = torch.from_numpy(frame).cuda(), torch.from_numpy(m2).cuda()
da = torch.zeros((y, x, 3), dtype=torch.float32, device="cuda")
dn = torch.zeros((y, x, 3), dtype=torch.float32, device="cuda")
dz = torch.zeros((y, x), dtype=torch.float32, device="cuda")
dout = torch.zeros((y, x, 3), dtype=torch.float32, device="cuda")
dvar = torch.zeros((y, x), dtype=torch.float32, device="cuda")


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


guides = lambda: dev.guides_device(cam, x, y, da.data_ptr(), dn.data_ptr(), dz.data_ptr(), s)
dp = ca.denoise_params()
full = lambda: dev.denoise_device(x, y, LAYERS, SPP, dp, df.data_ptr(), dm.data_ptr(), 0, da.data_ptr(), dn.data_ptr(),
                                  dz.data_ptr(), dout.data_ptr(), dvar.data_ptr(), s)
dp0 = ca.denoise_params(levels=0)
init = lambda: dev.denoise_device(x, y, LAYERS, SPP, dp0, df.data_ptr(), dm.data_ptr(), 0, da.data_ptr(), dn.data_ptr(),
                                  dz.data_ptr(), dout.data_ptr(), dvar.data_ptr(), s)
guides()
torch.cuda.synchronize()
out["hit_fraction"] = float((dz >= 0).float().mean())
init()
torch.cuda.synchronize()
# the packed buffers of one level, as guide_pack and var_init write them
src = torch.cat([dout, dvar[..., None]], dim=2).contiguous()
dst = torch.zeros_like(src)
rec = torch.stack([torch.cat([da, dz[..., None]], dim=2), torch.cat([dn, torch.zeros_like(dz)[..., None]], dim=2)],
                  dim=2).contiguous()
assert src.shape == (y, x, 4) and rec.shape == (y, x, 2, 4)
hip = ca.libs()[0]
launch = getattr(hip, "_ZN2cr13launch_atrousERKNS_6DnArgsEbP12ihipStream_t")
launch.restype, launch.argtypes = C.c_int, [C.POINTER(DnArgs), C.c_bool, C.c_void_p]


def level(step, lds):
    a = DnArgs(xres=x, yres=y, step=step, squarings=dp.normal_squarings, spp=SPP, n=float(LAYERS * SPP),
               sl2=dp.sigma_l * dp.sigma_l, sz_step=dp.sigma_z * step, inv_sa2=1.0 / (dp.sigma_a * dp.sigma_a),
               rec=rec.data_ptr(), src=src.data_ptr(), dst=dst.data_ptr())
    def run():
        rc = launch(C.byref(a), bool(lds), s)
        assert rc == 0, rc
    return run


level_bytes = npix * (16 + 32 + 16)  # compulsory: the frame and record read once, the frame written once
out["level_bytes"] = level_bytes
out["level_floor_us"] = level_bytes / HBM * 1e6
rows = {"guides_us": [], "denoise_default_us": [], "var_init_us": []}
for st in (1, 2, 4, 8):
    for lds in ((1, 0) if st <= 2 else (0,)):
        rows["step%d_%s_us" % (st, "lds" if lds else "l2")] = []
# the two forms write the same bits
for st in (1, 2):
    level(st, 1)()
    torch.cuda.synchronize()
    a = dst.clone()
    level(st, 0)()
    torch.cuda.synchronize()
    out["step%d_forms_bit_identical" % st] = bool((a.view(torch.int32) == dst.view(torch.int32)).all())
for r in range(3):
    rows["guides_us"].append(timed(guides, max(20, N // 4)))
    rows["denoise_default_us"].append(timed(full))
    rows["var_init_us"].append(timed(init))
    for st in (1, 2, 4, 8):
        for lds in ((1, 0) if st <= 2 else (0,)):
            rows["step%d_%s_us" % (st, "lds" if lds else "l2")].append(timed(level(st, lds)))
    out.update(rows)
    print(json.dumps(out), flush=True)
out["fraction_of_floor"] = {k: out["level_floor_us"] / min(v) for k, v in rows.items() if k.startswith("step")}
print(json.dumps(out), flush=True)
