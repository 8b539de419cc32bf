"""Cost of the moment tracking at the bench shape (sponza stand-in 1080p x 128 spp, a pass group of 16 layers, lean
build): cr_last_kernel_ms of cr_render_layers vs cr_render_layers_noise on the same layers, interleaved, and the
time of one noise evaluation at 1080p."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "chiaroscuro-raytracer_amd")]
os.environ.setdefault("CHIARO_QUIET", "1")
import numpy as np
import torch
import chiaroscuro_amd as ca
from chiaroscuro_amd import scenes

NL = int(sys.argv[1]) if len(sys.argv) > 1 else 16
rtc = scenes.config_rtc("sponza")
scene = ca.Scene(rtc)
info = scene.info
model = ca.Model(scene)
kd = ca.KDTree(model, scene)
dev = ca.Device(0)
dev.upload(kd.describe())
dev.set_option("counters", 0)
x, y, spp, k, seed = info["xres"], info["yres"], info["samples"], info["k"], info["seed"]
cam = ca.camera(info["VP"], info["LA"], info["UP"], info["yview"], x, y)
p = ca.render_params(x, y, spp, k, seed, layer=1)
out = {"shape": [x, y, spp], "layers": NL, "group": dev.layers_per_group(p, NL), "plain_ms_per_layer": [],
       "noise_ms_per_layer": []}
dev.render_layers(cam, p, 1)
dev.render_layers_noise(cam, p, 1)  # (warm-up: code objects, buffers)
fp = fn = m2 = None
for r in range(2):
    fp = dev.render_layers(cam, p, NL)
    out["plain_ms_per_layer"].append(dev.last_kernel_ms() / NL)
    fn, m2 = dev.render_layers_noise(cam, p, NL)
    out["noise_ms_per_layer"].append(dev.last_kernel_ms() / NL)
    print(json.dumps(out), flush=True)
out["frames_bit_identical"] = bool((fp.view(np.uint32) == fn.view(np.uint32)).all())
t0 = time.perf_counter()
st, _ = dev.noise(x, y, NL, spp, 0.05, 1e-3, want_err=False)
out["cr_noise_host_ms"] = (time.perf_counter() - t0) * 1e3
out["stats"] = st
df, dm = torch.from_numpy(fn).cuda(), torch.from_numpy(m2).cuda()
derr = torch.zeros((y, x), dtype=torch.float32, device="cuda")
dst = torch.zeros(6, dtype=torch.int32, device="cuda")
s = torch.cuda.current_stream().cuda_stream
for with_err in (1, 0):
    for _ in range(5):
        dev.noise_device(x, y, NL, spp, 0.05, 1e-3, df.data_ptr(), dm.data_ptr(), derr.data_ptr() if with_err else 0,
                         dst.data_ptr(), s)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(100):
        dev.noise_device(x, y, NL, spp, 0.05, 1e-3, df.data_ptr(), dm.data_ptr(), derr.data_ptr() if with_err else 0,
                         dst.data_ptr(), s)
    e1.record()
    torch.cuda.synchronize()
    out["noise_device_us_err%d" % with_err] = e0.elapsed_time(e1) * 10.0  # ms / 100 calls -> us per call
print(json.dumps(out), flush=True)
