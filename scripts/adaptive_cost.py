"""Costs of adaptive sampling at the bench shape (sponza stand-in 1080p x 128 spp, lean build), for DESIGN.md §3.23:

1. the price of a list pass: one pass group through cr_render_layers_noise against the same layers through
   cr_render_layers_list_device with the whole frame listed in work-item order -- the unfused camera path plus the
   list indirection -- interleaved, two rounds, cr_last_kernel_ms per layer;
2. one selection at 1080p, 100 calls between two events, at about 10 %, 50 % and 100 % selected;
3. where a list pass's cost per pixel-layer stops following the pixel count: one layer over prefixes of the list;
4. end to end: cr_render_adaptive against cr_render_until with the same threshold, floor, check_every and
   max_layers, the threshold taken from a first layer so that some pixels freeze early and some never do.
One JSON line per step (the last holds everything)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "chiaroscuro-raytracer_amd")]
os.environ.setdefault("CHIARO_QUIET", "1")
import numpy as np
import torch
import chiaroscuro_amd as ca
from chiaroscuro_amd import scenes

NL = int(sys.argv[1]) if len(sys.argv) > 1 else 2      # layers of the pass group of step 1
MAXL = int(sys.argv[2]) if len(sys.argv) > 2 else 4    # max_layers of step 4
FLOOR = 1e-3
scene = ca.Scene(scenes.config_rtc("sponza"))
info = scene.info
kd = ca.KDTree(ca.Model(scene), scene)
dev = ca.Device(0)
dev.upload(kd.describe())
dev.set_option("counters", 0)
x, y, spp, k, seed = info["xres"], info["yres"], info["samples"], info["k"], info["seed"]
cam = ca.camera(info["VP"], info["LA"], info["UP"], info["yview"], x, y)
p = ca.render_params(x, y, spp, k, seed, layer=1)
out = {"shape": [x, y, spp], "layers": NL, "group": dev.layers_per_group(p, NL)}

# the frame's work items in tile-major order (tile 32), the slots of partial tiles outside it left out
T = 32
tx, ty = (x + T - 1) // T, (y + T - 1) // T
lt = np.arange(tx * ty, dtype=np.int64)[:, None, None]
oy, ox = np.arange(T, dtype=np.int64)[None, :, None], np.arange(T, dtype=np.int64)[None, None, :]
px, py = (lt % tx) * T + ox + 0 * oy, (lt // tx) * T + oy + 0 * ox
inside = (px < x) & (py < y)
order = (py * x + px)[inside].astype(np.uint32)
assert order.size == x * y and np.unique(order).size == x * y
d_list = torch.from_numpy(order.view(np.int32).copy()).cuda()
d_frame = torch.zeros((y, x, 3), dtype=torch.float32, device="cuda")
d_m2 = torch.zeros((y, x, 3), dtype=torch.float32, device="cuda")
stream = torch.cuda.current_stream().cuda_stream


def list_layers(n_list, nl):
    dev.render_layers_list(cam, p, nl, d_list.data_ptr(), n_list, d_frame.data_ptr(), d_m2.data_ptr(), stream)
    torch.cuda.synchronize()
    return dev.last_kernel_ms()


# 1. the price of a list pass
dev.render_layers_noise(cam, p, 1)
list_layers(x * y, 1)  # (warm-up: code objects, buffers)
out["noise_ms_per_layer"], out["list_ms_per_layer"] = [], []
fn = m2 = None
for r in range(2):
    fn, m2 = dev.render_layers_noise(cam, p, NL)
    out["noise_ms_per_layer"].append(dev.last_kernel_ms() / NL)
    out["list_ms_per_layer"].append(list_layers(x * y, NL) / NL)
    print(json.dumps(out), flush=True)
out["list_frame_bit_identical"] = bool((d_frame.cpu().numpy().view(np.uint32) == fn.view(np.uint32)).all())
out["list_m2_bit_identical"] = bool((d_m2.cpu().numpy().view(np.uint32) == m2.view(np.uint32)).all())

# 2. one selection at 1080p
_, err = dev.noise(x, y, NL, spp, 0.05, FLOOR)
d_out = torch.zeros(x * y, dtype=torch.int32, device="cuda")
d_st = torch.zeros(6, dtype=torch.int32, device="cuda")
out["select_us"] = {}
for share in (0.1, 0.5, 1.0):
    thr = float(np.quantile(err, 1.0 - share)) if share < 1.0 else 0.0
    call = lambda: dev.noise_select(x, y, NL, spp, thr, FLOOR, d_frame.data_ptr(), d_m2.data_ptr(), d_list.data_ptr(),
                                    x * y, d_out.data_ptr(), d_st.data_ptr(), stream)
    for _ in range(5):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(100):
        call()
    e1.record()
    torch.cuda.synchronize()
    st = ca.CrSelectStats.from_buffer_copy(d_st.cpu().numpy().tobytes()).as_dict()
    out["select_us"]["%.0f%%" % (100 * share)] = {"us": e0.elapsed_time(e1) * 10.0, "selected": st["above"] / (x * y)}
print(json.dumps(out), flush=True)

# 3. one layer over prefixes of the list: ms, and ns per pixel-layer
out["list_prefix"] = []
for n in (x * y, 1 << 20, 1 << 18, 1 << 16, 1 << 14, 1 << 12, 1 << 10):
    list_layers(n, 1)
    ms = list_layers(n, 1)
    out["list_prefix"].append({"pixels": n, "ms": ms, "ns_per_pixel_layer": ms * 1e6 / n})
print(json.dumps(out), flush=True)

# 4. end to end: the threshold from the first layer's error map -- 60 % of the pixels are at or below it after one
#    layer, and the error falls about as 1 / sqrt(layers), so those above twice it never freeze within MAXL = 4
dev.render_layers_noise(cam, p, 1)
_, err1 = dev.noise(x, y, 1, spp, 0.05, FLOOR)
thr = float(np.quantile(err1, 0.6))
out["end_to_end"] = {"threshold": thr, "floor": FLOOR, "check_every": 1, "max_layers": MAXL}
for r in range(2):
    t0 = time.perf_counter()
    _, st = dev.render_until(cam, p, 1, MAXL, 1, thr, FLOOR, 0)
    wall = (time.perf_counter() - t0) * 1e3
    kms = dev.last_kernel_ms()
    pl = x * y * st["layers"]
    out["end_to_end"]["until_%d" % r] = {"wall_ms": wall, "kernel_ms": kms, "layers": st["layers"], "above": st["above"],
                                         "pixel_layers": pl, "kernel_ns_per_pixel_layer": kms * 1e6 / pl}
    t0 = time.perf_counter()
    _, _, lmap, ast = dev.render_adaptive(cam, p, 1, MAXL, 1, thr, FLOOR, want_m2=False)
    wall = (time.perf_counter() - t0) * 1e3
    kms = dev.last_kernel_ms()
    out["end_to_end"]["adaptive_%d" % r] = {"wall_ms": wall, "kernel_ms": kms, "layers": ast["layers"],
                                            "active": ast["active"], "pixel_layers": ast["pixel_layers"],
                                            "pixels_per_layer_count": np.bincount(lmap.reshape(-1), minlength=MAXL + 1)[1:].tolist(),
                                            "kernel_ns_per_pixel_layer": kms * 1e6 / ast["pixel_layers"]}
    print(json.dumps(out), flush=True)
