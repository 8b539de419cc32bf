"""One cr_ctx and one cr_group reused across frame sizes, scenes and entry points (csrc/devres.hpp's owners).

What the CPU checks cannot see: an accumulator that is resized, scoped buffers that come and go, a scene replaced by
another and put back, a group's frame resized, and everything destroyed at the end.  cornell_box at 8x8 and 16x8
(one tile each: the smallest frames that still resize an accumulator), 2 samples, depth 3; every comparison is
bitwise against a fresh ctx.
"""
import ctypes as C

import numpy as np
import pytest

import torture
from helpers import assert_bitwise

pytestmark = pytest.mark.gpu

SEED, SPP, K = 0xC41A05C0, 2, 3
CR_E_INVALID = -1


def _tree(ca, rtc, *overrides):
    scene = ca.Scene(rtc, *overrides)
    model = ca.Model(scene)
    return scene, ca.KDTree(model, scene)


def _tonemap(ca, dev, x, y):
    out = np.zeros((y, x, 3), np.uint8)
    t = ca.tonemap_params(2.0)
    rc = ca.libs()[0].cr_tonemap(dev._c, C.byref(t), x, y, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return rc, out


def test_ctx_and_group_reused(ca, scenes, tmp_path):
    import torch
    scene, kd = _tree(ca, scenes.config_rtc("cornell_box"))
    i = scene.info
    cam = {x: ca.camera(i["VP"], i["LA"], i["UP"], i["yview"], x, 8) for x in (8, 16)}
    par = {x: ca.render_params(x, 8, SPP, K, SEED) for x in (8, 16)}

    def fresh(x):
        d = ca.Device(0)
        d.upload(kd.describe())
        img = d.render(cam[x], par[x])
        return d, img

    (d8, want8), (d16, want16) = fresh(8), fresh(16)
    assert want8.any() and want16.any()
    want8_bytes = _tonemap(ca, d8, 8, 8)
    assert want8_bytes[0] == 0
    d8.close()
    d16.close()

    # one ctx: the accumulator resized there and back
    d = ca.Device(0)
    d.upload(kd.describe())
    a, b, c = (d.render(cam[x], par[x]) for x in (8, 16, 8))
    assert_bitwise(a, want8, "first 8x8")
    assert_bitwise(b, want16, "16x8 after 8x8")
    assert_bitwise(c, want8, "8x8 after 16x8")

    # both accumulators at 8x8; cr_noise and cr_tonemap refuse another size and still serve this one
    frame, _ = d.render_layers_noise(cam[8], par[8], 2)
    stats, err = d.noise(8, 8, 2, SPP, 0.05, 0.01)
    assert stats["pixels"] == 64 and stats["layers"] == 2 and err.shape == (8, 8)
    np_, st = ca.CrNoiseParams(0.05, 0.01), ca.CrNoiseStats()
    assert ca.libs()[0].cr_noise(d._c, 16, 8, 2, SPP, C.byref(np_), None, C.byref(st)) == CR_E_INVALID
    assert _tonemap(ca, d, 16, 8)[0] == CR_E_INVALID
    two = ca.Device(0)  # the fresh ctx of the two-layer frame
    two.upload(kd.describe())
    want_frame, _ = two.render_layers_noise(cam[8], par[8], 2)
    assert_bitwise(frame, want_frame, "two layers after the resizes")
    rc, got_bytes = _tonemap(ca, d, 8, 8)
    assert rc == 0 and np.array_equal(got_bytes, _tonemap(ca, two, 8, 8)[1])
    d.render(cam[8], par[8])
    assert np.array_equal(_tonemap(ca, d, 8, 8)[1], want8_bytes[1])
    two.close()

    # the scoped query buffers of cr_intersect against the ctx's own of cr_intersect_device
    eye = np.asarray(i["VP"], np.float32)
    to = np.asarray(i["LA"], np.float32) - eye
    offsets = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (-1, -1, 0))
    dirs = np.stack([to + np.float32(0.1) * np.asarray(o, np.float32) for o in offsets])
    dirs = (dirs / np.linalg.norm(dirs, axis=1)[:, None]).astype(np.float32)
    orig = np.tile(eye, (4, 1))
    host = d.intersect(orig, dirs)
    devq = d.intersect_tensors(torch.from_numpy(orig).cuda(), torch.from_numpy(dirs).cuda())
    torch.cuda.synchronize()
    assert host["hit"].any()
    for k in ("hit", "tri"):
        assert np.array_equal(host[k], devq[k].cpu().numpy().view(np.uint32)), k
    for k in ("bary", "dist"):
        assert_bitwise(host[k], devq[k].cpu().numpy(), k)

    # another scene and back
    soup = torture.build("mini", torture.PLACEMENTS["origin"])
    _, other = _tree(ca, scenes.config_rtc("cornell_box"), "input", str(torture.write_obj(tmp_path / "mini.obj", soup)))
    d.upload(other.describe())
    assert d.scene_triangles() == len(soup["pos"])
    d.upload(kd.describe())
    assert_bitwise(d.render(cam[8], par[8]), want8, "cornell_box after the torture scene")
    d.close()

    # a group over one device: its frame resized
    g = ca.Group([0])
    g.upload(kd.describe())
    assert_bitwise(g.render(cam[8], par[8]), want8, "group 8x8")
    assert_bitwise(g.render(cam[16], par[16]), want16, "group 16x8")
    g.close()

    last = ca.Device(0)
    last.synchronize()  # (raises unless cr_synchronize returns CR_OK)
    last.close()
