"""The adaptive-sampling entry points (include/chiaro_hip.h "adaptive sampling", include/chiaroscuro.h) without a GPU:
the symbols in both libraries, the structure layouts against the ctypes mirrors, and the order of the checks -- every
CR_E_INVALID case the header lists is answered on a ctx that has no device, before CR_E_HIP, and complete arguments
on such a ctx are CR_E_HIP with cr_create's message."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "chiaroscuro-raytracer_amd" / "lib"

CR_E_INVALID, CR_E_HIP = -1, -2
HIP_NEW = ("cr_adaptive_struct_sizes", "cr_render_layers_list_device", "cr_noise_select_device", "cr_render_adaptive")
HOST_NEW = ("chiaro_raytracer_raytrace_adaptive", "chiaro_raytracer_adaptive", "chiaro_raytracer_layer_map")
FAKE = 0x1000     # a non-null "device pointer": no call below may get as far as touching it
NO_DEVICE = 1 << 20


def test_symbols_are_exported():
    """By the libraries' own dynamic symbol tables."""
    import subprocess
    for lib, names in (("libchiaro_hip.so", HIP_NEW), ("libchiaroscuro.so", HOST_NEW)):
        table = subprocess.run(["nm", "-D", "--defined-only", str(LIB / lib)], capture_output=True, text=True,
                               check=True).stdout
        defined = {line.split()[-1] for line in table.splitlines() if line.strip()}
        for n in names:
            assert n in defined, (lib, n)


def test_signatures_and_mirrors(ca):
    hip, host = ca.libs()
    for n in HIP_NEW:
        assert n in ca.HIP_SYMBOLS and getattr(hip, n).argtypes is not None, n
    for n in HOST_NEW:
        assert n in ca.HOST_SYMBOLS and getattr(host, n).argtypes is not None, n
    assert len(hip.cr_render_layers_list_device.argtypes) == 9
    assert len(hip.cr_noise_select_device.argtypes) == 13
    assert len(hip.cr_render_adaptive.argtypes) == 9
    assert len(host.chiaro_raytracer_raytrace_adaptive.argtypes) == 11
    for m in ("render_layers_list", "noise_select", "render_adaptive"):
        assert callable(getattr(ca.Device, m)), m
    for m in ("rayTraceAdaptive", "lastAdaptive", "layerMap"):
        assert callable(getattr(ca.RayTracer, m)), m


def _header_struct(name):
    src = (ROOT / "include" / "chiaro_hip.h").read_text()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            t, names = decl.split(None, 1)
            out += [(t, n.strip()) for n in names.split(",")]
    return out


def test_structure_layouts_match(ca):
    hip, _ = ca.libs()
    ctype = {"float": C.c_float, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    for name, mirror in (("cr_adaptive_params", ca.CrAdaptiveParams), ("cr_select_stats", ca.CrSelectStats),
                         ("cr_adaptive_stats", ca.CrAdaptiveStats)):
        assert [(n, ctype[t]) for t, n in _header_struct(name)] == [(n, t) for n, t in mirror._fields_], name
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    hip.cr_adaptive_struct_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (C.sizeof(ca.CrAdaptiveParams), C.sizeof(ca.CrSelectStats),
                                           C.sizeof(ca.CrAdaptiveStats)) == (12, 24, 40)
    hip.cr_adaptive_struct_sizes(None, None, None)  # (null outputs are skipped)
    assert ca.CrSelectStats.above.offset == 8 and ca.CrSelectStats.max_err.offset == 16
    assert ca.CrAdaptiveStats.pixel_layers.offset == 8 and ca.CrAdaptiveStats.max_err.offset == 32


@pytest.fixture()
def ctx(ca):
    """A ctx without a device, with or without a GPU in the machine."""
    hip, _ = ca.libs()
    c = hip.cr_create(NO_DEVICE)
    assert c
    yield c
    hip.cr_destroy(c)


def _calls(ca, c, threshold=0.05, floor=1e-3, ap=(1, 4, 1), layer=1, nranks=1, spp=1):
    hip, _ = ca.libs()
    cam = ca.camera((0, 0, 2), (0, 0, 0), (0, 1, 0), 1.0, 4, 4)
    p = ca.render_params(4, 4, spp, 3, 0, layer=layer, nranks=nranks)
    np_ = ca.CrNoiseParams(threshold, floor)
    app = ca.CrAdaptiveParams(*ap)
    buf, buf2, lmap = (C.c_float * 48)(), (C.c_float * 48)(), (C.c_uint32 * 16)()
    st = ca.CrAdaptiveStats()
    keep = (cam, p, np_, app, buf, buf2, lmap, st)
    return keep, {
        "cr_render_layers_list_device": (hip.cr_render_layers_list_device,
                                         [c, C.byref(cam), C.byref(p), 1, FAKE, 4, FAKE, FAKE, None]),
        "cr_noise_select_device": (hip.cr_noise_select_device,
                                   [c, 4, 4, 1, 1, C.byref(np_), FAKE, FAKE, FAKE, 4, FAKE, FAKE, None]),
        "cr_render_adaptive": (hip.cr_render_adaptive, [c, C.byref(cam), C.byref(p), C.byref(app), C.byref(np_), buf,
                                                        buf2, lmap, C.byref(st)]),
    }


def test_complete_arguments_reach_the_device_check(ca, ctx):
    hip, _ = ca.libs()
    _, calls = _calls(ca, ctx)
    for name, (fn, args) in calls.items():
        assert fn(*args) == CR_E_HIP, name
        assert hip.cr_last_error(ctx), name
    # the optional pointers: no moment frame for a list render, no m2 / layer map out of the adaptive render
    fn, args = calls["cr_render_layers_list_device"]
    args[7] = None
    assert fn(*args) == CR_E_HIP
    fn, args = calls["cr_render_adaptive"]
    args[6] = args[7] = None
    assert fn(*args) == CR_E_HIP


# (entry point, index of the argument set to null) -- every pointer the header requires
NULLS = [("cr_render_layers_list_device", 1), ("cr_render_layers_list_device", 2), ("cr_render_layers_list_device", 4),
         ("cr_render_layers_list_device", 6),
         ("cr_noise_select_device", 5), ("cr_noise_select_device", 6), ("cr_noise_select_device", 7),
         ("cr_noise_select_device", 8), ("cr_noise_select_device", 10), ("cr_noise_select_device", 11),
         ("cr_render_adaptive", 1), ("cr_render_adaptive", 2), ("cr_render_adaptive", 3), ("cr_render_adaptive", 4),
         ("cr_render_adaptive", 5), ("cr_render_adaptive", 8)]


@pytest.mark.parametrize("name,index", NULLS)
def test_null_pointer_is_invalid_before_the_device(ca, ctx, name, index):
    _, calls = _calls(ca, ctx)
    fn, args = calls[name]
    args[index] = None
    assert fn(*args) == CR_E_INVALID
    args[0] = None  # and a null context
    assert fn(*args) == CR_E_INVALID


@pytest.mark.parametrize("what,kw", [
    ("check_every == 0", dict(ap=(1, 4, 0))),
    ("max_layers < 1", dict(ap=(0, 0, 1))),
    ("min_layers > max_layers", dict(ap=(5, 4, 1))),
    ("p->layer != 1", dict(layer=2)),
    ("nranks != 1", dict(nranks=2)),
    ("floor 0", dict(floor=0.0)),
    ("floor inf", dict(floor=float("inf"))),
    ("threshold negative", dict(threshold=-0.5)),
    ("threshold NaN", dict(threshold=float("nan"))),
    ("max_layers * spp above 32 bits", dict(ap=(1, 1 << 20, 1), spp=1 << 12)),
])
def test_adaptive_invalid_cases_come_before_the_device(ca, ctx, what, kw):
    hip, _ = ca.libs()
    _, calls = _calls(ca, ctx, **kw)
    fn, args = calls["cr_render_adaptive"]
    assert fn(*args) == CR_E_INVALID, what
    assert hip.cr_last_error(ctx), what


def test_list_and_select_invalid_cases(ca, ctx):
    _, calls = _calls(ca, ctx)
    fn, args = calls["cr_render_layers_list_device"]
    args[3] = 0  # no layers
    assert fn(*args) == CR_E_INVALID
    for index in (1, 2, 3, 4):  # xres, yres, layers, spp of a selection
        fn, args = _calls(ca, ctx)[1]["cr_noise_select_device"]
        args[index] = 0
        assert fn(*args) == CR_E_INVALID, index
    fn, args = _calls(ca, ctx)[1]["cr_noise_select_device"]
    args[3], args[4] = 1 << 20, 1 << 20  # layers * spp must fit 32 bits
    assert fn(*args) == CR_E_INVALID
    for bad in (dict(floor=0.0), dict(threshold=float("nan"))):
        fn, args = _calls(ca, ctx, **bad)[1]["cr_noise_select_device"]
        assert fn(*args) == CR_E_INVALID, bad
    # an empty list needs no list pointers -- and then reaches the device check
    fn, args = _calls(ca, ctx)[1]["cr_noise_select_device"]
    args[8], args[9], args[10] = None, 0, None
    assert fn(*args) == CR_E_HIP
    fn, args = _calls(ca, ctx)[1]["cr_render_layers_list_device"]
    args[4], args[5] = None, 0
    assert fn(*args) == CR_E_HIP


def test_host_mirror_rejects_null(ca):
    _, host = ca.libs()
    v = (C.c_float * 3)(0, 0, 0)
    assert host.chiaro_raytracer_raytrace_adaptive(None, 0.05, 4, v, v, v, 1.0, 1e-3, 1, 1, None) == CR_E_INVALID
    assert host.chiaro_raytracer_adaptive(None, None) == CR_E_INVALID
    assert host.chiaro_raytracer_layer_map(None, None) == CR_E_INVALID
