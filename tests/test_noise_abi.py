"""The noise-estimate entry points (include/chiaro_hip.h "noise estimate", include/chiaroscuro.h) without a GPU:
the symbols and their ctypes signatures, the structure layouts, and the error conventions -- a null pointer or a
bad parameter is CR_E_INVALID (checked before the device), and with no GPU every call that got that far reports
CR_E_HIP with a message instead of doing anything else."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

CR_E_INVALID, CR_E_HIP = -1, -2
HIP_NEW = ("cr_noise_struct_sizes", "cr_render_layers_noise_device", "cr_noise_device", "cr_render_layers_noise",
           "cr_noise", "cr_set_noise_accumulator", "cr_render_until")
HOST_NEW = ("chiaro_raytracer_raytrace_until", "chiaro_raytracer_noise", "chiaro_raytracer_noise_map",
            "chiaro_noise_struct_sizes")
FAKE = 0x1000  # a non-null "device pointer": no call below may get as far as touching it


def test_symbols_and_signatures(ca):
    hip, host = ca.libs()
    for n in HIP_NEW:
        assert n in ca.HIP_SYMBOLS and getattr(hip, n).argtypes is not None, n
    for n in HOST_NEW:
        assert n in ca.HOST_SYMBOLS and getattr(host, n).argtypes is not None, n
    assert len(hip.cr_render_layers_noise_device.argtypes) == 7
    assert len(hip.cr_noise_device.argtypes) == 11
    assert len(hip.cr_render_layers_noise.argtypes) == 6
    assert len(hip.cr_noise.argtypes) == 8
    assert len(hip.cr_set_noise_accumulator.argtypes) == 4
    assert len(hip.cr_render_until.argtypes) == 10
    assert len(host.chiaro_raytracer_raytrace_until.argtypes) == 11
    for m in ("render_layers_noise", "render_layers_noise_device", "noise", "noise_device", "render_until",
              "set_noise_accumulator"):
        assert callable(getattr(ca.Device, m)), m
    for m in ("rayTraceUntil", "lastNoise", "noiseMap"):
        assert callable(getattr(ca.RayTracer, m)), m


def _header_struct(name):
    """The (type, field) pairs of `typedef struct name { ... } name;` in chiaro_hip.h."""
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
    """Header, libchiaro_hip, libchiaroscuro and the ctypes mirrors agree on the two structures."""
    hip, host = ca.libs()
    ctype = {"float": C.c_float, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    for name, mirror in (("cr_noise_params", ca.CrNoiseParams), ("cr_noise_stats", ca.CrNoiseStats)):
        fields = _header_struct(name)
        assert [(n, ctype[t]) for t, n in fields] == [(n, t) for n, t in mirror._fields_], name
    for lib, fn in ((hip, "cr_noise_struct_sizes"), (host, "chiaro_noise_struct_sizes")):
        a, b = C.c_uint32(0), C.c_uint32(0)
        getattr(lib, fn)(C.byref(a), C.byref(b))
        assert (a.value, b.value) == (C.sizeof(ca.CrNoiseParams), C.sizeof(ca.CrNoiseStats)) == (8, 24), fn
    assert ca.CrNoiseStats.above.offset == 8 and ca.CrNoiseStats.max_err.offset == 16
    assert ca.CrNoiseStats.layers.offset == 20


@pytest.fixture()
def ctx(ca):
    hip, _ = ca.libs()
    c = hip.cr_create(0)
    assert c
    yield c
    hip.cr_destroy(c)


def _calls(ca, c, np_, cam=None, p=None):
    """Every new libchiaro_hip entry point with complete arguments: name -> (function, argument list)."""
    hip, _ = ca.libs()
    cam = cam or ca.camera((0, 0, 2), (0, 0, 0), (0, 1, 0), 1.0, 4, 4)
    p = p or ca.render_params(4, 4, 1, 3, 0)
    buf = (C.c_float * 48)()
    buf2 = (C.c_float * 48)()
    st = ca.CrNoiseStats()
    pn = C.byref(np_) if np_ is not None else None
    return {
        "cr_render_layers_noise_device": (hip.cr_render_layers_noise_device,
                                          [c, C.byref(cam), C.byref(p), 1, FAKE, FAKE, None]),
        "cr_noise_device": (hip.cr_noise_device, [c, 4, 4, 1, 1, pn, FAKE, FAKE, None, FAKE, None]),
        "cr_render_layers_noise": (hip.cr_render_layers_noise, [c, C.byref(cam), C.byref(p), 1, buf, buf2]),
        "cr_noise": (hip.cr_noise, [c, 4, 4, 1, 1, pn, buf, C.byref(st)]),
        "cr_set_noise_accumulator": (hip.cr_set_noise_accumulator, [c, 4, 4, buf]),
        "cr_render_until": (hip.cr_render_until, [c, C.byref(cam), C.byref(p), 1, 4, 1, pn, 0, buf, C.byref(st)]),
    }


def test_no_device_is_cr_e_hip_with_a_message(ca, ctx):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    hip, _ = ca.libs()
    for name, (fn, args) in _calls(ca, ctx, ca.CrNoiseParams(0.05, 1e-3)).items():
        assert fn(*args) == CR_E_HIP, name
        assert hip.cr_last_error(ctx), name


# (entry point, index of the argument set to null) -- every pointer the header requires
NULLS = [("cr_render_layers_noise_device", 1), ("cr_render_layers_noise_device", 2),
         ("cr_render_layers_noise_device", 4), ("cr_render_layers_noise_device", 5),
         ("cr_noise_device", 5), ("cr_noise_device", 6), ("cr_noise_device", 7), ("cr_noise_device", 9),
         ("cr_render_layers_noise", 1), ("cr_render_layers_noise", 2), ("cr_render_layers_noise", 4),
         ("cr_noise", 5), ("cr_noise", 7), ("cr_set_noise_accumulator", 3),
         ("cr_render_until", 1), ("cr_render_until", 2), ("cr_render_until", 6), ("cr_render_until", 8),
         ("cr_render_until", 9)]


@pytest.mark.parametrize("name,index", NULLS)
def test_null_pointer_is_invalid(ca, ctx, name, index):
    """With or without a GPU: the arguments are checked before the device."""
    fn, args = _calls(ca, ctx, ca.CrNoiseParams(0.05, 1e-3))[name]
    args[index] = None
    assert fn(*args) == CR_E_INVALID
    args[0] = None  # and a null context
    assert fn(*args) == CR_E_INVALID


@pytest.mark.parametrize("threshold,floor", [(0.05, 0.0), (0.05, -1.0), (0.05, float("nan")), (0.05, float("inf")),
                                             (-0.01, 1e-3), (float("nan"), 1e-3)])
def test_bad_noise_params_are_invalid(ca, ctx, threshold, floor):
    hip, _ = ca.libs()
    calls = _calls(ca, ctx, ca.CrNoiseParams(threshold, floor))
    for name in ("cr_noise_device", "cr_noise", "cr_render_until"):
        fn, args = calls[name]
        assert fn(*args) == CR_E_INVALID, name
        assert hip.cr_last_error(ctx), name


def test_bad_shapes_and_counts_are_invalid(ca, ctx):
    good = ca.CrNoiseParams(0.05, 1e-3)
    for name, index, value in (("cr_noise_device", 1, 0), ("cr_noise_device", 3, 0), ("cr_noise_device", 4, 0),
                               ("cr_noise", 2, 0), ("cr_noise", 3, 0), ("cr_set_noise_accumulator", 1, 0),
                               ("cr_render_layers_noise_device", 3, 0), ("cr_render_layers_noise", 3, 0),
                               ("cr_render_until", 5, 0),    # check_every 0
                               ("cr_render_until", 4, 0)):   # max_layers below p->layer
        fn, args = _calls(ca, ctx, good)[name]
        args[index] = value
        assert fn(*args) == CR_E_INVALID, (name, index)
    # layers * spp must fit the float conversion's 32-bit operand
    fn, args = _calls(ca, ctx, good)["cr_noise_device"]
    args[3], args[4] = 1 << 20, 1 << 20
    assert fn(*args) == CR_E_INVALID


def test_host_mirror_rejects_null(ca):
    _, host = ca.libs()
    v = (C.c_float * 3)(0, 0, 0)
    assert host.chiaro_raytracer_raytrace_until(None, 0.05, 4, v, v, v, 1.0, 1e-3, 1, 0, None) == CR_E_INVALID
    assert host.chiaro_raytracer_noise(None, None) == CR_E_INVALID
    assert host.chiaro_raytracer_noise_map(None, None) == CR_E_INVALID
