"""The radiance-query entry points (include/chiaro_hip.h "radiance queries", include/chiaroscuro.h) without a GPU:
the symbols in both libraries, the structure layout against the ctypes mirror, and the order of the checks -- every
CR_E_INVALID case the header lists is answered on a ctx that has no device, before CR_E_HIP, and complete arguments
on such a ctx are CR_E_HIP with cr_create's message."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "chiaroscuro-raytracer_amd" / "lib"

CR_OK, CR_E_INVALID, CR_E_HIP = 0, -1, -2
DEVICE_FORMS = ("cr_radiance_device", "cr_gather_device")
HOST_FORMS = ("cr_radiance", "cr_gather")
HIP_NEW = ("cr_radiance_struct_sizes",) + DEVICE_FORMS + HOST_FORMS
HOST_NEW = ("chiaro_raytracer_radiance", "chiaro_raytracer_gather")
FAKE = 0x1000     # a non-null "device pointer": no call below may get as far as touching it
NO_DEVICE = 1 << 20
N = 4


def test_symbols_are_exported():
    """By the libraries' own dynamic symbol tables."""
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
    for n in DEVICE_FORMS:
        assert len(getattr(hip, n).argtypes) == 9, n
    for n in HOST_FORMS:
        assert len(getattr(hip, n).argtypes) == 8, n
    for n in HOST_NEW:
        assert len(getattr(host, n).argtypes) == 6, n
    for m in ("radiance_device", "gather_device", "radiance", "gather"):
        assert callable(getattr(ca.Device, m)), m
    for m in ("radiance", "gather"):
        assert callable(getattr(ca.RayTracer, m)), m


def test_structure_layout_matches(ca):
    hip, _ = ca.libs()
    src = (ROOT / "include" / "chiaro_hip.h").read_text()
    body = re.search(r"typedef struct cr_radiance_params \{(.*?)\} cr_radiance_params;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"float": C.c_float, "uint32_t": C.c_uint32, "int32_t": C.c_int32}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            t, name = decl.split(None, 1)
            arr = re.fullmatch(r"(\w+)\[(\d+)\]", name.strip())
            fields.append((arr.group(1), ctype[t] * int(arr.group(2))) if arr else (name.strip(), ctype[t]))
    assert fields == [(n, t) for n, t in ca.CrRadianceParams._fields_]
    a = C.c_uint32(0)
    hip.cr_radiance_struct_sizes(C.byref(a))
    assert a.value == C.sizeof(ca.CrRadianceParams) == 32
    hip.cr_radiance_struct_sizes(None)  # (a null output is skipped)
    assert ca.CrRadianceParams.background.offset == 8 and ca.CrRadianceParams.id0.offset == 28
    rp = ca.radiance_params(5, 6, 0xC41A05C0, (0.1, 0.2, 0.3), layer=2, id0=100)
    assert (rp.spp, rp.k, rp.seed, rp.layer, rp.id0) == (5, 6, 0xC41A05C0, 2, 100)
    assert [rp.background[i] for i in range(3)] == [C.c_float(v).value for v in (0.1, 0.2, 0.3)]


@pytest.fixture()
def ctx(ca):
    """A ctx without a device, with or without a GPU in the machine."""
    hip, _ = ca.libs()
    c = hip.cr_create(NO_DEVICE)
    assert c
    yield c
    hip.cr_destroy(c)


def _call(ca, c, name, n=N, nlayers=1, **kw):
    """(function, arguments, what keeps them alive) of one entry point with complete arguments."""
    hip, _ = ca.libs()
    rp = ca.radiance_params(kw.pop("spp", 2), kw.pop("k", 3), 1, (0.1, 0.2, 0.3), layer=kw.pop("layer", 1),
                            id0=kw.pop("id0", 0))
    assert not kw
    if name in DEVICE_FORMS:
        return getattr(hip, name), [c, n, FAKE, FAKE, C.byref(rp), nlayers, FAKE, FAKE, None], rp
    a, b, out, m2 = ((C.c_float * (3 * N))() for _ in range(4))
    return getattr(hip, name), [c, n, a, b, C.byref(rp), nlayers, out, m2], (rp, a, b, out, m2)


@pytest.mark.parametrize("name", DEVICE_FORMS + HOST_FORMS)
def test_complete_arguments_reach_the_device_check(ca, ctx, name):
    hip, _ = ca.libs()
    fn, args, _keep = _call(ca, ctx, name)
    assert fn(*args) == CR_E_HIP
    assert hip.cr_last_error(ctx)
    args[7] = None  # the moment array is optional
    assert fn(*args) == CR_E_HIP
    # no rays need no arrays -- and then reach the device check (with a device and a scene: CR_OK, nothing launched)
    fn, args, _keep = _call(ca, ctx, name, n=0)
    args[2] = args[3] = args[6] = args[7] = None
    assert fn(*args) == CR_E_HIP


@pytest.mark.parametrize("name", DEVICE_FORMS + HOST_FORMS)
@pytest.mark.parametrize("index", [2, 3, 4, 6])  # the two input arrays, the params, the output
def test_null_pointer_is_invalid_before_the_device(ca, ctx, name, index):
    fn, args, _keep = _call(ca, ctx, name)
    args[index] = None
    assert fn(*args) == CR_E_INVALID
    args[0] = None  # and a null context
    assert fn(*args) == CR_E_INVALID


@pytest.mark.parametrize("name", DEVICE_FORMS + HOST_FORMS)
@pytest.mark.parametrize("what,kw", [
    ("spp == 0", dict(spp=0)),
    ("k == 0", dict(k=0)),
    ("k == 65", dict(k=65)),
    ("k negative", dict(k=-3)),
    ("layer == 0", dict(layer=0)),
    ("nlayers == 0", dict(nlayers=0)),
    ("id overflow", dict(id0=0xffffffff - N + 1)),
    ("id overflow with no rays' worth of room", dict(id0=0xffffffff)),
])
def test_invalid_cases_come_before_the_device(ca, ctx, name, what, kw):
    hip, _ = ca.libs()
    fn, args, _keep = _call(ca, ctx, name, **kw)
    assert fn(*args) == CR_E_INVALID, what
    assert hip.cr_last_error(ctx), what


@pytest.mark.parametrize("name", DEVICE_FORMS + HOST_FORMS)
def test_the_sound_edges_reach_the_device_check(ca, ctx, name):
    """k at 1 and 64 and the last stream id are sound: CR_E_HIP on a ctx without a device, not CR_E_INVALID."""
    for kw in (dict(k=1), dict(k=64), dict(id0=0xffffffff - N), dict(n=0, id0=0xffffffff)):
        fn, args, _keep = _call(ca, ctx, name, **kw)
        assert fn(*args) == CR_E_HIP, kw


def test_null_context(ca):
    for name in DEVICE_FORMS + HOST_FORMS:
        fn, args, _keep = _call(ca, None, name)
        assert fn(*args) == CR_E_INVALID, name


def test_host_mirror_rejects_null(ca):
    _, host = ca.libs()
    v = (C.c_float * 3)(0, 0, 1)
    for fn in (host.chiaro_raytracer_radiance, host.chiaro_raytracer_gather):
        assert fn(None, v, v, 1, 1, v) == CR_E_INVALID
