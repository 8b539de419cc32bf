"""The probe entry points (include/chiaro_hip.h "probes", include/chiaroscuro.h) without a GPU: the symbols in both
libraries, the structure layout against the ctypes mirror, cr_probe_grid_positions (which needs no device), and the
order of the checks -- every CR_E_INVALID case is answered on a ctx that has no device, before CR_E_HIP, complete
arguments on such a ctx are CR_E_HIP, and a null ctx is CR_E_INVALID."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import probe_model as pm

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "chiaroscuro-raytracer_amd" / "lib"
CR_OK, CR_E_INVALID, CR_E_HIP = 0, -1, -2
HIP_NEW = ("cr_probe_struct_sizes", "cr_probe_grid_positions", "cr_probe_sh_device", "cr_probe_sh",
           "cr_probe_eval_device", "cr_probe_sample_device", "cr_probe_eval", "cr_probe_sample")
HOST_NEW = ("chiaro_raytracer_probes", "chiaro_raytracer_probes_sample")
FAKE = 0x1000     # a non-null "device pointer": no call below may get as far as touching it
NO_DEVICE = 1 << 20
F32 = np.float32
FP, UP = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


def test_symbols_are_exported():
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
    for n, count in (("cr_probe_grid_positions", 2), ("cr_probe_sh_device", 8), ("cr_probe_sh", 7),
                     ("cr_probe_eval_device", 7), ("cr_probe_sample_device", 8), ("cr_probe_eval", 7),
                     ("cr_probe_sample", 7)):
        assert len(getattr(hip, n).argtypes) == count, n
    # every entry that takes the ctx takes it as the CTX kind
    for n in HIP_NEW[2:]:
        assert getattr(hip, n).argtypes[0] is ca.CTX, n
    assert len(host.chiaro_raytracer_probes.argtypes) == 6 and len(host.chiaro_raytracer_probes_sample.argtypes) == 7
    for m in ("probe_sh_device", "probe_sh", "probe_eval_device", "probe_sample_device", "probe_eval", "probe_sample"):
        assert callable(getattr(ca.Device, m)), m
    assert callable(ca.RayTracer.bakeProbes) and callable(ca.RayTracer.sampleProbes) and callable(ca.probe_grid)


def test_structure_layout_matches(ca):
    hip, _ = ca.libs()
    src = (ROOT / "include" / "chiaro_hip.h").read_text()
    body = re.search(r"typedef struct cr_probe_grid \{(.*?)\} cr_probe_grid;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"float": C.c_float, "uint32_t": C.c_uint32}
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            t, name = decl.split()
            arr = re.fullmatch(r"(\w+)\[(\d+)\]", name)
            fields.append((arr.group(1), ctype[t] * int(arr.group(2))))
    assert fields == [(n, t) for n, t in ca.CrProbeGrid._fields_]
    size = C.c_uint32(0)
    hip.cr_probe_struct_sizes(C.byref(size))
    assert size.value == C.sizeof(ca.CrProbeGrid) == 36
    hip.cr_probe_struct_sizes(None)
    assert (ca.CrProbeGrid.step.offset, ca.CrProbeGrid.dims.offset) == (12, 24)
    g = ca.probe_grid((0.5, 1, 2), (0.25, 1, 3), (4, 3, 2))
    assert g.count == 24 and list(g.dims) == [4, 3, 2] and list(g.origin) == [0.5, 1.0, 2.0]


GRIDS = [((0.25, -1.0, 2.0), (1.0, 1.0, 1.0), (1, 1, 1)), ((-1.5, 0.5, 0.0), (0.75, 3.0, 0.3), (2, 1, 3)),
         ((0.1, -0.2, 0.3), (0.37, 0.5, 1.25), (4, 3, 2))]
BAD_GRIDS = [((0, 0, 0), (1, 1, 1), (0, 3, 2)), ((0, 0, 0), (1, 1, 1), (4, 3, 0)), ((0, 0, 0), (1, 1, 1), (65536, 65536, 1)),
             ((float("nan"), 0, 0), (1, 1, 1), (4, 3, 2)), ((0, float("inf"), 0), (1, 1, 1), (4, 3, 2)),
             ((0, 0, 0), (1, 0, 1), (4, 3, 2)), ((0, 0, 0), (1, 1, -1), (4, 3, 2)),
             ((0, 0, 0), (float("inf"), 1, 1), (4, 3, 2)), ((0, 0, 0), (1, float("nan"), 1), (4, 3, 2))]


def test_grid_positions_need_no_device(ca):
    hip, _ = ca.libs()
    for origin, step, dims in GRIDS:
        got = ca.probe_grid_positions(ca.probe_grid(origin, step, dims))
        want = pm.grid_positions(origin, step, dims)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), dims
    # an axis of one probe does not read its step
    g = ca.probe_grid((1, 2, 3), (0.0, 0.5, -1), (1, 2, 1))
    assert np.array_equal(ca.probe_grid_positions(g), np.array([[1, 2, 3], [1, 2.5, 3]], F32))
    out = np.zeros((24, 3), F32)
    for origin, step, dims in BAD_GRIDS:
        g = ca.probe_grid(origin, step, dims)
        assert hip.cr_probe_grid_positions(C.byref(g), out.ctypes.data_as(FP)) == CR_E_INVALID, (origin, step, dims)
    g = ca.probe_grid(*GRIDS[2])
    assert hip.cr_probe_grid_positions(None, out.ctypes.data_as(FP)) == CR_E_INVALID
    assert hip.cr_probe_grid_positions(C.byref(g), None) == CR_E_INVALID
    with pytest.raises(RuntimeError):
        ca.probe_grid_positions(ca.probe_grid(*BAD_GRIDS[0]))


@pytest.fixture()
def ctx(ca):
    """A ctx without a device, with or without a GPU in the machine."""
    hip, _ = ca.libs()
    c = hip.cr_create(NO_DEVICE)
    assert c
    yield c
    hip.cr_destroy(c)


def _err(ca, c):
    return ca.libs()[0].cr_last_error(c).decode()


def _rp(ca, **kw):
    rp = ca.radiance_params(kw.pop("spp", 2), kw.pop("k", 3), 1, (0.1, 0.2, 0.3), layer=kw.pop("layer", 1),
                            id0=kw.pop("id0", 0))
    assert not kw
    return rp


def test_probe_sh_without_a_device(ca, ctx):
    hip, _ = ca.libs()
    P = C.c_void_p
    rp = _rp(ca)
    dev = lambda n=4, pos=FAKE, p=rp, nl=1, sh=FAKE: hip.cr_probe_sh_device(ctx, n, P(pos), C.byref(p) if p else None,
                                                                           nl, P(sh), None, None)
    assert dev() == CR_E_HIP and "device" in _err(ca, ctx)
    assert dev(n=0, pos=None, sh=None) == CR_E_HIP  # (the device before "nothing to do")
    for kw, part in ((dict(pos=None), "null"), (dict(sh=None), "null"), (dict(p=None), "params"), (dict(nl=0), "layers"),
                     (dict(p=_rp(ca, spp=0)), "spp"), (dict(p=_rp(ca, k=0)), "k must"), (dict(p=_rp(ca, k=65)), "k must"),
                     (dict(p=_rp(ca, layer=0)), "layer"), (dict(p=_rp(ca, id0=0xfffffffd)), "id0"),
                     (dict(p=_rp(ca, layer=0xffffffff), nl=2), "32 bits")):
        assert dev(**kw) == CR_E_INVALID, kw
        assert part in _err(ca, ctx), (kw, _err(ca, ctx))
    pos, sh = np.zeros((4, 3), F32), np.zeros((4, 27), F32)
    host = lambda n=4, a=pos, p=rp, nl=1, s=sh: hip.cr_probe_sh(ctx, n, a.ctypes.data_as(FP) if a is not None else None,
                                                               C.byref(p) if p else None, nl,
                                                               s.ctypes.data_as(FP) if s is not None else None, None)
    assert host() == CR_E_HIP
    for kw in (dict(a=None), dict(s=None), dict(p=None), dict(nl=0), dict(p=_rp(ca, spp=0)), dict(p=_rp(ca, id0=0xfffffffd))):
        assert host(**kw) == CR_E_INVALID, kw
    assert hip.cr_probe_sh_device(None, 4, P(FAKE), C.byref(rp), 1, P(FAKE), None, None) == CR_E_INVALID
    assert hip.cr_probe_sh(None, 4, pos.ctypes.data_as(FP), C.byref(rp), 1, sh.ctypes.data_as(FP), None) == CR_E_INVALID


def test_lookups_without_a_device(ca, ctx):
    hip, _ = ca.libs()
    P = C.c_void_p
    good = ca.probe_grid(*GRIDS[2])
    count = good.count
    ev = lambda m=8, sh=FAKE, probe=FAKE, nrm=FAKE, out=FAKE + (1 << 20): hip.cr_probe_eval_device(
        ctx, m, P(sh), P(probe), P(nrm), P(out), None)
    assert ev() == CR_E_HIP and ev(m=0, sh=None, probe=None, nrm=None, out=None) == CR_E_HIP
    for kw in (dict(sh=None), dict(probe=None), dict(nrm=None), dict(out=None)):
        assert ev(**kw) == CR_E_INVALID and "null" in _err(ca, ctx), kw
    assert ev(out=FAKE) == CR_E_INVALID and "alias" in _err(ca, ctx)
    assert ev(out=FAKE + 4) == CR_E_INVALID and ev(out=FAKE - 4) == CR_E_INVALID  # (inside the first probe / overlapping it)
    sm = lambda g=good, sh=FAKE, m=8, pos=FAKE, nrm=FAKE, out=FAKE + (1 << 20): hip.cr_probe_sample_device(
        ctx, C.byref(g) if g else None, P(sh), m, P(pos), P(nrm), P(out), None)
    assert sm() == CR_E_HIP and sm(m=0, sh=None, pos=None, nrm=None, out=None) == CR_E_HIP
    assert sm(g=None) == CR_E_INVALID and "grid" in _err(ca, ctx)
    for origin, step, dims in BAD_GRIDS:
        assert sm(g=ca.probe_grid(origin, step, dims)) == CR_E_INVALID, (origin, step, dims)
        assert sm(g=ca.probe_grid(origin, step, dims), m=0) == CR_E_INVALID  # (the grid is checked whatever m is)
    for kw in (dict(sh=None), dict(pos=None), dict(nrm=None), dict(out=None)):
        assert sm(**kw) == CR_E_INVALID and "null" in _err(ca, ctx), kw
    assert sm(out=FAKE) == CR_E_INVALID and "alias" in _err(ca, ctx)
    assert sm(out=FAKE + 27 * 4 * count - 4) == CR_E_INVALID and sm(out=FAKE + 27 * 4 * count) == CR_E_HIP
    # the host forms
    sh, nrm, out = np.zeros((count, 27), F32), np.zeros((8, 3), F32), np.zeros((8, 3), F32)
    probe = np.arange(8, dtype=np.uint32)
    f = lambda a: a.ctypes.data_as(FP)
    assert hip.cr_probe_eval(ctx, count, f(sh), 8, probe.ctypes.data_as(UP), f(nrm), f(out)) == CR_E_HIP
    assert hip.cr_probe_eval(ctx, count, None, 8, probe.ctypes.data_as(UP), f(nrm), f(out)) == CR_E_INVALID
    assert hip.cr_probe_eval(ctx, count, f(sh), 8, probe.ctypes.data_as(UP), f(nrm), f(sh)) == CR_E_INVALID
    assert hip.cr_probe_eval(ctx, 7, f(sh), 8, probe.ctypes.data_as(UP), f(nrm), f(out)) == CR_E_INVALID
    assert "index" in _err(ca, ctx)
    assert hip.cr_probe_sample(ctx, C.byref(good), f(sh), 8, f(nrm), f(nrm), f(out)) == CR_E_HIP
    assert hip.cr_probe_sample(ctx, None, f(sh), 8, f(nrm), f(nrm), f(out)) == CR_E_INVALID
    assert hip.cr_probe_sample(ctx, C.byref(good), f(sh), 8, None, f(nrm), f(out)) == CR_E_INVALID
    assert hip.cr_probe_sample(ctx, C.byref(ca.probe_grid(*BAD_GRIDS[5])), f(sh), 8, f(nrm), f(nrm), f(out)) == CR_E_INVALID
    # a null ctx
    assert hip.cr_probe_eval_device(None, 8, P(FAKE), P(FAKE), P(FAKE), P(FAKE + (1 << 20)), None) == CR_E_INVALID
    assert hip.cr_probe_sample_device(None, C.byref(good), P(FAKE), 8, P(FAKE), P(FAKE), P(FAKE + (1 << 20)), None) == CR_E_INVALID
    assert hip.cr_probe_eval(None, count, f(sh), 8, probe.ctypes.data_as(UP), f(nrm), f(out)) == CR_E_INVALID
    assert hip.cr_probe_sample(None, C.byref(good), f(sh), 8, f(nrm), f(nrm), f(out)) == CR_E_INVALID


def test_the_host_c_api_checks_its_pointers(ca):
    host = ca.libs()[1]
    out = np.zeros((4, 27), F32)
    g = ca.probe_grid(*GRIDS[0])
    assert host.chiaro_raytracer_probes(None, C.byref(g), None, 0, 1, out.ctypes.data_as(FP)) == CR_E_INVALID
    assert host.chiaro_raytracer_probes_sample(None, C.byref(g), out.ctypes.data_as(FP), out.ctypes.data_as(FP),
                                               out.ctypes.data_as(FP), 1, out.ctypes.data_as(FP)) == CR_E_INVALID
