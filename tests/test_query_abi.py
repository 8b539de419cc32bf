"""C-ABI surface of the device-resident ray queries (cr_intersect_device / cr_intersect_shadow_device):
declared in the header, exported by the library, listed by the Python binding, and loud about a missing
device.  What needs a GPU (results, stream order, the no-scene and null-pointer errors of a ctx that has a
device) is in tests/test_gpu_queries.py."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("cr_intersect_device", "cr_intersect_shadow_device")


def test_header_declares_and_library_exports(ca):
    text = (ROOT / "include" / "chiaro_hip.h").read_text()
    hip, _ = ca.libs()
    for name in NAMES:
        assert re.search(r"^int %s\(cr_ctx \*ctx, uint32_t n, const float \*d_orig, const float \*d_dir," % name,
                         text, re.M), name
        assert getattr(hip, name) is not None
    for opt in ("query_route", "query_sort", "query_chunk", "query_trace_min"):
        assert '"%s"' % opt in text, opt


def test_binding_lists_both(ca):
    for name in NAMES:
        assert name in ca.HIP_SYMBOLS
    for meth in ("intersect_device", "intersect_shadow_device", "intersect_tensors", "intersect_shadow_tensors"):
        assert callable(getattr(ca.Device, meth))


def _deviceless(hip):
    """A ctx without a device, on any machine: no GPU has this index."""
    c = hip.cr_create(1 << 20)
    assert c
    return c


def test_deviceless_ctx_reports_hip_error(ca):
    hip, _ = ca.libs()
    c = _deviceless(hip)
    try:
        buf = (ctypes.c_float * 16)()
        p = ctypes.cast(buf, ctypes.c_void_p)
        rc = hip.cr_intersect_device(c, 1, p, p, p, None, None, None, None)
        assert ca.CR_ERRORS.get(rc) == "CR_E_HIP"
        assert hip.cr_last_error(c)
        rc = hip.cr_intersect_shadow_device(c, 1, p, p, p, p, p, None)
        assert ca.CR_ERRORS.get(rc) == "CR_E_HIP"
        assert hip.cr_last_error(c)
        # the missing device is reported before anything else is looked at: n == 0 and null arrays too
        assert ca.CR_ERRORS.get(hip.cr_intersect_device(c, 0, None, None, None, None, None, None, None)) == "CR_E_HIP"
        # the four options exist without a device, and refuse values out of range
        for key, good, bad in ((b"query_route", 2, 3), (b"query_sort", -1, 2), (b"query_chunk", 1024, 100),
                               (b"query_trace_min", 0, -1)):
            assert hip.cr_set_option(c, key, good) == ca.CR_OK
            assert ca.CR_ERRORS.get(hip.cr_set_option(c, key, bad)) == "CR_E_INVALID"
    finally:
        hip.cr_destroy(c)


def test_null_ctx_is_invalid(ca):
    """Decided before any HIP call: a null ctx."""
    hip, _ = ca.libs()
    assert ca.CR_ERRORS.get(hip.cr_intersect_device(None, 1, None, None, None, None, None, None, None)) == "CR_E_INVALID"
    assert ca.CR_ERRORS.get(hip.cr_intersect_shadow_device(None, 1, None, None, None, None, None, None)) == "CR_E_INVALID"
