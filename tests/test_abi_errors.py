"""The order of the checks at every C-ABI entry point, without a GPU.

Every function of libchiaro_hip that takes a cr_ctx * or a cr_group * (and cr_tiles_for_rank / cr_tile_origin) is
called with a null handle and with a handle that has no device -- cr_create(1 << 20), a group over that device --
first with complete arguments, then with each pointer argument nulled in turn, then with each count or size
argument set to 0.  The return code and the handle's last error must equal tests/golden/abi_errors_parent.json:
what the library of the commit before crx::enter answered.  That pins which check comes first at each entry point:
the device for the older ones, the arguments for the noise entries ("C-ABI host layer").

Host pointers are real small buffers, device pointers a fake non-null value: neither handle can reach them.  The
message of the failed cr_create itself depends on the machine ("no HIP device" here, "bad device index" beside a
GPU), so it is recorded as <create>.
"""
import ctypes as C
import json
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "abi_errors_parent.json"
FAKE = 0x1000  # a non-null "device pointer": no call below may get as far as touching it
NO_DEVICE = 1 << 20


def _specs(ca):
    """name -> (handle kind, [(kind, value)]): kind "h" the handle, "p" a pointer (nulled in turn), "n" a count or
    size (zeroed in turn), "v" any other value."""
    f32 = lambda n: ("p", (C.c_float * n)())
    u32 = lambda n: ("p", (C.c_uint32 * n)())
    u64 = lambda n: ("p", (C.c_uint64 * n)())
    u8 = lambda n: ("p", (C.c_uint8 * n)())
    cam = lambda: ("p", C.pointer(ca.CrCamera()))
    par = lambda: ("p", C.pointer(ca.render_params(8, 8, 2, 3, 1)))
    dev, stream, h = ("p", FAKE), ("v", None), ("h", None)
    n = lambda v: ("n", v)
    desc = ("p", C.pointer(ca.CrSceneDesc()))
    tm = ("p", C.pointer(ca.CrTonemapParams(1, 1, 1, 1, 0, 2.2)))
    nparams = lambda: ("p", C.pointer(ca.CrNoiseParams(0.05, 0.01)))
    nstats = lambda: ("p", C.pointer(ca.CrNoiseStats()))
    ctx = {
        "cr_last_error": [h],
        "cr_upload_scene": [h, desc],
        "cr_render": [h, cam(), par(), f32(192)],
        "cr_render_device": [h, cam(), par(), dev, stream],
        "cr_render_tiles_device": [h, cam(), par(), dev, stream],
        "cr_blend_tiles_device": [h, par(), dev, dev, stream],
        "cr_intersect": [h, n(4), f32(12), f32(12), u32(4), u32(4), f32(8), f32(4)],
        "cr_intersect_shadow": [h, n(4), f32(12), f32(12), f32(4), u32(4), u32(4)],
        "cr_intersect_device": [h, n(4), dev, dev, dev, dev, dev, dev, stream],
        "cr_intersect_shadow_device": [h, n(4), dev, dev, dev, dev, dev, stream],
        "cr_get_counters": [h, ("p", C.pointer(ca.CrCounters()))],
        "cr_last_kernel_ms": [h],
        "cr_get_trace_stats": [h, ("p", C.pointer(ca.CrTraceStats()))],
        "cr_set_option": [h, ("p", C.c_char_p(b"refill")), ("v", 48)],
        "cr_synchronize": [h],
        "cr_get_diag": [h, u64(16), n(4)],
        "cr_get_perf": [h, u64(64), n(4)],
        "cr_last_trace_build": [h],
        "cr_tonemap_device": [h, tm, n(8), n(8), dev, dev, stream],
        "cr_tonemap": [h, tm, n(8), n(8), u8(192)],
        "cr_comm_init": [h, n(1), ("v", 0), u8(128)],
        "cr_comm_destroy": [h],
        "cr_render_dist_device": [h, cam(), par(), dev, stream],
        "cr_set_accumulator": [h, n(8), n(8), f32(192)],
        "cr_layers_per_pass": [h, par(), n(2)],
        "cr_render_layers_device": [h, cam(), par(), n(2), dev, stream],
        "cr_render_tiles_layers_device": [h, cam(), par(), n(2), dev, stream],
        "cr_render_layers": [h, cam(), par(), n(2), f32(192)],
        "cr_scene_triangles": [h],
        "cr_layers_per_group": [h, par(), n(2)],
        "cr_blend_tiles_layers_device": [h, par(), n(2), dev, dev, stream],
        "cr_render_dist_layers_device": [h, cam(), par(), n(2), dev, stream],
        "cr_render_layers_noise_device": [h, cam(), par(), n(2), dev, dev, stream],
        "cr_noise_device": [h, n(8), n(8), n(2), n(2), nparams(), dev, dev, dev, dev, stream],
        "cr_render_layers_noise": [h, cam(), par(), n(2), f32(192), f32(192)],
        "cr_noise": [h, n(8), n(8), n(2), n(2), nparams(), f32(64), nstats()],
        "cr_set_noise_accumulator": [h, n(8), n(8), f32(192)],
        "cr_render_until": [h, cam(), par(), n(1), n(4), n(2), nparams(), n(3), f32(192), nstats()],
    }
    group = {
        "cr_group_last_error": [h],
        "cr_group_size": [h],
        "cr_group_ok": [h],
        "cr_group_upload_scene": [h, desc],
        "cr_group_set_option": [h, ("p", C.c_char_p(b"refill")), ("v", 48)],
        "cr_group_render": [h, cam(), par(), f32(192)],
        "cr_group_get_counters": [h, ("p", C.pointer(ca.CrCounters()))],
        "cr_group_rank_ms": [h, f32(4)],
        "cr_group_ctx": [h, ("v", 0)],
        "cr_group_tonemap": [h, tm, n(8), n(8), u8(192)],
        "cr_group_set_accumulator": [h, n(8), n(8), f32(192)],
        "cr_group_render_layers": [h, cam(), par(), n(2), f32(192)],
    }
    free = {
        "cr_tiles_for_rank": [par(), ("v", 0)],
        "cr_tile_origin": [par(), ("v", 0), ("v", 0), u32(1), u32(1)],
    }
    specs = {k: ("ctx", v) for k, v in ctx.items()}
    specs.update({k: ("group", v) for k, v in group.items()})
    specs.update({k: ("none", v) for k, v in free.items()})
    return specs


def _variants(spec):
    """(label, which argument is nulled or zeroed) of one function: complete first."""
    yield "complete", None
    for kind, label in (("p", "null"), ("n", "zero")):
        for i, (k, _) in enumerate(spec):
            if k == kind:
                yield "%s %d" % (label, i), i


def _text(b, created):
    s = (b or b"").decode()
    return s.replace(created, "<create>") if created else s


def record(ca):
    """{function: {handle: [[variant, return value, last error], ...]}} of the loaded library."""
    hip = ca.libs()[0]
    probe = hip.cr_create(NO_DEVICE)
    created = hip.cr_last_error(probe).decode()
    hip.cr_destroy(probe)
    assert created in ("no HIP device", "bad device index")
    out = {}
    for name, (hkind, spec) in _specs(ca).items():
        fn = getattr(hip, name)
        handles = {"ctx": ("null", "deviceless"), "group": ("null", "deviceless"), "none": ("none",)}[hkind]
        out[name] = {}
        for handle in handles:
            rows = []
            for label, which in _variants(spec):
                c = None  # a fresh handle per call: the last error is this call's
                if handle == "deviceless":
                    c = hip.cr_create(NO_DEVICE) if hkind == "ctx" else \
                        hip.cr_group_create(1, (C.c_int * 1)(NO_DEVICE))
                args = [c if k == "h" else (None if k == "p" else 0) if i == which else v
                        for i, (k, v) in enumerate(spec)]
                rv = fn(*args)
                if isinstance(rv, bytes):
                    rv = _text(rv, created)
                elif fn.restype is ca.P:
                    rv = bool(rv)
                err = ""
                if c is not None:
                    err = _text((hip.cr_last_error if hkind == "ctx" else hip.cr_group_last_error)(c), created)
                    (hip.cr_destroy if hkind == "ctx" else hip.cr_group_destroy)(c)
                rows.append([label, rv, err])
            out[name][handle] = rows
    return out


def test_golden_covers_every_handle_function(ca):
    golden = json.loads(GOLDEN.read_text())
    assert re.fullmatch(r"[0-9a-f]{40}", golden["parent"])
    hip = ca.libs()[0]
    takes_handle = {n for n in ca.HIP_SYMBOLS
                    if getattr(hip, n).argtypes and getattr(hip, n).argtypes[0] is ca.P
                    and n not in ("cr_destroy", "cr_group_destroy")}
    assert takes_handle | {"cr_tiles_for_rank", "cr_tile_origin"} == set(golden["calls"]) == set(_specs(ca))
    for name, (hkind, spec) in _specs(ca).items():
        assert len(spec) == len(getattr(hip, name).argtypes), name
        nvar = len(list(_variants(spec)))
        assert all(len(rows) == nvar for rows in golden["calls"][name].values()), name
    # both conventions occur: the device first (cr_render), the arguments first (cr_noise)
    row = lambda name, label: [r for r in golden["calls"][name]["deviceless"] if r[0] == label][0]
    assert row("cr_render", "null 3")[1:] == [-2, "<create>"]
    assert row("cr_noise", "null 7")[1:] == [-1, "null stats"] and row("cr_noise", "complete")[1:] == [-2, "<create>"]


def test_every_entry_point_answers_as_the_parent(ca):
    golden = json.loads(GOLDEN.read_text())["calls"]
    got = json.loads(json.dumps(record(ca)))
    assert sum(len(rows) for f in got.values() for rows in f.values()) == 392  # no call skipped
    for name in golden:
        for handle in golden[name]:
            for want, have in zip(golden[name][handle], got[name][handle]):
                assert want == have, (name, handle)
    assert got == golden

