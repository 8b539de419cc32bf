"""CPU check of the option table (csrc/ctxopts.hpp).

cr_set_option is one walk over a table {name, lo, hi, rule, field}.  tests/golden/options_parent.json holds what the
commit before the table did -- its chain of string compares, on a ctx without a device -- for every key and every
probe value (-2 .. 9, every 2^k and 2^k +- 1 up to k = 41, the ends of the 32-bit, timeout and 65536 ranges, the
number of trace builds and one less): the return code, and which option field changed to what.
tests/native/options_check.cpp asserts the same acceptance for every pair, that an accepted pair changes exactly the
field the parent changed, to the same value, and that a rejected pair changes nothing.
"""
import json
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "options_check.cpp"
CSRC = ROOT / "chiaroscuro-raytracer_amd" / "csrc"
HDR = CSRC / "ctxopts.hpp"
GOLDEN = ROOT / "tests" / "golden" / "options_parent.json"
SIDE = "wf_side_priority"  # the one option with a side effect: cabi.cpp, not the table


def _golden(tmp_path):
    golden = json.loads(GOLDEN.read_text())
    assert re.fullmatch(r"[0-9a-f]{40}", golden["parent"])
    lines = ["probes " + " ".join(str(v) for v in golden["probes"])]
    for k in golden["keys"]:
        lines.append("key %s %s " % (k["name"], k["field"]) + " ".join("%d:%d" % (v, s) for v, s in k["accepted"]))
    (tmp_path / "options.txt").write_text("\n".join(lines) + "\n")
    return tmp_path / "options.txt", golden


def _build(tmp_path, header_dirs):
    exe = tmp_path / "options_check"
    cmd = ["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__"]
    for d in list(header_dirs) + ["/opt/rocm/include", ROOT / "include", CSRC]:
        cmd += ["-I", str(d)]
    subprocess.run(cmd + ["-o", str(exe), str(SRC)], check=True)
    return exe


def _run(exe, cases):
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=120)
    m = re.search(r"keys (\d+) probes (\d+) checks (\d+) failures (\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    return [int(x) for x in m.groups()], r.stdout, r.returncode


def test_golden_covers_what_it_claims(tmp_path):
    _, golden = _golden(tmp_path)
    probes, nvar = set(golden["probes"]), golden["variants"]
    want = set(range(-2, 10)) | {(1 << k) + d for k in range(42) for d in (-1, 0, 1)}
    want |= {0xffffffff, 0x100000000, 3600000, 3600001, 65536, 65537, nvar - 1, nvar}
    assert probes == want and len(golden["probes"]) == len(probes) == 130
    keys = {k["name"]: k for k in golden["keys"]}
    assert len(keys) == len(golden["keys"]) == 48
    assert all(k["accepted"] for k in keys.values())  # every key has a value the parent took
    acc = lambda name: [v for v, _ in keys[name]["accepted"]]
    assert acc("variant") == sorted(v for v in probes if -1 <= v < nvar)
    assert acc("wf_shade_waves") == [6, 8] and acc("wf_shade_block") == [256, 512, 1024]
    assert acc("wf_app_chunk") == [0] + [1 << k for k in range(8, 17)]
    assert acc("wf_dir_res_shadow") == [0] + [1 << k for k in range(9)] and acc("wf_dir_res") == [1 << k for k in range(9)]
    assert max(acc("comm_timeout_ms")) == 3600000 and max(acc("sample_buf_bytes")) == 1 << 40
    assert dict(map(tuple, keys["wf_tail_min"]["accepted"]))[0xffffffff] == 0xffffffff
    assert golden[SIDE] == {"deviceless_CR_E_HIP": [0, 1]}
    header = (ROOT / "include" / "chiaro_hip.h").read_text()
    for name in list(keys) + [SIDE]:
        assert re.search(r'"%s"' % name, header), name


def test_table_equals_parent(tmp_path):
    cases, golden = _golden(tmp_path)
    (keys, probes, checks, failures), out, rc = _run(_build(tmp_path, []), cases)
    assert failures == 0 and rc == 0, out[-4000:]
    assert (keys, probes, checks) == (48, 130, 48 * 130 * 2)  # every pair: its acceptance, its fields
    names = re.search(r"^names (.*)$", out, re.M).group(1).split()
    assert names == [k["name"] for k in golden["keys"]]  # the table's keys are the parent chain's, in its order
    assert int(re.search(r"^variants (\d+)$", out, re.M).group(1)) == golden["variants"]


def test_check_has_teeth(tmp_path):
    """Built against a table whose "refill_camera" row ends at 65, the acceptance of (refill_camera, 65) differs from
    the parent's and nothing else does."""
    cases, _ = _golden(tmp_path)
    src = HDR.read_text()
    old = 'CR_OPT("refill_camera", 0, 64,'
    assert src.count(old) == 1
    (tmp_path / "hdr").mkdir()
    (tmp_path / "hdr" / "ctxopts.hpp").write_text(src.replace(old, old.replace("64", "65")))
    (_, _, _, failures), out, rc = _run(_build(tmp_path, [tmp_path / "hdr"]), cases)
    assert failures == 2 and rc != 0, out[:2000]
    assert "FAIL refill_camera 65 accepted: 1 != 0" in out and "FAIL refill_camera 65 fields: refill_camera 65 != " in out


def test_side_priority_without_a_device(ca, tmp_path):
    """The special case keeps the parent's answers on a ctx without a device: CR_E_HIP and no message for 0 and 1,
    CR_E_INVALID and the common message for any other value; a table key through the library is the table's."""
    _, golden = _golden(tmp_path)
    hip = ca.libs()[0]
    c = hip.cr_create(1 << 20)
    try:
        for v in golden["probes"]:
            before = hip.cr_last_error(c)
            rc = hip.cr_set_option(c, SIDE.encode(), v)
            if v in golden[SIDE]["deviceless_CR_E_HIP"]:
                assert rc == -2 and hip.cr_last_error(c) == before, v
            else:
                assert rc == -1 and hip.cr_last_error(c) == b"unknown option or value: " + SIDE.encode()
        assert hip.cr_set_option(c, b"refill", 64) == ca.CR_OK and hip.cr_set_option(c, b"refill", 65) == -1
        assert hip.cr_last_error(c) == b"unknown option or value: refill"
        assert hip.cr_set_option(c, b"no_such_option", 0) == -1
        assert hip.cr_set_option(c, None, 0) == -1 and hip.cr_set_option(None, b"refill", 0) == -1
    finally:
        hip.cr_destroy(c)
