"""CPU checks of the trace builds' table and kernel selection (csrc/wfbuilds.hpp).

Every trace build is declared once there, and pure functions choose which kernel instantiation a launch
takes -- by build number, counting mode, eye_on_split, the fixed options, dead queue entries, wf_tail_waves
and wf_shade's options.  tests/native/wfbuilds_check.cpp walks the whole cross product on the host and
compares the chosen kernels, LDS ring depth, grid, cull level and leaf-cull form with expectations written
out as literal data, and requires that the kernels the selections can reach are exactly the ones the
kernel lists instantiate (37 wf_trace, 4 wf_trace_packet, 13 wf_tail, 9 wf_shade).
"""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "wfbuilds_check.cpp"
HDR = ROOT / "chiaroscuro-raytracer_amd" / "csrc" / "wfbuilds.hpp"


def _build(tmp_path, header_dirs):
    exe = tmp_path / "wfbuilds_check"
    cmd = ["g++", "-O1", "-std=c++17"]
    for d in header_dirs:
        cmd += ["-I", str(d)]
    subprocess.run(cmd + ["-o", str(exe), str(SRC)], check=True)
    return exe


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    m = re.search(r"checks (\d+) failures (\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    return int(m.group(1)), int(m.group(2)), r.stdout, r.returncode


def _patched(tmp_path, name, old, new):
    src = HDR.read_text()
    assert src.count(old) == 1, old
    d = tmp_path / name
    d.mkdir()
    (d / "wfbuilds.hpp").write_text(src.replace(old, new))
    sub = tmp_path / (name + "_exe")
    sub.mkdir()
    return _run(_build(sub, [d, HDR.parent]))


def test_every_selection(tmp_path):
    checks, failures, out, rc = _run(_build(tmp_path, [HDR.parent]))
    assert failures == 0 and rc == 0, out
    assert checks == 5025  # every case ran


def test_check_has_teeth(tmp_path):
    """The same program reports failures against a header with the fixed-options condition dropped (which also
    leaves the generic kernels of builds 44 and 59 unreachable), with
    build 59 counted through build 49's performed-work set, and with the 6-wave lean tail never chosen
    (which also leaves three wf_tail instantiations unreachable)."""
    _, failures, out, rc = _patched(tmp_path, "fixed", "return vis_mark == 1 && ended_only == 0u && lc_debug == 0;",
                                    "return true;")
    assert failures > 0 and rc != 0
    # (builds 44 and 59 then never launch their generic kernels: nothing reaches five of the six -- other builds
    # launch tc::ClosestFat)
    assert "closest kernel (44," in out and "shadow kernel (59," in out
    assert out.count("unreachable wf_trace instantiation") == 5

    _, failures, out, rc = _patched(tmp_path, "perf", "tc::PerfFatLc5Lx>(59)", "tc::PerfFatLc5>(59)")
    assert failures > 0 and rc != 0
    assert "closest kernel (59, 1," in out and "shadow kernel (59, 2," in out and "kernel (54," not in out

    _, failures, out, rc = _patched(tmp_path, "tail", "(lean_waves == 5 || lean_waves == 6)", "(lean_waves == 5)")
    assert failures > 0 and rc != 0
    assert "tail kernel (59, 0, 6)" in out and out.count("unreachable wf_tail instantiation") == 3
