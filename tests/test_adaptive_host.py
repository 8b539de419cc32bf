"""CPU checks of the adaptive render's host plan (csrc/adaptive.hpp): tests/native/adaptive_check.cpp runs

* the check schedule -- checks at the multiples of check_every that are >= min_layers, and at max_layers -- for every
  min_layers <= max_layers <= 9 and check_every up to max_layers + 2 (so check_every > max_layers and
  min_layers == max_layers occur);
* the pass plan of a list render for list lengths 0, 1, 1023, 1024, 1025, 4097 and 70000 under path caps and sample
  buffers that force splits by list range, by layers and by both: every (entry, layer) exactly once with a pixel's
  layers ascending, and wf_layers_fit on every pass that is not the smallest there is;
* once more with an off-by-one range planted in every plan (-DMUTATE): the same check must then fail.
"""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "adaptive_check.cpp"
CSRC = ROOT / "chiaroscuro-raytracer_amd" / "csrc"


def _run(tmp_path, name, *defines):
    exe = tmp_path / name
    cmd = ["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", *defines]
    for d in ("/opt/rocm/include", ROOT / "include", CSRC):
        cmd += ["-I", str(d)]
    subprocess.run(cmd + ["-o", str(exe), str(SRC)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)


def test_schedule_and_plan(tmp_path):
    r = _run(tmp_path, "adaptive_check")
    assert r.returncode == 0 and "adaptive_check: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert int(re.search(r"schedule cases (\d+)", r.stdout).group(1)) > 300
    m = re.search(r"plans (\d+) whole (\d+) split_range (\d+) split_layers (\d+) split_both (\d+)", r.stdout)
    plans, whole, by_range, by_layers, both = (int(v) for v in m.groups())
    assert plans == 7 * 2 * 3 * 5 * 2 * 6 and min(whole, by_range, by_layers, both) > 0, m.group(0)


def test_the_check_has_teeth(tmp_path):
    """An off-by-one list range in a plan is caught: the mutated program fails, and says that an entry is short."""
    r = _run(tmp_path, "adaptive_check_mutated", "-DMUTATE")
    assert r.returncode == 1 and "failures" in r.stdout, r.stdout[-3000:]
    assert re.search(r"entry \d+ ends at layer|range at pass", r.stdout), r.stdout[-3000:]
    assert "FAIL got == want" not in r.stdout  # (the schedule is not what was mutated)
