"""CPU model check of the camera packet's unanimous kd steps (csrc/wavefront.hip wf_trace_packet,
DESIGN.md §3.2): tests/native/packet_unanimous_check.cpp restates the packet walk WITH the hull
proofs -- a step at which every active ray goes to the near child only, or every one to the far child
only, decided once per packet from the hull of the live rays' direction components and two bounds over
the active rays' intervals -- and compares, ray by ray, the sequence of (leaf, tmin, tmax) tests and
the answer with the per-ray recursion of kdtree.cpp:248-281.  Its inputs include fans whose hull
contains 0, components at the 2^-40 / 2^40 guard, ties tsp == tmax / tmin, quotients that underflow,
an eye one ulp from a split plane, dead and box-missed rays and stacks deeper than the bound storage.
(The GPU tests check the kernel itself: test_gpu_packet_unanimous.py.)
"""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "packet_unanimous_check.cpp"
KEYS = ("violations", "rays", "leaf_tests", "steps", "proven", "near", "far", "loose")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("packet_unanimous") / "packet_unanimous_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(out), str(SRC)], check=True)
    return out


def _run(exe, seed, cases, mutant=0):
    r = subprocess.run([str(exe), str(seed), str(cases), str(mutant)], capture_output=True, text=True, timeout=300)
    m = re.search(" ".join(k + r" (\d+)" for k in KEYS), r.stdout)
    assert m, r.stdout + r.stderr
    print(r.stdout.strip())
    return dict(zip(KEYS, (int(v) for v in m.groups())))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_unanimous_steps_equal_recursion(exe, seed):
    r = _run(exe, seed, 1500)
    assert r["rays"] > 150_000 and r["leaf_tests"] > 500_000
    assert r["violations"] == 0 and r["loose"] == 0
    # the share of level-steps decided once per packet; both kinds of proof occur
    print("proven share %.3f" % (r["proven"] / r["steps"]))
    assert r["proven"] > 0 and r["near"] > 0 and r["far"] > 0


@pytest.mark.parametrize("mutant", [1, 2, 3])
def test_unanimous_model_has_teeth(exe, mutant):
    """`<=` in the far-only proof (1: a ray with tsp == tmin == tmax is near-only) and bounds kept across a
    pop (3) send rays to the wrong child; a hull that takes in the dead slots' (0, 0, 1) (2) is no longer
    the live rays' hull -- its ends are no live ray's component."""
    r = _run(exe, 1, 600, mutant)
    assert (r["loose"] if mutant == 2 else r["violations"]) > 0
