"""CPU checks of the wavefront pass plan and the path-chunk layout (csrc/wfplan.hpp).

run_render (cabi.cpp) takes every size it allocates, every key width and every array's place inside a chunk's
buffer from one pure host function, wf_plan, and one list of arrays, wf_arrays.  A wrong size there is a
kernel writing past an array inside a 100 GB allocation, which the GPU parity tests notice only by luck, so
tests/native/wfplan_check.cpp runs the plan on the host:

* equal to the parent: tests/golden/wfplan_parent.json holds what the commit before the plan existed computed --
  its run_render lines, unchanged, in a throwaway program -- for 244 inputs: four scenes (36 / 20k / 261k
  triangles and one whose node count turns leaf keys off) x five frames and shares (80x45x4, 64x36x2 with two
  layers as rank 0 of 2, 1920x1080x128, 3840x2160x100 with sample chunks, one tile) x twelve option vectors
  (wf_paths, sample_buf_bytes, lanes, a 260 GB or 8 GB budget, wf_sort, wf_leaf_keys, wf_world_keys,
  wf_dir_res_shadow, wf_app_chunk, K), and each of the three refusals.  Every output and every offset must match;
* sound: offsets on multiples of 256 in the list's order, no overlap, room for the elements the WfArgs comments
  promise, the last array inside `need` <= `need_alloc`, wf_bytes_per_path an upper bound;
* the layers rule (cr_layers_per_pass) agrees with the plan: what it accepts is one sample chunk, one path chunk.
"""
import json
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "wfplan_check.cpp"
CSRC = ROOT / "chiaroscuro-raytracer_amd" / "csrc"
HDR = CSRC / "wfplan.hpp"
GOLDEN = ROOT / "tests" / "golden" / "wfplan_parent.json"


def _cases(tmp_path):
    """The golden cases as the check reads them: "name value" pairs, the refusal after a '|'."""
    golden = json.loads(GOLDEN.read_text())
    assert re.fullmatch(r"[0-9a-f]{40}", golden["parent"])
    lines = []
    for case in golden["cases"]:
        pairs = [("in." + k, v) for k, v in case["in"].items()]
        if "out" in case:
            out = dict(case["out"])
            pairs += [("off." + k, v) for k, v in out.pop("offsets").items()]
            pairs += [("gstack.%d" % i, v) for i, v in enumerate(out.pop("gstack"))]
            pairs += [("out." + k, v) for k, v in out.items()]
        else:
            pairs.append(("code", case["code"]))
        lines.append(" ".join("%s %d" % p for p in pairs) + " |" + case.get("refusal", ""))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    return path, golden["cases"]


def _build(tmp_path, header_dirs):
    exe = tmp_path / "wfplan_check"
    cmd = ["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__"]
    for d in list(header_dirs) + ["/opt/rocm/include", ROOT / "include", CSRC]:
        cmd += ["-I", str(d)]
    subprocess.run(cmd + ["-o", str(exe), str(SRC)], check=True)
    return exe


def _run(exe, cases):
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=120)
    m = re.search(r"checks (\d+) failures (\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    return int(m.group(1)), int(m.group(2)), r.stdout, r.returncode


def test_golden_covers_what_it_claims(tmp_path):
    _, cases = _cases(tmp_path)
    assert len(cases) == 244
    refusals = {c["refusal"] for c in cases if "refusal" in c}
    assert refusals == {"layers x spp too large", "layers per pass: the samples do not fit one buffer",
                        "stack-overflow area above 4 GiB"}
    plans = [c for c in cases if "out" in c]
    assert any(c["out"]["qspare"] for c in plans) and any(not c["out"]["qspare"] for c in plans)
    assert {c["out"]["dir_res"] for c in plans if c["in"]["n_nodes"] == 900001 and c["out"]["leaf_keys"]} == {64}
    assert not any(c["out"]["leaf_keys"] for c in plans if c["in"]["n_nodes"] > 100000000)
    assert any(c["out"]["P"] == 1 << 20 and c["in"]["path_cap"] // c["in"]["wf_lanes"] < 1 << 20 for c in plans)
    assert any(c["out"]["chunk"] % 16 == 0 and c["out"]["chunk"] < c["in"]["spp"] for c in plans)
    assert any(c["out"]["need_alloc"] > c["out"]["need"] for c in plans)
    assert any(c["in"]["path_cap"] == 2 ** 64 - 1 for c in plans)


CHECKS = 41509  # 244 cases: the parent's outputs, the soundness of every array, the layers rule for nl 1..4


def test_plan_equals_parent_and_layout_is_sound(tmp_path):
    cases, _ = _cases(tmp_path)
    checks, failures, out, rc = _run(_build(tmp_path, []), cases)
    assert failures == 0 and rc == 0, out[-4000:]
    assert "cases 244" in out
    assert checks == CHECKS  # every case ran every check


def test_check_has_teeth(tmp_path):
    """Built against a header whose sizes count P slots where they count Q, the room checks fail on a case with
    spare slots; with the leaf-key width bound loosened by one bit, parent equality fails on the 900k-node scene."""
    cases, _ = _cases(tmp_path)
    src = HDR.read_text()
    old_q = "const size_t Q = d.Q, P = d.P;"
    old_leaf = "while (pl.dres_l > 8 && leaf_width(pl.dres_l) > 32) pl.dres_l >>= 1;"
    assert src.count(old_q) == 1 and src.count(old_leaf) == 1
    for name, old, new, want in (
            ("p_for_q", old_q, old_q.replace("d.Q", "d.P", 1), r"FAIL case \d+ \[[^\]]* spare [^\]]*\] room: ray0 "),
            ("leaf_33", old_leaf, old_leaf.replace("> 32", "> 33"), r"FAIL case \d+ \[nodes=900001 [^\]]*\] parent: ")):
        d = tmp_path / name
        (d / "hdr").mkdir(parents=True)
        (d / "hdr" / "wfplan.hpp").write_text(src.replace(old, new))
        _, failures, out, rc = _run(_build(d, [d / "hdr"]), cases)
        assert failures > 0 and rc != 0, name
        assert re.search(want, out), (name, out[:2000])
