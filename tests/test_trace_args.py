"""The trace kernels' registers and the kernel-argument offsets their device code assumes.

The default builds' trace kernels (wfbuilds.hpp tc::Fixed, builds 59 and 44) read what they need once per
query -- the queues, their counters and order, the result arrays -- from the kernel-argument segment at the
offsets KARG_W / KARG_G of csrc/kernels.hpp instead of holding it in scalar registers (or spill lanes of a
VGPR) across the traversal.  A wrong offset would be a wild pointer, so the offsets are compared here with
the argument metadata of the built code object, and the registers with the caps the change reached.

CPU only: reads the notes of build/wavefront.o (scripts/kernel_regs.py) and compiles a few lines of host
C++ against csrc/kernels.hpp for the header's own idea of the offsets.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_regs  # noqa: E402

PKG = os.path.join(ROOT, "chiaroscuro-raytracer_amd")
OBJ = os.path.join(PKG, "build", "wavefront.o")
HAVE_TOOLS = os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler"))
pytestmark = pytest.mark.skipif(not os.path.exists(OBJ) or not HAVE_TOOLS,
                                reason="build/wavefront.o or the ROCm LLVM tools absent")


@pytest.fixture(scope="module")
def notes():
    return kernel_regs.notes(OBJ)


@pytest.fixture(scope="module")
def regs():
    return {k["name"]: k for k in kernel_regs.kernels(OBJ)}


def one(regs, *parts):
    """The kernel whose mangled name holds every part."""
    hits = [k for n, k in regs.items() if all(p in n for p in parts)]
    assert len(hits) == 1, (parts, [k["name"] for k in hits])
    return hits[0]


# the fixed instantiations the default builds launch: mangled-name parts -> (SGPR spills, VGPR spills, scratch)
# at most.  Shadow and closest: what the compile-only experiment before the change had reached
# (23 / 0 / 0 and 9 / - / 32 B; the built kernels have 2 / 0 / 0 and 2 / 6 / 28 B).
# The camera packet and wf_shade keep their arguments in registers: point-of-use loads were built for both
# (packet 58 -> 10 SGPR spills, 36 -> 20 B; wf_shade 136 -> 78..101 SGPR spills, but 52 B or more of scratch
# in every form tried, against its cap of 28 B) and taken out again because the packet's launch time did not
# move (34.67 -> 34.76 ms) and wf_shade's gain (3.81 -> 3.70 ms of a 265 ms step) is below the bench's noise:
# DESIGN.md §3.17.  So for these two the caps are the parent's own figures -- no more spills or scratch than
# before -- not the "fewer than 58 / 136" a kept change would have had to show.
CAPS = [
    (("wf_trace", "FixedINS1_17ShadowFatLc5FdLxDE"), (23, 0, 0)),
    (("wf_trace", "FixedINS1_21ShadowFatLc5FdDeadLxDE"), (23, 0, 0)),
    (("wf_trace", "FixedINS1_16ClosestFatLc5LxDE"), (9, None, 32)),
    (("wf_trace_packetILi8ELi2ELb0ELb1E",), (58, None, 36)),
    (("wf_shadeILi8ELb0ELi1024E",), (136, None, 28)),
    (("wf_shadeILi8ELb1ELi1024E",), (141, None, 36)),
]


@pytest.mark.parametrize("parts,cap", CAPS, ids=[c[0][-1] for c in CAPS])
def test_default_kernels_within_register_caps(regs, parts, cap):
    k = one(regs, *parts)
    print(k)
    sspill, vspill, scratch = cap
    assert k["vgpr"] <= 64, k  # 8 waves per SIMD: the launch bounds' budget, unchanged
    assert k["sgpr_spill"] <= sspill, k
    if vspill is not None:
        assert k["vgpr_spill"] <= vspill, k
    assert k["scratch"] <= scratch, k


def test_fixed_instantiations_of_build_44_exist(regs):
    for cfg in ("10ClosestFatE", "11ShadowFatFdE", "15ShadowFatFdDeadE"):
        k = one(regs, "wf_trace", "FixedINS1_" + cfg)
        assert k["vgpr"] <= 64 and k["scratch"] <= 20, k


def header_offsets(tmp_path):
    """KARG_W, sizeof(WfArgs), KARG_G, sizeof(RenderArgs) as csrc/kernels.hpp states them."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if not cxx:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "karg.cpp"
    src.write_text('#include <cstdio>\n#include "kernels.hpp"\n'
                   'int main() { std::printf("%u %zu %u %zu\\n", (unsigned)cr::KARG_W, sizeof(cr::WfArgs), '
                   '(unsigned)cr::KARG_G, sizeof(cr::RenderArgs)); return 0; }\n')
    exe = tmp_path / "karg"
    subprocess.run([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    return [int(v) for v in out]


def kernel_args(notes):
    """name -> [(offset, size)] of the explicit (by_value) arguments of every kernel."""
    out = {}
    for b in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        args = re.findall(r"- \.offset:\s+(\d+)\s+\.size:\s+(\d+)\s+\.value_kind:\s+by_value", b)
        out[name] = [(int(o), int(s)) for o, s in args]
    return out


def test_assumed_argument_offsets_match_the_code_object(notes, tmp_path):
    karg_w, size_w, karg_g, size_a = header_offsets(tmp_path)
    checked = 0
    for name, args in kernel_args(notes).items():
        # every kernel launched with (RenderArgs, WfArgs, uint32_t): the mangled parameter list
        if not name.endswith("ENS_10RenderArgsENS_6WfArgsEj") and "10RenderArgsENS_6WfArgsEj" not in name:
            continue
        assert args == [(0, size_a), (karg_w, size_w), (karg_g, 4)], (name, args)
        checked += 1
    # the trace instantiations (reference, fat, leaf-cull, exchange, fixed, perf, count), packets, shade, resolve
    assert checked >= 40, checked
