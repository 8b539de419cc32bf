"""scripts/kernel_regs.py --diff: the three tiers a kernel of two objects falls into (identical, equivalent,
changed) -- the gate a refactor of the trace kernels is held to.

CPU only, and skipped where test_trace_args.py is: it reads build/wavefront.o with the ROCm LLVM tools.
"""
import os

import pytest

from test_trace_args import HAVE_TOOLS, OBJ, kernel_regs

pytestmark = pytest.mark.skipif(not os.path.exists(OBJ) or not HAVE_TOOLS,
                                reason="build/wavefront.o or the ROCm LLVM tools absent")


def test_object_against_itself_is_all_identical(capsys):
    assert kernel_regs.diff(OBJ, OBJ) == 0
    last = capsys.readouterr().out.strip().splitlines()[-1]
    n = len(kernel_regs.note_blocks(OBJ))
    assert n > 40 and last == "kernels A %d B %d, identical %d, equivalent 0, changed 0, missing 0" % (n, n, n)


def test_tiers_of_hand_made_instruction_lists():
    note = ".sgpr_count: 40\n.sgpr_spill_count: 2\n.vgpr_count: 64\n.vgpr_spill_count: 0\n.private_segment_fixed_size: 20"
    a = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mov_b32_e32 v1, v0", "v_add_u32_e32 v2, v1, v0", "s_endpgm"]
    swapped = [a[1], a[0], a[2], a[3]]
    assert kernel_regs.classify(note, note, a, list(a)) == "identical"
    assert kernel_regs.classify(note, note, a, swapped) == "equivalent"
    # another opcode at the same length, another length, other notes: changed
    assert kernel_regs.classify(note, note, a, [a[0], a[1], "v_sub_u32_e32 v2, v1, v0", a[3]]) == "changed"
    assert kernel_regs.classify(note, note, a, a + ["s_nop 0"]) == "changed"
    more = note.replace(".sgpr_spill_count: 2", ".sgpr_spill_count: 6")
    assert kernel_regs.classify(note, more, a, swapped) == "changed"
    assert kernel_regs.deltas(note, more, a, a + ["s_nop 0"]) == {
        "vgpr": 0, "sgpr": 0, "vspill": 0, "sspill": 4, "scratch": 0, "instructions": 1}
