"""Register use, spills and LDS of the device kernels in a built object (gfx950 code-object notes).
    python scripts/kernel_regs.py [chiaroscuro-raytracer_amd/build/wavefront.o] [name-filter]
    python scripts/kernel_regs.py --diff A.o B.o     the two objects' device code kernel by kernel: the notes
        (registers, spills, LDS, scratch, argument layout) and the instruction stream.  Every kernel is
        identical, equivalent (same notes, the same instructions in another order) or changed (with the deltas
        of registers, spills, scratch and instruction count); exit 1 on any difference"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def device_tool(obj, tool):
    """Output of an LLVM tool (a command line without its input) on the object's gfx950 code object."""
    with tempfile.TemporaryDirectory() as td:
        fat, dev = os.path.join(td, "fat"), os.path.join(td, "dev")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(td, "x")],
                       check=True, capture_output=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={dev}"], check=True,
                       capture_output=True)
        return subprocess.run([f"{LLVM}/{tool[0]}", *tool[1:], dev], check=True, capture_output=True,
                              text=True).stdout


def notes(obj):
    return device_tool(obj, ["llvm-readelf", "--notes"])


def kernels(obj):
    out = []
    for b in notes(obj).split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        get = lambda k: int((re.search(r"\." + k + r":\s+(\d+)", b) or [0, 0])[1])
        out.append({"name": name, "vgpr": get("vgpr_count"), "sgpr": get("sgpr_count"),
                    "vgpr_spill": get("vgpr_spill_count"), "sgpr_spill": get("sgpr_spill_count"),
                    "lds": get("group_segment_fixed_size"), "scratch": get("private_segment_fixed_size")})
    return out


def note_blocks(obj):
    """kernel name -> its whole metadata note (registers, spills, LDS, scratch and the argument list)."""
    out = {}
    for b in notes(obj).split("- .agpr_count")[1:]:
        b = b.split("amdhsa.target")[0]
        out[re.search(r"\.name:\s+(\S+)", b).group(1)] = b.strip()
    return out


def bodies(obj):
    """kernel name -> its instruction stream, addresses, comments and inter-kernel padding stripped."""
    out, cur = {}, None
    for line in device_tool(obj, ["llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr"]).splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and line.strip() != "...":  # ("...": zero padding up to the next symbol)
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return out


def opcode(ins):
    """An instruction's mnemonic; a label line (no operands, ends with ':') counts as itself."""
    return ins.split(None, 1)[0] if ins else ins


NOTE_KEYS = (("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("vspill", "vgpr_spill_count"),
             ("sspill", "sgpr_spill_count"), ("scratch", "private_segment_fixed_size"))


def classify(note_a, note_b, ins_a, ins_b):
    """One kernel of two objects, from its notes (text) and instruction lists:
    "identical"   same notes, same instruction stream;
    "equivalent"  same notes, same instruction count, same multiset of opcodes (a reordering);
    "changed"     anything else."""
    if note_a != note_b or not ins_a or not ins_b:
        return "changed"
    if ins_a == ins_b:
        return "identical"
    if len(ins_a) == len(ins_b) and sorted(map(opcode, ins_a)) == sorted(map(opcode, ins_b)):
        return "equivalent"
    return "changed"


def deltas(note_a, note_b, ins_a, ins_b):
    """B - A of the register, spill and scratch notes and of the instruction count."""
    get = lambda b, k: int((re.search(r"\." + k + r":\s+(\d+)", b) or [0, 0])[1])
    out = {n: get(note_b, k) - get(note_a, k) for n, k in NOTE_KEYS}
    out["instructions"] = len(ins_b or []) - len(ins_a or [])
    return out


def diff(a, b):
    """Prints the comparison of two objects' device code, every kernel classified (classify); the number of
    kernels that are not identical or are missing."""
    na, nb, ba, bb = note_blocks(a), note_blocks(b), bodies(a), bodies(b)
    count = {"identical": 0, "equivalent": 0, "changed": 0, "missing": 0}
    for name in sorted(set(na) | set(nb)):
        if name not in na or name not in nb:
            print("only in %s: %s" % ("A" if name in na else "B", name))
            count["missing"] += 1
            continue
        tier = classify(na[name], nb[name], ba.get(name), bb.get(name))
        count[tier] += 1
        if tier == "equivalent":
            print("equivalent: %s" % name)
        elif tier == "changed":
            d = deltas(na[name], nb[name], ba.get(name), bb.get(name))
            print("changed (%s): %s" % (" ".join("%s %+d" % kv for kv in d.items()), name))
    print("kernels A %d B %d, identical %d, equivalent %d, changed %d, missing %d" % (
        len(na), len(nb), count["identical"], count["equivalent"], count["changed"], count["missing"]))
    return count["equivalent"] + count["changed"] + count["missing"]


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        sys.exit(1 if diff(sys.argv[2], sys.argv[3]) else 0)
    obj = sys.argv[1] if len(sys.argv) > 1 else "chiaroscuro-raytracer_amd/build/wavefront.o"
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    for k in kernels(obj):
        if flt in k["name"]:
            print(f'{k["name"][:72]:72s} vgpr {k["vgpr"]:3d} sgpr {k["sgpr"]:3d} vspill {k["vgpr_spill"]:3d} '
                  f'sspill {k["sgpr_spill"]:3d} lds {k["lds"]:5d} scratch {k["scratch"]}')
