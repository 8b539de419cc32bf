"""Register use, spills and LDS of the device kernels in a built object (gfx950 code-object notes).
    python scripts/kernel_regs.py [chiaroscuro-raytracer_amd/build/wavefront.o] [name-filter]
    python scripts/kernel_regs.py --diff A.o B.o     the two objects' device code kernel by kernel: the notes
        (registers, spills, LDS, scratch, argument layout) and the instruction stream; exit 1 on any difference"""
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


def diff(a, b):
    """Prints the comparison of two objects' device code; the number of kernels that differ or are missing."""
    na, nb, ba, bb = note_blocks(a), note_blocks(b), bodies(a), bodies(b)
    bad = 0
    for name in sorted(set(na) | set(nb)):
        if name not in na or name not in nb:
            print("only in %s: %s" % ("A" if name in na else "B", name))
            bad += 1
        elif na[name] != nb[name] or ba.get(name) != bb.get(name) or not ba.get(name):
            what = [w for w, ne in (("notes", na[name] != nb[name]), ("instructions", ba.get(name) != bb.get(name))) if ne]
            print("differs (%s): %s" % (", ".join(what) or "no body", name))
            bad += 1
    same = len(set(na) & set(nb)) - sum(1 for n in set(na) & set(nb)
                                         if na[n] != nb[n] or ba.get(n) != bb.get(n) or not ba.get(n))
    print("kernels A %d B %d, identical notes and instructions %d, different or missing %d" % (len(na), len(nb), same, bad))
    return bad


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        sys.exit(1 if diff(sys.argv[2], sys.argv[3]) else 0)
    obj = sys.argv[1] if len(sys.argv) > 1 else "chiaroscuro-raytracer_amd/build/wavefront.o"
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    for k in kernels(obj):
        if flt in k["name"]:
            print(f'{k["name"][:72]:72s} vgpr {k["vgpr"]:3d} sgpr {k["sgpr"]:3d} vspill {k["vgpr_spill"]:3d} '
                  f'sspill {k["sgpr_spill"]:3d} lds {k["lds"]:5d} scratch {k["scratch"]}')
