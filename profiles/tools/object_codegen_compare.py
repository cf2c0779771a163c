"""Are the kernels of two builds of an object file the same instructions?  Kernel by kernel, from the objects, without a GPU:

  python profiles/tools/object_codegen_compare.py OLD_DIR NEW_DIR wave_box.hip.o [wave_box_f32.hip.o ...]

For every named object in both directories: takes the gfx950 code object out of the fat binary (the llvm-objcopy and
clang-offload-bundler steps of kernel_registers.py), disassembles it (llvm-objdump -d) and compares the instruction text of every
kernel, operands and encodings included, addresses left out.  Kernels are matched by their demangled name without the argument
list, so a kernel whose argument types were renamed (StageArgs32 -> StageArgsT<float>) still meets itself; a kernel whose own
name changed is matched through --renamed OLD=NEW (demangled, without arguments; may be given more than once).  Prints one line per
object and one per kernel that differs or has no partner; exit status 1 if anything differs.
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def short(symbol):
    name = subprocess.run(["c++filt", symbol], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(anonymous namespace\)::|cuddh_k::wave::|cuddh_k::|void |\(.*$", "", name)


def kernels(obj):
    """demangled name -> the kernel's instructions, one string each"""
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([LLVM / "llvm-objcopy", "--dump-section", f".hip_fatbin={d}/fat.bin", obj], check=True)
        subprocess.run([LLVM / "clang-offload-bundler", "--unbundle", "--type=o", f"--input={d}/fat.bin", f"--output={d}/dev.co", f"--targets={TARGET}"],
                       check=True)
        text = subprocess.run([LLVM / "llvm-objdump", "-d", f"{d}/dev.co"], capture_output=True, text=True, check=True).stdout
    found = {}
    for block in re.split(r"\n(?=[0-9a-f]{16} <)", text)[1:]:
        head, *body = block.splitlines()
        symbol = re.match(r"[0-9a-f]{16} <(.*)>:", head).group(1)
        lines = []
        for ln in body:
            if not ln.strip():
                continue
            # "\tv_mov_b32 v0, 0   // 000000001000: 7E000280": the address goes, the encoding stays; a branch target is named by
            # its offset from the kernel's own symbol, which goes too
            ln = re.sub(r"// [0-9A-F]+:", "//", " ".join(ln.split()))
            lines.append(ln.replace(symbol, "KERNEL"))
        found[short(symbol)] = lines
    return found


def main():
    args = sys.argv[1:]
    renamed = {}
    while "--renamed" in args:
        i = args.index("--renamed")
        old, new = args[i + 1].split("=", 1)
        renamed[old] = new
        del args[i:i + 2]
    old_dir, new_dir, *objects = args
    differs = False
    for name in objects:
        old, new = kernels(Path(old_dir) / name), kernels(Path(new_dir) / name)
        bad = []
        for k, lines in old.items():
            partner = new.pop(renamed.get(k, k), None)
            if partner is None:
                bad.append(f"    {k}: MISSING in the new object")
            elif partner != lines:
                first = next((i for i, (a, b) in enumerate(zip(lines, partner)) if a != b), min(len(lines), len(partner)))
                bad.append(f"    {k}: DIFFERS, {len(lines)} -> {len(partner)} instructions, first at instruction {first}")
        bad += [f"    {k}: NEW in the new object" for k in new]
        n = sum(len(v) for v in old.values())
        print(f"{name}: {len(old)} kernels, {n} instructions: " + ("DIFFERENT" if bad else "identical kernel by kernel"))
        print("\n".join(bad), end="\n" if bad else "")
        differs = differs or bool(bad)
    sys.exit(1 if differs else 0)


if __name__ == "__main__":
    main()
