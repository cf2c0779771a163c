"""VGPRs, SGPRs, scratch and LDS of every kernel in a compiled object of the library, from the code object's metadata: no GPU.

  python profiles/tools/kernel_registers.py build/obj/wave_pair.hip.o [build/obj/wave_pair_f32.hip.o ...]

Takes the gfx950 code object out of the object file's fat binary (llvm-objcopy, clang-offload-bundler), reads the kernels' notes
(llvm-readelf --notes: .vgpr_count, .sgpr_count, .private_segment_fixed_size = scratch, .group_segment_fixed_size = LDS bytes) and
prints one line per kernel under its demangled, shortened name (profiles/r27/wave_pair_registers.txt was written this way).
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernels(obj):
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([LLVM / "llvm-objcopy", "--dump-section", f".hip_fatbin={d}/fat.bin", obj], check=True)
        subprocess.run([LLVM / "clang-offload-bundler", "--unbundle", "--type=o", f"--input={d}/fat.bin", f"--output={d}/dev.co", f"--targets={TARGET}"],
                       check=True)
        notes = subprocess.run([LLVM / "llvm-readelf", "--notes", f"{d}/dev.co"], capture_output=True, text=True, check=True).stdout
    rows = []
    for block in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        field = lambda key: re.search(rf"\.{key}:\s+(\S+)", block).group(1)  # noqa: E731
        name = subprocess.run(["c++filt", field("name")], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"\(anonymous namespace\)::|cuddh_k::wave::|cuddh_k::|void |\(.*$", "", name)
        name = re.sub(r"Pair(\w+)T<(float|double)>", r"\1", name)
        rows.append((name, int(field("vgpr_count")), int(field("sgpr_count")), int(field("private_segment_fixed_size")), int(field("group_segment_fixed_size"))))
    return sorted(rows)


for obj in sys.argv[1:]:
    rows = kernels(obj)
    print(f"== {Path(obj).name}")
    print(f"{'kernel':58s}  VGPR  SGPR  scratch     LDS")
    for name, vgpr, sgpr, scratch, lds in rows:
        print(f"{name:58s} {vgpr:5d} {sgpr:5d} {scratch:8d} {lds:7d}")
    print()
    print(f"{len(rows)} kernels; VGPR max {max(r[1] for r in rows)}, scratch max {max(r[3] for r in rows)}, LDS max {max(r[4] for r in rows)} bytes")
    print()
