"""Recipe for the reference binaries of the drop-in checks -- TEST INFRASTRUCTURE, like the rest of oracle/.

Where the reference tree is readable at build time, its own examples/{DDH,Poisson,Helmholtz}.cpp and its test suite
(tests/test.cpp + quadrature_rule, basis, gmres, linalg, mass, stiffness and the text-mesh loader) are compiled UNCHANGED
against csrc/include/cuddh.hpp, linked against libcuddh_amd.so, into oracle/_ref/ (git-ignored; the binaries travel with
the tree, the reference's sources do not).  Where it is not, nothing is built and what an earlier build left is kept.
tests/test_dropin_build.py and tests/test_gpu_native_drivers.py use the binaries.
"""
from __future__ import annotations

import subprocess
from pathlib import Path

REF_OUT = Path(__file__).resolve().parent / "_ref"
EXAMPLES = ("DDH", "Poisson", "Helmholtz")


def build_reference_drivers(verbose: bool = False) -> list[Path]:
    from cuddhelmholtz_amd.build import ARCH, BUILD_LOG, CSRC, INCLUDES, LIB_DIR, LIB_PATH, REFERENCE_EXAMPLES, _present, hipcc, write_build_info

    jobs = []
    if _present(REFERENCE_EXAMPLES):
        jobs += [([REFERENCE_EXAMPLES / f"{n}.cpp"], f"{n}_reference_driver") for n in EXAMPLES]
    # the reference's OWN test suite, every file compiled where it lies; the mesh fixture it reads is the copy under
    # tests/golden/ (data)
    reference_tests = REFERENCE_EXAMPLES.parent / "tests"
    if _present(reference_tests):
        jobs.append((sorted(reference_tests.glob("*.cpp")), "reference_tests_driver"))
    if not jobs:
        return []
    REF_OUT.mkdir(parents=True, exist_ok=True)
    env_hdr = CSRC / "examples" / "reference_tests_env.hpp"
    outs = []
    for src, name in jobs:
        out = REF_OUT / name
        suite = name == "reference_tests_driver"
        deps = [f.stat().st_mtime for f in src] + [LIB_PATH.stat().st_mtime] + ([env_hdr.stat().st_mtime] if suite else [])
        if out.exists() and out.stat().st_mtime > max(deps):
            outs.append(out)
            BUILD_LOG["drivers_reused"].append(name)
            continue
        BUILD_LOG["drivers_built"].append(name)
        cmd = [hipcc(), "-O2", "-std=c++17", "-x", "hip", f"--offload-arch={ARCH}", "-munsafe-fp-atomics", *[f"-I{p}" for p in INCLUDES]]
        if suite:
            cmd += [f"-I{src[0].parent}",
                    # the reference reads `std::string dir = UNSTRUCTURED_SQUARE_MESH_DIR;` (tests/load_unstructured_square.cpp:13): the
                    # macro is an expression here, resolved at run time from the binary's own location (or CUDDH_MESH_DIR), so the
                    # driver works from any checkout path
                    "-include", str(env_hdr), "-DUNSTRUCTURED_SQUARE_MESH_DIR=cuddh_reference_mesh_dir()"]
        else:
            cmd += [f"-I{CSRC / 'examples'}", f"-I{REFERENCE_EXAMPLES}"]
        # oracle/_ref/<name> -> ../../cuddhelmholtz_amd/lib, as from build/examples/
        cmd += [*map(str, src), "-o", str(out), f"-L{LIB_DIR}", "-lcuddh_amd", "-Wl,-rpath,$ORIGIN/../../cuddhelmholtz_amd/lib"]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"building {name} failed:\n{r.stderr}")
        outs.append(out)
    write_build_info()
    return outs
