"""Drop-in check: the reference's own example drivers compile UNCHANGED against the host mirror
(csrc/include/cuddh.hpp) and link against libcuddh_amd.so.  build() compiles them (oracle/ref_drivers.py) into
oracle/_ref/ where the reference tree is readable at build time; these tests check what it made, so they read nothing
outside the repository, and skip where the tree was absent (build/BUILD_INFO.json records which)."""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
EX = ROOT / "oracle" / "_ref"
LIB = ROOT / "cuddhelmholtz_amd" / "lib" / "libcuddh_amd.so"


def reference_was_present() -> bool:
    info = ROOT / "build" / "BUILD_INFO.json"
    if not info.exists():
        pytest.fail("build/BUILD_INFO.json missing: run __graft_entry__.build()")
    return bool(json.loads(info.read_text()).get("reference_tree_present"))


def check_driver(name):
    exe = EX / name
    if reference_was_present():
        assert exe.exists(), f"{exe} missing although build() saw the reference tree"
    elif not exe.exists():
        pytest.skip("reference tree not present at build time")
    assert LIB.exists()
    assert exe.read_bytes()[:4] == b"\x7fELF"
    dyn = subprocess.run(["readelf", "-d", str(exe)], capture_output=True, text=True)
    if dyn.returncode == 0:
        assert "libcuddh_amd.so" in dyn.stdout


@pytest.mark.parametrize("name", ["DDH", "Poisson", "Helmholtz"])
def test_reference_example_compiles_unchanged(name):
    check_driver(f"{name}_reference_driver")


def test_reference_test_suite_compiles_unchanged():
    """The reference's own tests (tests/test.cpp and the files it drives), compiled where they lie.  The binary the GPU
    test runs (tests/test_gpu_native_drivers.py::test_reference_test_suite_runs_unchanged) is built by build_examples()."""
    check_driver("reference_tests_driver")
