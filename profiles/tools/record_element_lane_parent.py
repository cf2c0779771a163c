"""Records the fixtures of tests/test_gpu_ddh_element_lane_packed.py: rhs, action and postprocess of DDH kernel 5's
element-lane form on that module's cases (a) and (b), as the library in use computes them.  Run once on an MI355X with a
build of the commit BEFORE the packed time loop (CUDDH_AMD_LIBRARY_VARIANT names that library, profiles/tools/build_variant.py):
  python profiles/tools/record_element_lane_parent.py [OUT_DIR]     (default tests/golden/element_lane_parent)
The inputs come from fixed seeds and closed-form functions (the test module builds them again); the files hold outputs only."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import torch  # noqa: E402

import cuddhelmholtz_amd as cd  # noqa: E402
import test_gpu_ddh_element_lane_packed as T  # noqa: E402

out = Path(sys.argv[1]) if len(sys.argv) > 1 else T.FIXTURES
out.mkdir(parents=True, exist_ok=True)
assert torch.cuda.is_available()
cuda = torch.device("cuda:0")
cd.use_torch_stream()
from cuddhelmholtz_amd import _native  # noqa: E402

print("library:", _native.LIB_PATH)
cases = {"case_a": lambda: T.outputs_a(cd, torch, cuda), "case_b": lambda: T.outputs_b(torch, cuda, *T.plan_b(cd))}
for name, run in cases.items():
    first, again = run(), run()
    for nm, a, b in zip(T.NAMES, first, again):
        assert np.array_equal(a, b), (name, nm, "not reproducible from run to run")
        print(f"{name} {nm}: {a.dtype} {a.shape}, max |value| {np.abs(a).max():.6e}")
    np.savez(out / f"{name}.npz", **dict(zip(T.NAMES, first)))
    print("wrote", out / f"{name}.npz")
