"""Records the fixtures of tests/test_gpu_ddh_element_lane_assembly.py: rhs, action and postprocess of DDH kernel 5's
element-lane form on that module's cases (i) and (ii) (one-hot traces, one Gaussian source), as the library in use computes
them.  Run once on an MI355X with a build of the commit BEFORE the write-masked assembly:
  git show PARENT:cuddhelmholtz_amd/csrc/kernels/ddh.hip > cuddhelmholtz_amd/csrc/kernels/ddh.hip   (in a checkout of its own)
  python profiles/tools/build_variant.py parent ddh.hip          (there; copy lib/libcuddh_amd_parent.so into this tree's lib/)
  CUDDH_AMD_LIBRARY_VARIANT=libcuddh_amd_parent.so python profiles/tools/record_element_lane_assembly_parent.py [OUT_DIR]
(default tests/golden/element_lane_assembly).  The inputs come from the plan's tables and closed-form functions (the test
module builds them again); the files hold outputs only.  Two runs must agree bitwise before a file is written."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import torch  # noqa: E402

import cuddhelmholtz_amd as cd  # noqa: E402
import test_gpu_ddh_element_lane_assembly as T  # noqa: E402

out = Path(sys.argv[1]) if len(sys.argv) > 1 else T.FIXTURES
out.mkdir(parents=True, exist_ok=True)
assert torch.cuda.is_available()
cuda = torch.device("cuda:0")
cd.use_torch_stream()
from cuddhelmholtz_amd import _native  # noqa: E402

print("library:", _native.LIB_PATH)
for name in T.MESHES:
    first, again = T.record(cd, torch, cuda, name), T.record(cd, torch, cuda, name)
    for nm, a, b in zip(T.NAMES, first, again):
        assert np.array_equal(a, b) and a.tobytes() == b.tobytes(), (name, nm, "not reproducible from run to run")
        assert np.isfinite(a).all() and np.abs(a).max() > 0, (name, nm)
        print(f"{name} {nm}: {a.dtype} {a.shape}, max |value| {np.abs(a).max():.6e}, {int(np.count_nonzero(a == 0))} exact zeros")
    np.savez(out / f"{name}.npz", **dict(zip(T.NAMES, first)))
    print("wrote", out / f"{name}.npz")
