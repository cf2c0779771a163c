"""Records what tests/test_gpu_ddh_element_lane_head.py::test_head_1_is_the_march_as_it_was compares head 1 with: the local traces
of kernel 5's element-lane form forced to (form, 2, 2, 2), form 2 and 3, at 8 x 8 elements (tests/test_gpu_ddh_mfma_layout.case(8)),
sources only, traces only and both, as the library of the commit BEFORE the head attribute gives them on an MI355X.
usage: record_element_lane_head_parent.py PARENT_TREE [OUT.npz]
PARENT_TREE: a checkout of that commit with its library built; its package is imported, this tree's tests supply the inputs.
Writes tests/golden/ddh_head/march2_before_8x8.npz (float32 arrays form{2,3}_{0,1,2}), or OUT.npz."""
import sys
from pathlib import Path

import numpy as np
import torch

root = Path(__file__).resolve().parents[2]
parent = Path(sys.argv[1]).resolve()
sys.path[:0] = [str(parent), str(root / "tests")]
import cuddhelmholtz_amd as cd  # noqa: E402

assert Path(cd.__file__).resolve().is_relative_to(parent), cd.__file__
assert not hasattr(cd.DDH, "set_head"), "the parent is the commit before the attribute"
import test_gpu_ddh_element_lane as E  # noqa: E402
import test_gpu_ddh_element_lane_forcing as FO  # noqa: E402
import test_gpu_ddh_mfma_layout as L  # noqa: E402
from test_gpu_parity import to_dev  # noqa: E402

cuda = torch.device("cuda:0")
cd.use_torch_stream()
nx = 8
c = L.case(nx)
f = to_dev(torch, c[3], cuda)
lam = to_dev(torch, c[5].astype(np.float32), cuda)
out = {}
for form in (2, 3):
    F, _ = E.make(cd, nx, form)
    F.set_chain_order(2)
    F.set_forcing(2)
    F.set_march(2)
    assert (F.sweep_form(), F.chain_order(), F.forcing(), F.march()) == (form, 2, 2, 2)
    for i, t in enumerate(FO._traces(torch, cuda, F, f, lam)):
        out[f"form{form}_{i}"] = t.cpu().numpy()
        assert out[f"form{form}_{i}"].dtype == np.float32
for i in range(3):
    assert np.array_equal(out[f"form2_{i}"], out[f"form3_{i}"])  # the owner rule
dst = Path(sys.argv[2]) if len(sys.argv) > 2 else root / "tests" / "golden" / "ddh_head" / "march2_before_8x8.npz"
dst.parent.mkdir(parents=True, exist_ok=True)
np.savez_compressed(dst, **out)
print("wrote", dst, {k: (v.shape, float(np.abs(v).max())) for k, v in out.items()})
