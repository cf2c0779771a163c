"""kernel 5 and kernel 3 (fp32) against the fp64 oracle on tests/test_gpu_ddh_mfma_layout.py's cases, for whichever library is loaded"""
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import numpy as np
import torch

import cuddhelmholtz_amd as cd
import test_gpu_ddh_mfma_layout as T
from test_gpu_parity import rel

cd.use_torch_stream()
dev = torch.device("cuda:0")
print("library:", os.environ.get("CUDDH_AMD_LIBRARY_VARIANT", "libcuddh_amd.so"))
for nx in (8, 16):
    c = T.case(nx)
    ref = T.oracle_outputs(c)
    for k in (5, 3):
        _, _, out = T.entry_points(cd, torch, dev, nx, "f32", k, c)
        e = [rel(a, r) for a, r in zip(out, ref)]
        print(f"{nx}x{nx} a=1 kernel {k} vs fp64 oracle: rhs {e[0]:.4e} action {e[1]:.4e} postprocess {e[2]:.4e}")
