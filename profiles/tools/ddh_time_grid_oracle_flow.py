"""What the oracle's own DDH flow reaches with every subdomain on the time grid of its coefficient, on the CPU:
  python profiles/tools/ddh_time_grid_oracle_flow.py [wh_iters]        (default 20)
The problem is tests/ddh_time_grids.physics_case: 8 x 8 elements on [-1,1]^2, blocks of 4 x 4, n_basis 4, fp64, a from 0.4 to 1
across the domain (ratios 3, 2, 3, 2), omega = 2 pi nx / 10, the sources of tests/test_gpu_ddh_mfma_layout.case:
rhs -> GMRES(120) to 1e-6 -> postprocess of tests/ddh_time_grids.PerSubdomainOracle, and the relative l2 distance of the result
to tests/ddh_general.fixed_point (DDH with exact local solves).  tests/test_gpu_ddh_time_grids.py gates the product's flow at
twice this distance.  The same flow on the mesh grid is printed beside it."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import ddh_general as dg  # noqa: E402
import ddh_time_grids as tg  # noqa: E402
import oracle  # noqa: E402


def main():
    wh = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    d, omega, h_a, f, labels, n_domains, O, ratios = tg.physics_case()
    want = dg.fixed_point(O.t, O.G, d.ndof, f)
    oracle.ddh_set_wh_iters(wh)
    try:
        for name, P in (("per subdomain " + str([int(r) for r in ratios]), tg.PerSubdomainOracle(O, ratios)), ("mesh grid", O)):
            b = P.rhs(f)
            with np.errstate(all="ignore"):
                lam, info = oracle.gmres(P.action, b, m=120, maxit=30, tol=1e-6)
                u = P.postprocess(lam, f)
            e = float(np.linalg.norm(u - want) / np.linalg.norm(want))
            print(f"{name}, wh_iters {wh}: nt {O.t.nt}, {info['num_matvec']} matvecs, success {info['success']}, "
                  f"distance to the exact-local-solve fixed point {e:.4e}", flush=True)
    finally:
        oracle.ddh_set_wh_iters(5)


if __name__ == "__main__":
    main()
