"""What the DDH flow reaches with RK4 local solves on a coarser grid, on the CPU, with the numpy restatement of tests/ddh_rk.py:
  python profiles/tools/ddh_rk4_restatement_flow.py [wh_iters] [coarsen]        (defaults 20 and 4)
The problem is tests/ddh_time_grids.physics_case (8 x 8 elements on [-1,1]^2, blocks of 4 x 4, n_basis 4, fp64, a from 0.4 to 1,
`coefficient` ratios 3, 2, 3, 2 on top of the coarsened base grid): rhs -> GMRES(120) to 1e-6 -> postprocess of
ddh_rk.Restatement in "rk4" mode, and the relative l2 distance of the result to tests/ddh_general.fixed_point (DDH with exact
local solves).  tests/test_gpu_ddh_rk4.py gates the product's flow at twice this distance.  The same flow with "rk2" on the mesh
grid (the per-subdomain oracle's, profiles/tools/ddh_time_grid_oracle_flow.py) is printed beside it.
The local solves are linear in the traces, so the operator is marched once, on all unit vectors as columns, and GMRES runs on
the matrix."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import ddh_general as dg  # noqa: E402
import ddh_rk as rk  # noqa: E402
import ddh_time_grids as tg  # noqa: E402
import oracle  # noqa: E402


def main():
    wh = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    coarsen = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    d, omega, h_a, f, labels, n_domains, O, ratios = tg.physics_case()
    want = dg.fixed_point(O.t, O.G, d.ndof, f)
    n = O.size
    for scheme, c in (("rk4", coarsen), ("rk2", 1)):
        R = rk.Restatement(O, scheme, ratios, c, wh_iters=wh)
        eye = np.eye(n)
        out = R.solve_many([(f, None, False, True)] + [(None, eye[:, k], False, True) for k in range(n)])
        b = out[0][1]
        A = eye - np.stack([o[1] for o in out[1:]], axis=1)  # action(lam) = lam - update(lam)
        lam, info = oracle.gmres(lambda v: A @ v, b, m=120, maxit=30, tol=1e-6)
        u = R.postprocess(lam, f)
        e = float(np.linalg.norm(u - want) / np.linalg.norm(want))
        print(f"{scheme}, coarsen {c}, ratios {[int(r) for r in ratios]}, wh_iters {wh}: base grid nt {R.nt_base} (mesh grid {O.t.nt}), "
              f"{info['num_matvec']} matvecs, success {info['success']}, distance to the exact-local-solve fixed point {e:.4e}", flush=True)


if __name__ == "__main__":
    main()
