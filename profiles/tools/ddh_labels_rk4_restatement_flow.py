"""What the DDH flow reaches on label-built subdomains with RK4 local solves on per-subdomain time grids, on the CPU, with the
numpy restatement of tests/ddh_rk.py:
  python profiles/tools/ddh_labels_rk4_restatement_flow.py [wh_iters] [coarsen] [tol ...]        (defaults 12, 4 and 1e-10)
The problem is tests/ddh_labels_rk.case (the reference's unstructured square, 119 quads, n_basis 4, omega = 2 pi, 9 subdomains
from Morton labels, a = 0.4 / 0.5 / 1, `coefficient` ratios 1, 2, 3 on top of the coarsened base grid, fp64): rhs -> GMRES(100)
to tol -> postprocess of ddh_rk.Restatement in "rk4" mode, and the relative l2 distance of the result to
tests/ddh_general.fixed_point (DDH with exact local solves), one line per tol.  tests/test_gpu_ddh_labels_rk4.py gates the
product's flow at twice this distance.
The local solves are linear in the traces, so the operator is marched once, on all unit vectors as columns, and GMRES runs on
the matrix."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import ddh_general as dg  # noqa: E402
import ddh_labels_rk as lr  # noqa: E402
import ddh_rk as rk  # noqa: E402
import oracle  # noqa: E402


def main():
    wh = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    coarsen = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    c = lr.case()
    O = c.O["f64"]
    want = dg.fixed_point(O.t, O.G, c.d.ndof, c.f)
    n = O.size
    tols = [float(v) for v in sys.argv[3:]] or [1e-10]
    R = rk.Restatement(O, "rk4", c.ratios, coarsen, wh_iters=wh)
    eye = np.eye(n)
    out = R.solve_many([(c.f, None, False, True)] + [(None, eye[:, k], False, True) for k in range(n)])
    b = out[0][1]
    A = eye - np.stack([o[1] for o in out[1:]], axis=1)  # action(lam) = lam - update(lam)
    for tol in tols:
        lam, info = oracle.gmres(lambda v: A @ v, b, m=100, maxit=20, tol=tol)
        u = R.postprocess(lam, c.f)
        e = float(np.linalg.norm(u - want) / np.linalg.norm(want))
        print(f"rk4, coarsen {coarsen}, ratios {[int(r) for r in c.ratios]}, wh_iters {wh}: base grid nt {R.nt_base} (mesh grid {O.t.nt}), "
              f"{n} traces, GMRES(100) to {tol:g}: {info['num_matvec']} matvecs, success {info['success']}, distance to the "
              f"exact-local-solve fixed point {e:.4e}", flush=True)


if __name__ == "__main__":
    main()
