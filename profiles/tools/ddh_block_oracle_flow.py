"""What the oracle's own DDH flow reaches with subdomains of block x block elements, on the CPU:
  python profiles/tools/ddh_block_oracle_flow.py [nx] [block] [wh_iters]        (defaults 16 8 20)
a = 1, omega = 2 pi nx / 10 on [-1,1]^2, n_basis 4, fp64, the sources of tests/test_gpu_ddh_mfma_layout.case:
rhs -> GMRES(120) to 1e-6 -> postprocess of tests/ddh_general.OracleDDH, and the relative l2 distance of the result to
tests/ddh_general.fixed_point (DDH with exact local solves).  tests/test_gpu_ddh_block_size.py gates the product's flow at
twice this distance."""
import math
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import ddh_general as dg  # noqa: E402
import oracle  # noqa: E402


def main():
    nx, block, wh = (int(a) for a in (sys.argv[1:4] + ["16", "8", "20"][len(sys.argv) - 1:]))
    nb, omega = 4, 2 * math.pi * nx / 10
    d = oracle.Discretization(oracle.Mesh.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), nb)
    h_a = np.ones(d.ndof)
    f = np.concatenate([oracle.linear_functional(d, oracle.gaussians(omega)), 0.1 * oracle.linear_functional(d, oracle.mass_poly)])
    i, j = np.meshgrid(np.arange(nx), np.arange(nx), indexing="xy")
    labels = ((i // block) + (nx // block) * (j // block)).reshape(-1).astype(np.int32)
    n_domains = (nx // block) ** 2
    t = dg.tables(d.mesh, d.I, d.ndof, n_domains, labels, omega, h_a, d.gll_x, d.gll_w, oracle.basis_tables(nb, d.gll_x)[1],
                  d.metrics(d.gll_x)[1], np.float64)
    O = dg.OracleDDH(d, n_domains, labels, omega, h_a, np.float64)
    want = dg.fixed_point(t, O.G, d.ndof, f)
    oracle.ddh_set_wh_iters(wh)
    try:
        b = O.rhs(f)
        lam, info = oracle.gmres(O.action, b, m=120, maxit=30, tol=1e-6)
        u = O.postprocess(lam, f)
    finally:
        oracle.ddh_set_wh_iters(5)
    e = float(np.linalg.norm(u - want) / np.linalg.norm(want))
    print(f"nx {nx} block {block} wh_iters {wh}: nt {t.nt}, {info['num_matvec']} matvecs, success {info['success']}, "
          f"distance to the exact-local-solve fixed point {e:.4e}")


if __name__ == "__main__":
    main()
