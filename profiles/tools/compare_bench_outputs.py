"""Relative l2 differences between bench.py --dump-outputs directories, pair by pair, and how much of the norm of A v_k the
orthogonalisation removed (from hessenberg_column: |h| / h[k+1]), which is the factor by which a difference in A v_k grows
relative to the Krylov vector.      usage: compare_bench_outputs.py NAME=DIR NAME=DIR ..."""
import itertools
import sys
from pathlib import Path

import numpy as np

runs = {}
for arg in sys.argv[1:]:
    name, d = arg.split("=", 1)
    runs[name] = {k: np.load(Path(d) / f"{k}.npy").astype(np.float64) for k in ("krylov_vector", "hessenberg_column")}
    h = runs[name]["hessenberg_column"]
    print(f"{name}: hessenberg_column has {h.size} entries, |h| = {np.linalg.norm(h):.6e}, h[k+1] = {h[-1]:.6e}, |h| / h[k+1] = {np.linalg.norm(h) / abs(h[-1]):.1f}")
for a, b in itertools.combinations(runs, 2):
    for k in ("krylov_vector", "hessenberg_column"):
        x, y = runs[a][k], runs[b][k]
        print(f"{a} vs {b}: {k} ({x.size} entries) relative l2 difference {np.linalg.norm(x - y) / np.linalg.norm(y):.4e}")
