"""Bits of small GMRES solves, for comparing two builds of the library (a refactor of the GMRES host code must not move one).
Run on an MI355X, once per build:
  python profiles/tools/gmres_bits.py record OUT.json [TREE]     TREE: the built checkout whose package is imported (default: this one)
  python profiles/tools/gmres_bits.py compare PARENT_1.json PARENT_2.json THIS.json
  rocprofv3 --kernel-trace -d DIR -- python profiles/tools/gmres_bits.py record OUT.json [TREE]      (no counters in the same run)
  python profiles/tools/gmres_bits.py launches DIR      length and SHA-256 of the ordered list of kernel names of that trace
`record` writes, per case, success, num_iter, num_matvec, the hex bits of every res_norm entry and a SHA-256 of the bytes of x
(`time` is left out).  `compare` lists the cases whose two parent runs differ as not repeatable and compares those on the three
integers only; every other case must be identical in THIS.json.  Callable-operator cases are built of element-wise torch operations,
so the operator itself repeats exactly: one of them not repeatable is an error.  Exit status 1 on any difference."""
import hashlib
import itertools
import json
import math
import sys
from pathlib import Path

M, MAXIT = 5, 4
NX_DDH, NB, BLOCK, OMEGA_DDH = 16, 4, 4, 3.2 * math.pi  # tests/test_gpu_gmres_complex.py
NX_SMALL = 8  # the 8 x 8-element mesh of smoke()


def record(out_path, tree):
    sys.path.insert(0, str(tree))
    import numpy as np
    import torch

    import cuddhelmholtz_amd as cd

    dev = torch.device("cuda:0")
    cd.use_torch_stream()
    cases = {}

    def vector(n, dtype, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return torch.randn(n, dtype=torch.float64, generator=g).to(dtype).to(dev)

    def keep(name, out, x):
        torch.cuda.synchronize()
        cases[name] = {"success": bool(out.success), "num_iter": int(out.num_iter), "num_matvec": int(out.num_matvec),
                       "res_norm": [float(r).hex() for r in out.res_norm],
                       "x_sha256": hashlib.sha256(x.detach().cpu().numpy().tobytes()).hexdigest()}

    def tridiagonal(n, dtype):
        """y = d x + l shift(x) + u shift(x), nonsymmetric and diagonally dominant"""
        i = torch.arange(n, dtype=torch.float64)
        d = (2.5 + 0.5 * torch.sin(i)).to(dtype).to(dev)
        lo = (-1.1 + 0.2 * torch.cos(2 * i)).to(dtype).to(dev)
        up = (-0.3 + 0.1 * torch.sin(3 * i)).to(dtype).to(dev)

        def apply(x, y):
            torch.mul(d, x, out=y)
            y[1:].addcmul_(lo[1:], x[:-1])
            y[:-1].addcmul_(up[:-1], x[1:])

        return apply

    # ---- a callable operator: every orthogonalisation, augmentation and reduce, a mid-cycle exit, the 16-byte rounding of ldv
    for dtype, n, tol, orth, aug, red in itertools.product((torch.float64, torch.float32), (37, 64), (0.0, 1e-3), ("mgs", "cgs2"), (0, 2), (False, True)):
        x = torch.zeros(n, dtype=dtype, device=dev)
        out = cd.gmres(n, x, tridiagonal(n, dtype), vector(n, dtype, 7), M, MAXIT, tol, orth=orth, augment=aug, reduce=(lambda t: None) if red else None)
        keep(f"callable {'f64' if dtype == torch.float64 else 'f32'} n={n} tol={tol:g} {orth} augment={aug} reduce={'one rank' if red else 'none'}", out, x)

    # ---- complex arithmetic: (T + 0.7 i) on [Re; Im], T the tridiagonal on each half
    for dtype, tol in itertools.product((torch.float64, torch.float32), (0.0, 1e-3)):
        n, h = 64, 32
        T = tridiagonal(h, dtype)

        def complex_apply(x, y, T=T, h=h):
            T(x[:h], y[:h])
            T(x[h:], y[h:])
            y[:h].add_(x[h:], alpha=-0.7)
            y[h:].add_(x[:h], alpha=0.7)

        x = torch.zeros(n, dtype=dtype, device=dev)
        out = cd.gmres(n, x, complex_apply, vector(n, dtype, 9), M, MAXIT, tol, arithmetic="complex")
        keep(f"callable complex {'f64' if dtype == torch.float64 else 'f32'} n={n} tol={tol:g}", out, x)

    # ---- breakdown: the identity, column 0 ends the cycle
    for arithmetic, n in (("real", 37), ("complex", 64)):
        x = torch.zeros(n, dtype=torch.float64, device=dev)
        out = cd.gmres(n, x, lambda p, q: q.copy_(p), vector(n, torch.float64, 11), M, MAXIT, 1e-3, arithmetic=arithmetic)
        keep(f"callable breakdown {arithmetic} n={n}", out, x)

    # ---- operators of the library on the 8 x 8-element mesh: preconditioned mass operator, HelmholtzOperator.gmres (one step ahead)
    mesh = cd.Mesh2D.uniform_rect(NX_SMALL, -1.0, 1.0, NX_SMALL, -1.0, 1.0)
    fem = cd.H1Space(mesh, cd.Basis(NB))
    nd = fem.size()
    coef = torch.from_numpy(1.0 + 0.5 * np.cos(np.arange(nd))).to(dev)
    for orth, aug in (("mgs", 0), ("cgs2", 0), ("mgs", 2)):
        x = torch.zeros(nd, dtype=torch.float64, device=dev)
        out = cd.gmres(nd, x, cd.MassMatrix(fem, coef), vector(nd, torch.float64, 13), M, MAXIT, 0.0, Precond=cd.DiagInvMassMatrix(fem), orth=orth, augment=aug)
        keep(f"mass, DiagInvMassMatrix {orth} augment={aug}", out, x)
    fs = cd.FaceSpace(fem, mesh.boundary_edges())
    omega = 2 * math.pi * NX_SMALL / 10
    A = cd.HelmholtzOperator(omega, torch.ones(nd, dtype=torch.float64, device=dev), torch.ones(fs.size(), dtype=torch.float64, device=dev), fem, fs)
    b = torch.zeros(2 * nd, dtype=torch.float64, device=dev)
    cd.linear_functional(fem, cd.GAUSSIANS, b[:nd], param=omega)
    for orth, aug in (("mgs", 0), ("cgs2", 0), ("mgs", 2)):
        x = torch.zeros_like(b)
        out = A.gmres(x, b, M, MAXIT, 0.0, orth=orth, augment=aug)
        keep(f"HelmholtzOperator.gmres native={A.has_native()} {orth} augment={aug}", out, x)
        x = torch.zeros_like(b)
        out = cd.gmres(2 * nd, x, A, b, M, MAXIT, 0.0, orth=orth, augment=aug)
        keep(f"gmres(HelmholtzOperator) {orth} augment={aug}", out, x)

    # ---- DDH, 16 x 16 elements in 4 x 4-element subdomains, both precisions, real and complex
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(NX_DDH, -1.0, 1.0, NX_DDH, -1.0, 1.0), cd.Basis(NB))
    nd = fem.size()
    f = torch.zeros(2 * nd, dtype=torch.float64, device=dev)
    cd.linear_functional(fem, cd.GAUSSIANS, f[:nd], param=OMEGA_DDH)
    for precision, arithmetic in itertools.product(("f64", "f32"), ("real", "complex")):
        F = cd.DDH(OMEGA_DDH, np.ones(nd), fem, NX_DDH, NX_DDH, precision=precision, block=BLOCK)
        b = torch.zeros(F.size(), dtype=F.trace_dtype, device=dev)
        F.rhs(f, b)
        x = torch.zeros_like(b)
        out = cd.gmres(F.size(), x, F, b, M, MAXIT, 0.0, arithmetic=arithmetic)
        keep(f"DDH {precision} {arithmetic}", out, x)

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(json.dumps(cases, indent=1) + "\n")
    print(f"{len(cases)} cases -> {out_path}")


def compare(parent_1, parent_2, this):
    p1, p2, t = (json.loads(Path(p).read_text()) for p in (parent_1, parent_2, this))
    integers = lambda c: (c["success"], c["num_iter"], c["num_matvec"])  # noqa: E731
    bad = []
    if not (p1.keys() == p2.keys() == t.keys()):
        bad.append("the three files hold different cases")
    not_repeatable = [name for name in p1 if p1[name] != p2.get(name)]
    for name in not_repeatable:
        print("not repeatable at the parent (compared on success, num_iter, num_matvec only):", name)
        if name.startswith("callable"):
            bad.append(f"{name}: a callable-operator case is not repeatable")
    for name, c in p1.items():
        if name not in t:
            continue
        same = integers(c) == integers(t[name]) if name in not_repeatable else c == t[name]
        if not same:
            bad.append(f"{name}: parent {c} this {t[name]}")
    print(f"{len(p1)} cases, {len(not_repeatable)} not repeatable, {len(bad)} differences")
    for line in bad:
        print("DIFFERENT:", line)
    return 1 if bad else 0


def launches(trace_dir):
    import csv
    import sqlite3

    dbs = sorted(Path(trace_dir).rglob("*.db"))
    if dbs:
        names = [r[0] for r in sqlite3.connect(dbs[-1]).execute("select name from kernels order by start").fetchall()]
    else:  # a rocprofv3 that writes CSV
        with open(sorted(Path(trace_dir).rglob("*kernel_trace.csv"))[-1], newline="") as f:
            names = [r["Kernel_Name"] for r in sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))]
    print(f"{len(names)} launches, SHA-256 of the ordered names {hashlib.sha256(chr(10).join(names).encode()).hexdigest()}")
    Path(trace_dir, "kernel_names.txt").write_text("\n".join(names) + "\n")


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "record":
        record(sys.argv[2], Path(sys.argv[3]).resolve() if len(sys.argv) > 3 else Path(__file__).resolve().parents[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    elif len(sys.argv) == 3 and sys.argv[1] == "launches":
        launches(sys.argv[2])
    else:
        sys.exit(__doc__)
