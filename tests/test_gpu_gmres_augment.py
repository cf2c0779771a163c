"""gmres(..., augment=k) on the device against tests/lgmres_reference.py::lgmres_ref, and augment = 0 through the new `_aug` entry
points against the existing ones.

Operator of most tests: HelmholtzOperator on uniform_rect(8, ...), n_basis 4 (625 nodes, vectors of 1250 doubles), the case of
tests/test_gpu_gmres_cgs2.py.  Its dense matrix is obtained once by applying it to the unit vectors; the model runs on that matrix.
"""
import ctypes as C
import math

import numpy as np
import pytest

import blas1_reference as br
import lgmres_reference as lr
from test_gpu_gmres_cgs2 import M, MAXIT, NB, NX, Case, bitwise, distance, out_tuple, same_run

pytestmark = pytest.mark.gpu

K = 3  # corrections kept


class AugCase(Case):
    def model(self, tol, T=np.float64, orth="mgs"):
        """(x, info) of lgmres_ref with k = 3, computed once per (tol, type, orth); tol = 0 from x = 0, tol > 0 from the near start vector"""
        key = ("lgmres", tol, T, orth)
        if key not in self._ref:
            x0 = None if tol == 0 else self.x0h
            self._ref[key] = lr.lgmres_ref(self.Ad, self.bh, M, MAXIT if tol == 0 else 6, tol, K, T, x0=x0, orth=orth)
        return self._ref[key]


@pytest.fixture(scope="module")
def case(cuda):
    return AugCase(cuda)


# ================================================================== augment = 0 through the new entry points
def test_augment_zero_through_the_aug_entry_points_is_the_existing_path(case, monkeypatch):
    """every one of the five `_aug` entry points with orth = 0, augment = 0 against its counterpart: identical bits in x and res_norm,
    the same counts (Python stays on the existing entry points for augment = 0; here it is made to call the new ones)"""
    cd, torch, N = case.cd, case.torch, case.cd._native
    lib = N.lib
    seen = []

    def forced(name, code, head, res, h_res, h_time):
        seen.append(name + "_aug")
        return getattr(lib, name + "_aug")(*head, code, 0, C.byref(res), h_res.ctypes.data_as(C.c_void_p), h_time.ctypes.data_as(C.c_void_p))

    nd = case.fem.size()
    F = cd.DDH(2 * math.pi * NX / 10, np.ones(nd), case.fem, NX, NX)
    f = torch.zeros(2 * nd, dtype=torch.float64, device=case.dev)
    cd.linear_functional(case.fem, cd.GAUSSIANS, f[:nd], param=2 * math.pi * NX / 10)
    bl = torch.zeros(F.size(), dtype=torch.float32, device=case.dev)
    F.rhs(f, bl)
    wrapped = lambda p, q: case.A.action(p, q)  # noqa: E731

    def runs():
        got = {}
        x = torch.zeros_like(case.b)
        got["helmholtz"] = out_tuple(case.A.gmres(x, case.b, M, MAXIT, 0.0), x)
        x = torch.zeros_like(case.b)
        got["f64"] = out_tuple(cd.gmres(case.n, x, case.A, case.b, M, MAXIT, 0.0), x)
        x = torch.zeros_like(case.b)
        got["callback"] = out_tuple(cd.gmres(case.n, x, wrapped, case.b, M, MAXIT, 0.0), x)
        x = torch.zeros_like(case.b)
        got["sharded"] = out_tuple(cd.gmres(case.n, x, wrapped, case.b, M, MAXIT, 0.0, reduce=lambda t: None), x)
        x = torch.zeros_like(bl)
        got["ddh"] = out_tuple(cd.gmres(F.size(), x, F, bl, 10, 20, 1e-4), x)
        return got

    old = runs()
    assert not seen
    monkeypatch.setattr(cd.api, "_gmres_entry", forced)
    new = runs()
    assert sorted(set(seen)) == sorted(["cuddh_gmres_helmholtz_aug", "cuddh_gmres_f64_aug", "cuddh_gmres_callback_aug",
                                        "cuddh_gmres_callback_sharded_aug", "cuddh_gmres_ddh_aug"])
    for name in old:
        assert same_run(old[name], new[name]), name
        assert old[name][2] > 3


# ================================================================== augment = 3 against the model
def sensitivity(case, orth):
    """float64 run against longdouble run of the model, the longdouble results not rounded first: (of x, of res_norm)"""
    xr, ir = case.model(0.0, orth=orth)
    xl, il = case.model(0.0, np.longdouble, orth=orth)
    rl = np.asarray(il["res_norm_unrounded"], dtype=np.longdouble)
    sx = float(np.linalg.norm(xr.astype(np.longdouble) - xl) / np.linalg.norm(xl))
    sr = float(np.max(np.abs(np.asarray(ir["res_norm"]).astype(np.longdouble) - rl) / rl))
    assert sx > 0 and sr > 0
    return sx, sr


@pytest.mark.parametrize("orth", ["mgs", "cgs2"])
def test_augmented_against_the_model(case, orth):
    """GMRES(20), maxit 4, tol 0, augment = 3: num_matvec is the model's, 1 + 21 + 20 + 19 (the initial residual, then 20, 19 and 18
    Krylov columns and one true residual per cycle); x and res_norm agree with the model within 10 x the model's own sensitivity
    (float64 against longdouble on the same matrix; the factor 10, as in the CGS2 test, for the device's summation order).  Both
    distances are printed.  On MI355X (profiles/r18/gmres_augment_tests.txt): sensitivity 4.7e-16 (x) and 1.3e-16 (res_norm) under mgs,
    6.4e-16 and 1.3e-16 under cgs2; the device is 1.0e-15 / 5.2e-16 (mgs) and 1.2e-15 / 4.2e-16 (cgs2) from the model."""
    xr, ir = case.model(0.0, orth=orth)
    rr = np.asarray(ir["res_norm"])
    assert ir["num_matvec"] == 1 + 21 + 20 + 19 and ir["cycles"] == [(M, M), (M, M - 1), (M, M - 2)]
    sens = sensitivity(case, orth)
    for how in ("HelmholtzOperator.gmres", "gmres"):
        x = case.start(0.0)
        if how == "gmres":
            out = case.cd.gmres(case.n, x, case.A, case.b, M, MAXIT, 0.0, orth=orth, augment=K)
        else:
            out = case.A.gmres(x, case.b, M, MAXIT, 0.0, orth=orth, augment=K)
        got = distance(x.cpu().numpy(), np.asarray(out.res_norm), xr, rr) if len(out.res_norm) == len(rr) else (np.inf, np.inf)
        print(f"{how} orth={orth}: num_matvec {out.num_matvec} (model {ir['num_matvec']}); distance to the model: x {got[0]:.3e}, res_norm {got[1]:.3e}; "
              f"the model's sensitivity (float64 against longdouble): x {sens[0]:.3e}, res_norm {sens[1]:.3e}")
        assert out.num_matvec == ir["num_matvec"]
        assert len(out.res_norm) == len(rr) and not out.success and out.num_iter == ir["num_iter"]
        assert got[0] <= 10 * sens[0], f"{how}: x {got[0]:.3e} from the model, 10 x sensitivity = {10 * sens[0]:.3e}"
        assert got[1] <= 10 * sens[1], f"{how}: res_norm {got[1]:.3e} from the model, 10 x sensitivity = {10 * sens[1]:.3e}"


def test_a_counting_callable_sees_num_matvec_applications(case):
    count = [0]

    def op(p, q):
        count[0] += 1
        case.A.action(p, q)

    x = case.torch.zeros_like(case.b)
    out = case.cd.gmres(case.n, x, op, case.b, M, MAXIT, 0.0, augment=K)
    assert count[0] == out.num_matvec == 1 + 21 + 20 + 19


@pytest.mark.parametrize("orth", ["mgs", "cgs2"])
def test_ahead_path_equals_the_strict_path(case, orth):
    """the operator as a handle (driven one Arnoldi step ahead of the host; an augmentation column is a device copy and is queued
    ahead like an operator application) and wrapped in a Python callable (every step waits for its column): identical bits in x
    and res_norm, the same counts -- over three cycles, and with an exit in the middle of a cycle (the step queued ahead is
    discarded)"""
    cd, torch = case.cd, case.torch
    x1, x2 = torch.zeros_like(case.b), torch.zeros_like(case.b)
    o1 = cd.gmres(case.n, x1, case.A, case.b, M, MAXIT, 0.0, orth=orth, augment=K)
    o2 = cd.gmres(case.n, x2, lambda p, q: case.A.action(p, q), case.b, M, MAXIT, 0.0, orth=orth, augment=K)
    assert same_run(out_tuple(o1, x1), out_tuple(o2, x2)) and o1.num_matvec == 61
    # a short restart, so that augmentation columns are in play when the tolerance is met
    x1, x2 = torch.zeros_like(case.b), torch.zeros_like(case.b)
    o1 = cd.gmres(case.n, x1, case.A, case.b, 6, 40, 1e-3, orth=orth, augment=K)
    o2 = cd.gmres(case.n, x2, lambda p, q: case.A.action(p, q), case.b, 6, 40, 1e-3, orth=orth, augment=K)
    assert same_run(out_tuple(o1, x1), out_tuple(o2, x2))


def test_exit_in_the_middle_of_a_cycle_matches_the_model(case):
    """tol = 1e-6 from a start vector 8e-6 |b| away from the solution: the inner exit fires after a few columns of the first cycle;
    success, num_matvec, num_iter and len(res_norm) are the model's"""
    _, ir = case.model(1e-6)
    assert ir["success"] and len(ir["res_norm"]) == 2 and 4 < ir["num_matvec"] < M
    x = case.start(1e-6)
    out = case.A.gmres(x, case.b, M, 6, 1e-6, augment=K)
    print(f"num_matvec {out.num_matvec} (model {ir['num_matvec']}), res_norm {list(out.res_norm)} (model {ir['res_norm']})")
    assert bool(out.success) == ir["success"] and out.num_matvec == ir["num_matvec"] and len(out.res_norm) == len(ir["res_norm"])
    assert out.num_iter == ir["num_iter"]
    assert out.res_norm[-1] < 1e-6 * np.linalg.norm(case.bh)


# ================================================================== partitioned path with one rank
@pytest.mark.parametrize("orth", ["mgs", "cgs2"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_partitioned_path_with_one_rank(cuda, dtype, orth):
    """reduce= with a hook that sums over one rank (nothing to do) against the unpartitioned run on a diagonal operator (1003
    entries: no multiple of a 16-byte vector), GMRES(6) with augment = 2 over five cycles.  Under cgs2 both paths sum through the
    same routine and the runs are equal bit for bit; under mgs the partitioned path takes dot + axpy where the unpartitioned one
    takes the fused stages, so the counts are equal and the first residual norms agree to rounding (as without augmentation).  The hook
    sees one more scalar per cycle than without augmentation: |dx|^2."""
    import torch

    import cuddhelmholtz_amd as cd

    n, T = 1003, getattr(torch, "float64" if dtype == "f64" else "float32")
    d = torch.linspace(1.0, 3.0, n, dtype=T, device=cuda)
    b = torch.from_numpy(np.random.default_rng(5).standard_normal(n)).to(T).to(cuda)
    op = lambda p, q: torch.mul(d, p, out=q)  # noqa: E731
    calls = {0: [], 2: []}
    x1, x2, x3 = torch.zeros_like(b), torch.zeros_like(b), torch.zeros_like(b)
    o1 = cd.gmres(n, x1, op, b, 6, 6, 0.0, orth=orth, augment=2)
    o2 = cd.gmres(n, x2, op, b, 6, 6, 0.0, reduce=lambda t: calls[2].append(t.numel()), orth=orth, augment=2)
    cd.gmres(n, x3, op, b, 6, 6, 0.0, reduce=lambda t: calls[0].append(t.numel()), orth=orth)
    assert o1.num_matvec == o2.num_matvec == 1 + 7 + 6 + 5 + 5 + 5 and o1.num_iter == o2.num_iter
    if orth == "cgs2":
        assert same_run(out_tuple(o1, x1), out_tuple(o2, x2))
    else:
        assert np.allclose(o1.res_norm[:2], o2.res_norm[:2], rtol=1e-3 if dtype == "f32" else 1e-9, atol=0)
    assert len(calls[2]) == len(calls[0]) + 5 and set(calls[2]) == set(calls[0])
    xr, ir = lr.lgmres_ref(lambda v: d.cpu().numpy() * v, b.cpu().numpy(), 6, 6, 0.0, 2, br.NP[dtype], orth=orth)
    assert ir["num_matvec"] == o1.num_matvec
    assert np.allclose(o1.res_norm[:2], ir["res_norm"][:2], rtol=1e-3 if dtype == "f32" else 1e-9, atol=0)  # (later ones: rounding level in f32)


# ================================================================== breakdown
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_breakdown_ends_as_the_default_path(cuda, dtype):
    """A = identity, b = e_1: h[1] == 0 exactly after the first step.  The run ends as without augmentation (x = b exactly, three
    applications, residuals [1, 0]); it converged, so no pair was built -- the model says the same
    (test_lgmres_reference.py::test_model_breakdown_stores_no_pair)"""
    import torch

    import cuddhelmholtz_amd as cd

    n, T = 37, br.NP[dtype]
    bh = np.zeros(n, dtype=T)
    bh[0] = 1
    b = torch.from_numpy(bh).to(cuda)
    for reduce in (None, lambda t: None):
        runs = []
        for aug in (0, 2):
            x = torch.zeros_like(b)
            out = cd.gmres(n, x, lambda u, v: v.copy_(u), b, 5, 10, 1e-6, reduce=reduce, augment=aug)
            got = x.cpu().numpy()
            assert out.success and np.all(np.isfinite(got)) and bitwise(got, bh)
            assert out.num_matvec == 3 and list(out.res_norm) == [1.0, 0.0]
            runs.append(out_tuple(out, x))
        assert same_run(*runs)


# ================================================================== the trace system: augmentation pays
def test_augmentation_cuts_the_matvecs_on_the_trace_system(cuda):
    """lr.trace_system(16, 2, pi) (exact local solves, 8 x 8 subdomains, 3,136 real unknowns) as a dense torch matvec in fp64,
    GMRES(20), tol 1e-6, at most 60 cycles: both runs succeed, the augmented one with at most 0.75 x the plain run's operator
    applications (the model: 0.56), and the true residuals recomputed on the host are below 2e-6 |b|.  On MI355X: 551 and 309
    applications, 27 and 17 cycles -- the model's counts; recomputed residuals 9.9e-7 |b|."""
    import torch

    import cuddhelmholtz_amd as cd

    Ah, bh = lr.trace_system(*lr.TRACE_CASE)
    n = len(bh)
    A, b = torch.from_numpy(Ah).to(cuda), torch.from_numpy(bh).to(cuda)
    op = lambda p, q: torch.mv(A, p, out=q)  # noqa: E731
    outs = {}
    for aug in (0, K):
        x = torch.zeros_like(b)
        outs[aug] = cd.gmres(n, x, op, b, 20, 61, 1e-6, augment=aug)
        res = np.linalg.norm(bh - Ah @ x.cpu().numpy()) / np.linalg.norm(bh)
        print(f"augment={aug}: {outs[aug].num_matvec} matvecs, {outs[aug].num_iter} cycles, recomputed relative residual {res:.3e}")
        assert outs[aug].success and outs[aug].num_iter <= 60
        assert res < 2e-6
    assert outs[K].num_matvec <= 0.75 * outs[0].num_matvec


# ================================================================== fp32 DDH
def test_fp32_ddh_solve_with_augmentation(cuda):
    """cd.DDH on uniform_rect(8, ...), n_basis 4 (4 subdomains), fp32 traces: gmres(m = 10, maxit = 20, tol = 1e-4, augment = 2)
    succeeds, and |b - F x| recomputed through F.action agrees with res_norm[-1] to fp32 accuracy: the solver's norm is an fp32
    sum of squares and a square root (br.norm_bound), and the recomputed F x may differ from the solver's by the rounding of its
    entries where the action's summation order is not fixed (4 eps_32 |F x|)"""
    import torch

    import cuddhelmholtz_amd as cd

    omega, tol = 2 * math.pi * NX / 10, 1e-4
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(NX, -1.0, 1.0, NX, -1.0, 1.0), cd.Basis(NB))
    nd = fem.size()
    F = cd.DDH(omega, np.ones(nd), fem, NX, NX)
    assert F.info()["n_domains"] == 4 and F.trace_dtype == torch.float32
    f = torch.zeros(2 * nd, dtype=torch.float64, device=cuda)
    cd.linear_functional(fem, cd.GAUSSIANS, f[:nd], param=omega)
    b = torch.zeros(F.size(), dtype=torch.float32, device=cuda)
    F.rhs(f, b)
    x = torch.zeros_like(b)
    out = cd.gmres(F.size(), x, F, b, 10, 20, tol, augment=2)
    y = torch.zeros_like(b)
    F.action(x, y)
    bn = float(torch.linalg.norm(b.double()))
    res = float(torch.linalg.norm((b - y).double()))
    plain = cd.gmres(F.size(), torch.zeros_like(b), F, b, 10, 20, tol)
    print(f"fp32 DDH 8x8: augment=2 {out.num_matvec} matvecs, {out.num_iter} cycles (plain {plain.num_matvec}); recomputed residual {res / bn:.3e}, "
          f"res_norm[-1] {out.res_norm[-1] / bn:.3e}")
    assert out.success
    assert res < 2 * tol * bn
    yn = float(torch.linalg.norm(y.double()))
    assert abs(res - out.res_norm[-1]) <= br.norm_bound(F.size(), "f32", res) + 4 * float(np.finfo(np.float32).eps) * yn
