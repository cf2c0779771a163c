"""DDH kernels 5 and 8 with the element's nodes numbered by class (register 0 = element-interior nodes, 1 = xi-face nodes,
2 = eta-face nodes, 3 = corners).

The layout changes which lane and register holds a node, which lanes exchange values in the assembly, the order of K's rows
and columns, and which terms of the update a register computes (register 0: no H term, and no sources unless x is given).
A mistake in any of them is wrong by O(1).  Checked on the stable coefficient a = 1, where fp32 has digits:
  * kernel 5 (fp32) against the fp64 oracle for rhs (x given, no lambda), action (lambda, no x) and postprocess (both), and
    against kernel 3, which shares nothing with it but load_dof and publish_dof.  The bound is 2 x the distance the kernel 5 of
    the commit before this layout had to the same oracle on the same inputs (PARENT5, profiles/r07/kernel5_distances.txt):
    another equally valid summation order can land on either side of the old one, a layout bug cannot hide in a factor 2.
    Kernel 5 against kernel 3, measured in units of the oracle's norm, is bounded by the triangle inequality: 2 x PARENT5 plus
    kernel 3's own distance to the oracle (kernel 3 is not touched by the layout);
  * kernel 8 (fp64) against the oracle and kernel 2 at the fp64 gates of tests/test_gpu_ddh_fp64_mfma.py;
  * listed launches and launches that hold issue priority (the second form of that template parameter) are bitwise the plain
    launch, with and without x (both forms of the other one);
  * the guard: a descriptor in which an element-interior node is a trace dof is refused for kernels 5 and 8, and auto stays on
    kernel 3.  Nothing is launched on that table but the checks of plan_create.
Every distance is printed (`pytest -s`).
"""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu

# distance of the previous layout's kernel 5 to the fp64 oracle on case(nx), measured with that commit's library
# (profiles/r07/kernel5_distances.txt): nx -> (rhs, action, postprocess)
PARENT5 = {8: (1.1465e-06, 4.2275e-07, 1.0577e-06), 16: (7.9688e-07, 5.1238e-07, 1.1167e-06)}


def case(nx):
    """a = 1, the example's frequency and sources, traces drawn on the slots that are in use"""
    nb = 4
    omega = 2 * math.pi * nx / 10
    d = oracle.Discretization(oracle.Mesh.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), nb)
    h_a = np.ones(d.ndof)
    fh = np.concatenate([oracle.linear_functional(d, oracle.gaussians(omega)), 0.1 * oracle.linear_functional(d, oracle.mass_poly)])
    O = oracle.DDH(d, nx, nx, omega, h_a, np.float64)
    n = O.size
    lam = np.random.default_rng(7).standard_normal(n)
    used = np.unique(O.t.B[O.t.B >= 0])
    lam[np.setdiff1d(np.arange(n), np.concatenate([used, used + O.t.n_lambda]))] = 0.0
    written = np.unique(O.t.B[:, 1, :][O.t.B[:, 1, :] >= 0])
    written = np.concatenate([written, written + O.t.n_lambda])
    return omega, d, h_a, fh, O, lam, written


def entry_points(cd, torch, cuda, nx, precision, kernel, c):
    omega, d, h_a, fh, O, lam_h, written = c
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(4))
    F = cd.DDH(omega, h_a, fem, nx, nx, precision=precision, kernel=kernel)
    assert F.info()["kernel"] == kernel
    f = to_dev(torch, fh, cuda)
    lam = to_dev(torch, lam_h.astype(np.float32 if precision == "f32" else np.float64), cuda)
    b = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
    F.rhs(f, b)
    y = torch.zeros_like(b)
    F.action(lam, y)
    u = torch.zeros(2 * d.ndof, dtype=torch.float64, device=cuda)
    F.postprocess(lam, f, u)
    return F, fem, (b.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)[written], u.cpu().numpy())


def oracle_outputs(c):
    _, _, _, fh, O, lam_h, written = c
    return O.rhs(fh), O.action(lam_h)[written], O.postprocess(lam_h, fh)


@pytest.mark.parametrize("nx", [8, 16])
def test_kernel5_vs_fp64_oracle_and_kernel3(cuda, nx):
    import torch

    import cuddhelmholtz_amd as cd

    c = case(nx)
    ref = oracle_outputs(c)
    _, _, out5 = entry_points(cd, torch, cuda, nx, "f32", 5, c)
    _, _, out3 = entry_points(cd, torch, cuda, nx, "f32", 3, c)
    names = ("rhs", "action", "postprocess")
    e5 = tuple(rel(a, r) for a, r in zip(out5, ref))
    e3 = tuple(rel(a, r) for a, r in zip(out3, ref))
    e53 = tuple(float(np.linalg.norm(a - b) / np.linalg.norm(r)) for a, b, r in zip(out5, out3, ref))
    for i, nm in enumerate(names):
        print(f"[{nx}x{nx}, a=1] {nm}: kernel 5 vs fp64 oracle {e5[i]:.3e} (before the layout {PARENT5[nx][i]:.3e}, gate 2 x), "
              f"kernel 3 vs oracle {e3[i]:.3e}, kernel 5 vs kernel 3 {e53[i]:.3e}")
    for i, nm in enumerate(names):
        assert e5[i] < 2 * PARENT5[nx][i], (nm, e5[i], PARENT5[nx][i])
        assert e53[i] < 2 * PARENT5[nx][i] + e3[i], (nm, e53[i], e3[i])


@pytest.mark.parametrize("nx", [8, 16])
def test_kernel8_vs_fp64_oracle_and_kernel2(cuda, nx):
    import torch

    import cuddhelmholtz_amd as cd

    c = case(nx)
    ref = oracle_outputs(c)
    _, _, out8 = entry_points(cd, torch, cuda, nx, "f64", 8, c)
    _, _, out2 = entry_points(cd, torch, cuda, nx, "f64", 2, c)
    e8 = tuple(rel(a, r) for a, r in zip(out8, ref))
    e82 = tuple(rel(a, b) for a, b in zip(out8, out2))
    print(f"[{nx}x{nx}, a=1] kernel 8 vs fp64 oracle: rhs {e8[0]:.2e} action {e8[1]:.2e} postprocess {e8[2]:.2e}; "
          f"vs kernel 2: {e82[0]:.2e} {e82[1]:.2e} {e82[2]:.2e}")
    assert max(e8) < 1e-10
    assert max(e82) < 1e-11


@pytest.mark.parametrize("precision,kernel", [("f32", 5), ("f64", 8)])
def test_listed_and_priority_launches_are_bitwise_the_plain_one(cuda, precision, kernel):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 16
    c = case(nx)
    F, _, _ = entry_points(cd, torch, cuda, nx, precision, kernel, c)
    nd = F.info()["n_domains"]
    f = to_dev(torch, c[3], cuda)
    lam = to_dev(torch, c[5].astype(np.float32 if precision == "f32" else np.float64), cuda)
    perm = np.random.default_rng(3).permutation(nd).astype(np.int32)
    cut = max(1, nd // 3) | 1
    for x, l in ((f, None), (None, lam), (f, lam)):  # sources only, traces only (the form without x), both
        plain = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
        F.local_traces(0, nd, x, l, plain)
        assert plain.abs().max().item() > 0
        listed = torch.zeros_like(plain)
        for ids in (perm[:cut], perm[cut:]):
            F.local_traces_listed(to_dev(torch, ids, cuda), x, l, listed)
        assert torch.equal(listed, plain)
        F.set_wave_priority(True)
        held = torch.zeros_like(plain)
        F.local_traces(0, nd // 2, x, l, held)
        F.local_traces_listed(to_dev(torch, np.arange(nd // 2, nd, dtype=np.int32), cuda), x, l, held)
        F.set_wave_priority(False)
        assert torch.equal(held, plain)


def test_interior_trace_dof_is_refused(cuda):
    """one 4 x 4-element subdomain handed to cuddh_hip_ddh_plan_create directly: with the boundary dofs numbered first
    (what every block-built plan has) kernels 5 and 8 are built; with the dofs numbered row by row and the same s_fdof, the
    element-interior node (1, 1) of element 0 is dof 14 < s_fdof, a 'trace dof': 5 and 8 refuse, auto takes kernel 3"""
    import torch

    from cuddhelmholtz_amd import _native as N

    side, nbnd = 13, 48
    X, Y = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    rowwise = (X + side * Y).astype(np.int32)
    on_bnd = (X == 0) | (X == side - 1) | (Y == 0) | (Y == side - 1)
    facefirst = np.empty_like(rowwise)
    facefirst[on_bnd] = np.arange(nbnd, dtype=np.int32)
    facefirst[~on_bnd] = np.arange(nbnd, side * side, dtype=np.int32)

    def sI_of(numbering):
        sI = np.empty(256, dtype=np.int32)
        for el in range(16):
            for l in range(4):
                for k in range(4):
                    sI[k + 4 * (l + 4 * el)] = numbering[3 * (el % 4) + k, 3 * (el // 4) + l]
        return sI

    rng = np.random.default_rng(1)
    Dm = rng.standard_normal(16)
    Gel = rng.standard_normal(48)

    def create(numbering, is_f64, kernel):
        real = np.float64 if is_f64 else np.float32
        keep = [to_dev(torch, a, cuda) for a in (np.array([side * side], np.int32), np.array([nbnd], np.int32), sI_of(numbering),
                                                 Dm.astype(real), np.tile(Gel, 16).astype(real))]
        desc = N.DdhDesc(g_ndof=side * side, n_domains=1, n_lambda=nbnd, nb=4, nel1d=4, mx_dof=side * side, mx_fdof=nbnd, nt=1, omega=1.0,
                         dt=1.0, s_dof=keep[0].data_ptr(), s_fdof=keep[1].data_ptr(), sI=keep[2].data_ptr(), D=keep[3].data_ptr(),
                         G=keep[4].data_ptr())
        plan = C.c_void_p()
        err = N.lib.cuddh_hip_ddh_plan_create(C.byref(plan), C.byref(desc), int(is_f64), kernel)
        picked = N.lib.cuddh_hip_ddh_plan_kernel(plan) if err == 0 else None
        if err == 0:
            N.lib.cuddh_hip_ddh_plan_destroy(plan)
        torch.cuda.synchronize()
        return err, picked

    assert create(facefirst, False, 5) == (0, 5)
    assert create(facefirst, False, 0) == (0, 5)
    assert create(facefirst, True, 8) == (0, 8)
    assert create(rowwise, False, 3) == (0, 3)  # the table is a valid one for the kernels without the shortcut
    assert create(rowwise, False, 0) == (0, 3)
    assert create(rowwise, False, 5)[0] != 0
    assert create(rowwise, True, 8)[0] != 0
