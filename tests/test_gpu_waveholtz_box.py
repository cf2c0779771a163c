"""cd.WaveHoltzBox on the GPU: the whole-domain WaveHoltz march in three dimensions, one launch per sweep.

Against the numpy model (tests/wave_box_reference.py, pinned by tests/test_wave_box_host.py): period from zero, from a random z,
with and without a load, and action, at 1e-10 relative, the project's gate for fp64 periods; the measured distances are printed.
Cases: (3, 2, 2) elements of size 0.5, n_basis 4, omega = pi (nt = 640 for rk2, 160 for rk4 / 4), a smooth a in [0.8, 1.25]; the
same with only x0, x1 absorbing; (2, 2, 2) with three different edge lengths; n_basis 3, 5, 6 on (2, 2, 3), (2, 1, 2), (1, 2, 2);
time ratio 2; time ratio "coefficient" with min a = 0.5, the ratio asserted against the rule.

Against the existing product, with no model at all: a box with z-independent a, sound-hard z0 and z1, a z-constant start and the
load f3 = (hz / 2) Wz (x) f2.  Every z plane of the period is the period of cd.WaveHoltz(stiffness="lobatto", sweep="lattice") on
the cross-section, to 1e-10: (4, 3, 2) elements, n_basis 4, rk2 and rk4 / 4, hz >= min(hx, hy) so that the time grids coincide.

Absent arguments and repeated periods bit for bit; info(); GMRES(20) on (2, 2, 2) elements, n_basis 4, with the model's counts and
residual norms, solve() equal to the three calls, and the same under orth="cgs2" and augment=2 against the model run the same way.
The residual falls by about a third per matvec here, so no tolerance has a factor 2 of room; SOLVE_TOL = 1e-7 (three cycles: 49
matvecs, 50 with augment=2) is one where the model's counts at 1.001 and at 1 / 1.001 times the tolerance are its counts at the
tolerance (asserted), seven orders above the distance between the device's operator and the model's.
"""
import functools
import math

import numpy as np
import pytest

import wave_box_reference as wb
import waveholtz_reference as wr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

GATE = 1e-10
HALF = ((0.0, 1.5), (0.0, 1.0), (0.0, 1.0))  # with (3, 2, 2) elements: h = 0.5 throughout
BOX3 = ((-1.0, 0.5), (0.25, 1.0), (-0.5, 1.5))
SOLVE_TOL = 1e-7

PERIOD_CASES = {
    # id: (shape, box, n_basis, omega, absorbing, coefficient range, scheme, coarsen, time_ratio)
    "3x2x2-rk2": ((3, 2, 2), HALF, 4, math.pi, wb.FACES, (0.8, 1.25), "rk2", None, 1),
    "3x2x2-rk4": ((3, 2, 2), HALF, 4, math.pi, wb.FACES, (0.8, 1.25), "rk4", 4, 1),
    "3x2x2-x-faces-rk2": ((3, 2, 2), HALF, 4, math.pi, ("x0", "x1"), (0.8, 1.25), "rk2", None, 1),
    "3x2x2-x-faces-rk4": ((3, 2, 2), HALF, 4, math.pi, ("x0", "x1"), (0.8, 1.25), "rk4", 4, 1),
    "2x2x2-three-edges": ((2, 2, 2), BOX3, 4, math.pi, wb.FACES, (0.8, 1.25), "rk4", 4, 1),
    "2x2x3-nb3": ((2, 2, 3), BOX3, 3, math.pi, wb.FACES, (0.8, 1.25), "rk2", None, 1),
    "2x1x2-nb5": ((2, 1, 2), BOX3, 5, math.pi, wb.FACES, (0.8, 1.25), "rk4", 4, 1),
    "1x2x2-nb6": ((1, 2, 2), BOX3, 6, math.pi, wb.FACES, (0.8, 1.25), "rk4", 4, 1),
    "3x2x2-ratio2": ((3, 2, 2), HALF, 4, math.pi, wb.FACES, (0.8, 1.25), "rk4", 4, 2),
    "3x2x2-coefficient": ((3, 2, 2), HALF, 4, math.pi, wb.FACES, (0.5, 1.25), "rk4", 4, "coefficient"),
}


@functools.lru_cache(maxsize=None)
def reference(shape, box, nb, absorbing):
    return wb.Box(shape, box, nb, absorbing)


def dev(x, cuda):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(cuda)


def make(B, omega, a, scheme="rk2", coarsen=None, time_ratio=1):
    import cuddhelmholtz_amd as cd

    Lx, Ly, Lz = B.L
    W = cd.WaveHoltzBox(omega, a.reshape(Lz, Ly, Lx), shape=B.shape, box=B.box, n_basis=B.nb, integrator=scheme, coarsen=coarsen,
                        time_ratio=time_ratio, absorbing=B.absorbing)
    info = W.info()
    ratio = wr.coefficient_ratio(a) if time_ratio == "coefficient" else time_ratio
    M = B.model(omega, a, scheme, info["coarsen"], ratio)
    assert (info["nt"], info["ratio"], info["integrator"], info["nodes"]) == (M.nt, ratio, scheme, B.n)
    assert info["sweeps_per_period"] == M.nt * (2 if scheme == "rk2" else 4) and math.isclose(info["dt"], M.dt, rel_tol=1e-15)
    assert W.lattice_shape() == B.L and W.size() == 2 * B.n
    return W, M


@pytest.mark.parametrize("name", list(PERIOD_CASES))
def test_period_and_action_match_the_model(cuda, name):
    import torch

    shape, box, nb, omega, absorbing, (lo, hi), scheme, coarsen, time_ratio = PERIOD_CASES[name]
    B = reference(shape, box, nb, tuple(absorbing))
    a = B.smooth_coefficient(lo, hi)
    assert a.min() == lo and a.max() == hi
    W, M = make(B, omega, a, scheme, coarsen, time_ratio)
    if name == "3x2x2-rk2":
        assert M.nt == 640
    if name == "3x2x2-rk4":
        assert M.nt == 160
    if time_ratio == "coefficient":
        assert W.info()["ratio"] == wr.coefficient_ratio(a) == 2
    assert W.info()["stiffness_kernel"] == f"wave_box nb{nb}" + ("" if nb == 4 else " (run-time n_basis)")
    n = W.size()
    f = B.example_load(omega)
    z = np.random.default_rng(11).standard_normal(n)
    outs = [torch.full((n,), float("nan"), dtype=torch.float64, device=cuda) for _ in range(5)]
    W.period(None, dev(f, cuda), outs[0])
    W.period(dev(z, cuda), dev(f, cuda), outs[1])
    W.period(dev(z, cuda), None, outs[2])
    W.action(dev(z, cuda), outs[3])
    W.rhs(dev(f, cuda), outs[4])
    torch.cuda.synchronize()
    wants = [M.period(None, f), M.period(z, f), M.period(z, None), M.action(z), M.rhs(f)]
    errs = [wr.rel(o.cpu().numpy(), w) for o, w in zip(outs, wants)]
    print(f"waveholtz box period {name}: nodes={B.n} nt={M.nt} kernel={W.info()['stiffness_kernel']!r} vs model: from zero {errs[0]:.3e}, "
          f"from z {errs[1]:.3e}, without a load {errs[2]:.3e}, action {errs[3]:.3e}, rhs {errs[4]:.3e}")
    assert max(errs) < GATE
    if tuple(absorbing) != wb.FACES:
        assert wr.rel(wants[1], reference(shape, box, nb, wb.FACES).model(omega, a, scheme, 4 if scheme == "rk4" else 1).period(z, f)) > 1e-3  # the faces matter


@pytest.mark.parametrize("scheme,coarsen", [("rk2", None), ("rk4", 4)])
def test_every_plane_of_an_extruded_problem_is_the_two_dimensional_lattice_form(cuda, scheme, coarsen):
    import torch

    import cuddhelmholtz_amd as cd
    from cuddhelmholtz_amd import _native as N

    nx, ny, nz, nb, omega = 4, 3, 2, 4, 1.3 * math.pi
    box = ((-1.0, 1.0), (0.0, 1.2), (0.0, 1.5))  # hx = 0.5, hy = 0.4, hz = 0.75 >= min(hx, hy)
    B = reference((nx, ny, nz), box, nb, ("x0", "x1", "y0", "y1"))
    Lx, Ly, Lz = B.L
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, *box[0], ny, *box[1]), cd.Basis(nb))
    dims, h, node_of = np.zeros(5, dtype=np.int32), np.zeros(2), np.full(fem.size(), -7, dtype=np.int32)
    assert N.lib.cuddh_wave_lattice_map(fem._h, dims.ctypes.data, h.ctypes.data, node_of.ctypes.data) == 0 and fem.size() == Lx * Ly
    assert (int(dims[2]), int(dims[3])) == (Lx, Ly)
    # z-independent data, in the cross-section's lattice order
    X = B.nodes[0].reshape(-1, 3)
    a2 = 1.0 + 0.2 * np.sin(2.0 * X[:, 0] + 0.3) * np.cos(1.5 * X[:, 1] - 0.2)
    rng = np.random.default_rng(17)
    z2, f2 = rng.standard_normal((2, Lx * Ly)), rng.standard_normal((2, Lx * Ly))
    Wz = B.lines[2][1]
    hz = B.hs[2]
    W2 = cd.WaveHoltz(omega, a2[node_of], fem, integrator=scheme, coarsen=coarsen, stiffness="lobatto", sweep="lattice")
    W3 = cd.WaveHoltzBox(omega, np.tile(a2, Lz), shape=(nx, ny, nz), box=box, n_basis=nb, integrator=scheme, coarsen=coarsen, absorbing=B.absorbing)
    assert W2.info()["nt"] == W3.info()["nt"] and W2.info()["dt"] == W3.info()["dt"]
    to_dofs = lambda v: np.concatenate([v[0][node_of], v[1][node_of]])  # noqa: E731
    extrude = lambda v, wts: np.concatenate([np.kron(wts, v[0]), np.kron(wts, v[1])])  # noqa: E731
    out2 = torch.full((W2.size(),), float("nan"), dtype=torch.float64, device=cuda)
    out3 = torch.full((W3.size(),), float("nan"), dtype=torch.float64, device=cuda)
    W2.period(dev(to_dofs(z2), cuda), dev(to_dofs(f2), cuda), out2)
    W3.period(dev(extrude(z2, np.ones(Lz)), cuda), dev(extrude(f2, hz / 2 * Wz), cuda), out3)
    torch.cuda.synchronize()
    got2 = out2.cpu().numpy().reshape(2, -1)
    plane = np.empty((2, Lx * Ly))
    plane[:, node_of] = got2
    got3 = out3.cpu().numpy().reshape(2, Lz, Lx * Ly)
    errs = [wr.rel(got3[:, k], plane) for k in range(Lz)]
    print(f"waveholtz box {scheme}: nt={W3.info()['nt']}, planes of the extruded period vs the 2-D lattice form: {max(errs):.3e}")
    assert max(errs) < GATE and np.abs(plane).max() > 0


@pytest.mark.parametrize("scheme,nb", [("rk2", 4), ("rk4", 4), ("rk4", 3)])
def test_absent_arguments_and_reproducibility_bit_for_bit(cuda, scheme, nb):
    import torch

    B = reference((2, 2, 2), BOX3, nb, wb.FACES)
    W, _ = make(B, math.pi, B.smooth_coefficient(), scheme)
    n = W.size()
    zero = torch.zeros(n, dtype=torch.float64, device=cuda)
    f, z = dev(B.example_load(math.pi), cuda), dev(np.random.default_rng(5).standard_normal(n), cuda)
    a, b = torch.empty_like(zero), torch.empty_like(zero)
    W.period(None, f, a)
    W.period(zero, f, b)
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    W.rhs(f, b)
    assert torch.equal(a, b)
    W.period(z, None, a)
    W.period(z, zero, b)
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    W.period(z, f, a)
    W.period(z, f, b)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    W.action(zero, a)
    assert float(a.abs().max()) == 0.0
    W.action(z, a)
    y = torch.ones_like(zero)
    W.action(-0.5, z, y)
    assert wr.rel((y - 1.0).cpu().numpy(), (-0.5 * a).cpu().numpy()) < 1e-13
    W.solution(z, b)
    want = z.clone()
    want[n // 2:] *= 1.0 / math.pi
    assert torch.equal(b, want)


def test_info_nodes_mass_and_kernel_names(cuda):
    import cuddhelmholtz_amd as cd

    for nb, kernel in ((4, "wave_box nb4"), (5, "wave_box nb5 (run-time n_basis)"), (2, "wave_box nb2 (run-time n_basis)")):
        B = reference((2, 1, 2), BOX3, nb, wb.FACES)
        W = cd.WaveHoltzBox(2.0, np.ones(B.n), shape=B.shape, box=B.box, n_basis=nb, integrator="rk4")
        info = W.info()
        assert info["stiffness_kernel"] == kernel == W.kernel() and (info["integrator"], info["coarsen"], info["ratio"]) == ("rk4", 4, 1)
        assert info["nt"] == B.nt(2.0, 4) and info["sweeps_per_period"] == 4 * info["nt"] and info["nodes"] == B.n
        assert W.lattice_shape() == B.L and W.size() == 2 * B.n
        assert np.abs(W.nodes() - B.nodes).max() < 1e-14 and W.nodes().shape == (B.L[2], B.L[1], B.L[0], 3)
        assert np.abs(W.mass().reshape(-1) - B.m).max() <= 1e-12 * B.m.max() and W.mass().shape == (B.L[2], B.L[1], B.L[0])


@functools.lru_cache(maxsize=None)
def solve_reference(orth, augment):
    """the model's GMRES(20) at SOLVE_TOL on (2, 2, 2) elements, n_basis 4, rk4 / 4; and its counts at 1.001 and 1 / 1.001 times that tolerance"""
    import lgmres_reference as lr

    B = reference((2, 2, 2), ((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), 4, wb.FACES)
    a = B.smooth_coefficient()
    M = B.model(2 * math.pi, a, "rk4", 4)
    f = B.example_load(2 * math.pi)
    run = lambda tol: lr.lgmres_ref(M.action, M.rhs(f), 20, 100, tol, augment, orth=orth)  # noqa: E731
    z, info = run(SOLVE_TOL)
    return B, a, M, f, z, info, [run(t)[1] for t in (1.001 * SOLVE_TOL, SOLVE_TOL / 1.001)]


@pytest.mark.parametrize("orth,augment", [("mgs", 0), ("cgs2", 0), ("mgs", 2)])
def test_solve_follows_the_model(cuda, orth, augment):
    import torch

    import cuddhelmholtz_amd as cd

    B, a, M, f, z_ref, info, around = solve_reference(orth, augment)
    for other in around:  # every comparison the model's GMRES makes against tol is 1e-3 away from it, the device within 1e-10 of the model
        assert (other["num_matvec"], other["num_iter"], other["success"]) == (info["num_matvec"], info["num_iter"], True)
    W, _ = make(B, 2 * math.pi, a, "rk4", 4)
    n = W.size()
    fd = dev(f, cuda)
    b, z, u, u2 = (torch.zeros(n, dtype=torch.float64, device=cuda) for _ in range(4))
    W.rhs(fd, b)
    out = cd.gmres(n, z, W, b, 20, 100, SOLVE_TOL, orth=orth, augment=augment)
    W.solution(z, u)
    res, ref = np.asarray(out.res_norm), np.asarray(info["res_norm"])
    res_err = float(np.abs(res - ref).max() / ref[0]) if res.shape == ref.shape else float("inf")
    sol_err = wr.rel(u.cpu().numpy(), M.solution(z_ref))
    direct = M.direct(f)
    print(f"waveholtz box solve orth={orth} augment={augment}: matvecs {out.num_matvec} cycles {out.num_iter} (model {info['num_matvec']}, "
          f"{info['num_iter']}) res_norm vs model {res_err:.3e} of |b|, solution vs model {sol_err:.3e}, vs direct "
          f"{wr.rel(u.cpu().numpy(), direct):.3e} (model {wr.rel(M.solution(z_ref), direct):.3e})")
    assert out.success and (out.num_matvec, out.num_iter) == (info["num_matvec"], info["num_iter"])
    assert abs(res[0] - ref[0]) < 1e-8 * ref[0] and res_err < 1e-8
    assert sol_err < 1e-6
    # solve() is the three calls
    out2 = W.solve(fd, u2, m=20, maxit=100, tol=SOLVE_TOL, orth=orth, augment=augment)
    assert (out2.num_matvec, out2.num_iter, list(out2.res_norm)) == (out.num_matvec, out.num_iter, list(out.res_norm)) and torch.equal(u, u2)
