"""cd.WaveHoltz(..., stiffness="lobatto", sweep="lattice") on the GPU: one launch per sweep on lattice-ordered vectors.

period and action against the numpy model tests/waveholtz_reference.py Case.model(scheme, coarsen, ratio, "lobatto") AND against the
same object built with sweep="operator", stiffness="lobatto", both at 1e-10 relative, the project's fp64 gate (measured values:
profiles/r25/wave_lattice_tests.txt).  Cases: 8 x 8 at n_basis 4 with rk2 and rk4 / 4; time ratio 2; the smooth coefficient with
the ratio taken from it; half the boundary faces absorbing; 6 x 6 at n_basis 3 and 5; 2 x 2 at n_basis 2; 4 x 2 elements of
[-1, 1] x [0, 0.7] (nx != ny, hx != hy) and 1 x 5 elements at n_basis 4.  period(None, f) against period(0, f) and f = None
against f = 0 bit for bit, action(0) = 0; two periods from the same input are bitwise equal.

solve: 8 x 8, rk2, GMRES(20), tol 1.6e-8.  The lobatto model's residual estimate is 3.504e-8 |b| after 19 matvecs and 7.259e-9 |b|
after 20 (measured on the CPU: tolerances 4e-8 and 6.4e-8 stop at 19, 5e-9 at 21), so every comparison GMRES makes is a factor
2.19 away from tol; checked here by running the model at 2 tol and at tol / 2 and asking for the same counts (20 matvecs in one
cycle).  res_norm is compared on the scale GMRES itself uses, |b|, as in tests/test_gpu_waveholtz.py.

driver: waveholtz_solve 16 4 3.2 20 100 1e-6 --integrator rk4 --coarsen 4 --sweep lattice against the lobatto model's count (30
matvecs in two cycles), +- 2.
"""
import functools
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import waveholtz_reference as wr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

ROOT = Path(__file__).resolve().parent.parent
GATE = 1e-10
SOLVE_TOL = 1.6e-8
SQUARE = (-1.0, 1.0, -1.0, 1.0)


@functools.lru_cache(maxsize=None)
def rect_case(nx, ny, nb, box, smooth=False):
    """wr.uniform_case for nx != ny and any box; omega = 2 pi max(nx, ny) / 10 as there"""
    import oracle

    if nx == ny and box == SQUARE:
        return wr.uniform_case(nx, nb, smooth)
    d = oracle.Discretization(oracle.Mesh.uniform_rect(nx, box[0], box[1], ny, box[2], box[3]), nb)
    return wr.Case(d, 2 * math.pi * max(nx, ny) / 10, wr.smooth_coefficient(d) if smooth else None)


def space_of(nx, ny, nb, box):
    import cuddhelmholtz_amd as cd

    return cd.H1Space(cd.Mesh2D.uniform_rect(nx, box[0], box[1], ny, box[2], box[3]), cd.Basis(nb))


def make(c, fem, scheme="rk2", coarsen=None, time_ratio=1, sweep="lattice", faces=None):
    import cuddhelmholtz_amd as cd

    W = cd.WaveHoltz(c.omega, c.h_a, fem, integrator=scheme, coarsen=coarsen, time_ratio=time_ratio, stiffness="lobatto", faces=faces, sweep=sweep)
    info = W.info()
    assert info["sweep"] == sweep
    ratio = wr.coefficient_ratio(c.h_a) if time_ratio == "coefficient" else time_ratio
    if faces is None:
        M = c.model(scheme, info["coarsen"], ratio, "lobatto")
    else:
        m, h = wr.lumped(c.d, faces)
        M = wr.Model(c.K_lobatto, m, h, c.h_a, c.omega, c.nt(info["coarsen"], ratio), scheme)
    assert (info["nt"], info["ratio"], info["integrator"]) == (M.nt, ratio, scheme)
    assert info["sweeps_per_period"] == M.nt * (2 if scheme == "rk2" else 4) and math.isclose(info["dt"], M.dt, rel_tol=1e-15)
    return W, M


def dev(x, cuda):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(cuda)


PERIOD_CASES = {
    # id: (nx, ny, n_basis, box, smooth a, scheme, coarsen, time_ratio, half the faces)
    "8x8-rk2": (8, 8, 4, SQUARE, False, "rk2", None, 1, False),
    "8x8-rk4": (8, 8, 4, SQUARE, False, "rk4", 4, 1, False),
    "8x8-rk2-ratio2": (8, 8, 4, SQUARE, False, "rk2", None, 2, False),
    "8x8-smooth-a-coefficient": (8, 8, 4, SQUARE, True, "rk4", 4, "coefficient", False),
    "8x8-half-the-faces": (8, 8, 4, SQUARE, False, "rk4", 4, 1, True),
    "6x6-nb3": (6, 6, 3, SQUARE, False, "rk2", None, 1, False),
    "6x6-nb5": (6, 6, 5, SQUARE, False, "rk4", 4, 1, False),
    "2x2-nb2": (2, 2, 2, SQUARE, False, "rk4", 2, 1, False),
    "4x2-box": (4, 2, 4, (-1.0, 1.0, 0.0, 0.7), False, "rk2", None, 1, False),
    "1x5": (1, 5, 4, SQUARE, False, "rk4", 4, 1, False),
}


@pytest.mark.parametrize("name", list(PERIOD_CASES))
def test_period_and_action_match_the_model_and_the_operator_form(cuda, name):
    import torch

    nx, ny, nb, box, smooth, scheme, coarsen, time_ratio, half_faces = PERIOD_CASES[name]
    c = rect_case(nx, ny, nb, box, smooth)
    fem = space_of(nx, ny, nb, box)
    assert fem.size() == c.d.ndof
    faces = np.asarray(c.d.mesh.boundary_edges[::2], dtype=np.int32) if half_faces else None
    W, M = make(c, fem, scheme, coarsen, time_ratio, "lattice", faces)
    Wo, _ = make(c, fem, scheme, coarsen, time_ratio, "operator", faces)
    assert W.info()["stiffness_kernel"].startswith(f"wave_lattice nb{nb}")
    n = W.size()
    assert n == 2 * c.d.ndof
    z = np.random.default_rng(11).standard_normal(n)
    out, out_o, y, y_o = (torch.full((n,), float("nan"), dtype=torch.float64, device=cuda) for _ in range(4))
    W.period(dev(z, cuda), dev(c.f, cuda), out)
    Wo.period(dev(z, cuda), dev(c.f, cuda), out_o)
    W.action(dev(z, cuda), y)  # the homogeneous march: y = x - S x
    Wo.action(dev(z, cuda), y_o)
    torch.cuda.synchronize()
    want, want_action = M.period(z, c.f), M.action(z)
    err, err_action = wr.rel(out.cpu().numpy(), want), wr.rel(y.cpu().numpy(), want_action)
    err_o, err_action_o = wr.rel(out.cpu().numpy(), out_o.cpu().numpy()), wr.rel(y.cpu().numpy(), y_o.cpu().numpy())
    print(f"waveholtz lattice period {name}: ndof={c.d.ndof} nt={M.nt} kernel={W.info()['stiffness_kernel']!r} vs model: period {err:.3e} action "
          f"{err_action:.3e}; vs operator form: period {err_o:.3e} action {err_action_o:.3e}")
    assert err < GATE and err_action < GATE
    assert err_o < GATE and err_action_o < GATE
    if half_faces:
        assert wr.rel(want, c.model(scheme, 4, 1, "lobatto").period(z, c.f)) > 1e-3  # the faces matter


@pytest.mark.parametrize("scheme", ["rk2", "rk4"])
def test_absent_arguments_and_reproducibility_bit_for_bit(cuda, scheme):
    import torch

    c = rect_case(8, 8, 4, SQUARE)
    W, _ = make(c, space_of(8, 8, 4, SQUARE), scheme)
    n = W.size()
    zero = torch.zeros(n, dtype=torch.float64, device=cuda)
    f, z = dev(c.f, cuda), dev(np.random.default_rng(5).standard_normal(n), cuda)
    a, b = torch.empty_like(zero), torch.empty_like(zero)
    W.period(None, f, a)
    W.period(zero, f, b)
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    W.rhs(f, b)
    assert torch.equal(a, b)
    W.period(z, None, a)
    W.period(z, zero, b)
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    # two periods from the same input are the same bits
    W.period(z, f, a)
    W.period(z, f, b)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    # action(0) = 0, and action(c, x, y) accumulates c (x - S x)
    W.action(zero, a)
    assert float(a.abs().max()) == 0.0
    W.action(z, a)
    y = torch.ones_like(zero)
    W.action(-0.5, z, y)
    assert wr.rel((y - 1.0).cpu().numpy(), (-0.5 * a).cpu().numpy()) < 1e-13
    W.solution(z, b)
    want = z.clone()
    want[n // 2:] *= 1.0 / c.omega
    assert torch.equal(b, want)


@functools.lru_cache(maxsize=None)
def solve_reference():
    """the lobatto model's GMRES(20) at SOLVE_TOL on 8 x 8, rk2; and its counts at twice and half that tolerance"""
    c = wr.uniform_case(8, 4)
    M = c.model("rk2", 1, 1, "lobatto")
    z, info = M.gmres(c.f, 20, 100, SOLVE_TOL)
    around = [M.gmres(c.f, 20, 100, t)[1] for t in (2 * SOLVE_TOL, SOLVE_TOL / 2)]
    return M, z, info, around


def check_solve(out, u, what):
    c = wr.uniform_case(8, 4)
    M, z, info, around = solve_reference()
    # every comparison the model's GMRES makes against tol is a factor 2 away from it
    for other in around:
        assert (other["num_matvec"], other["num_iter"], other["success"]) == (info["num_matvec"], info["num_iter"], True)
    assert (info["num_matvec"], info["num_iter"]) == (20, 1)
    direct = M.direct(c.f)
    model_distance = wr.rel(M.solution(z), direct)
    res, ref = np.asarray(out.res_norm), np.asarray(info["res_norm"])
    res_err = float(np.abs(res - ref).max() / ref[0]) if res.shape == ref.shape else float("inf")
    sol_err, distance = wr.rel(u, M.solution(z)), wr.rel(u, direct)
    print(f"waveholtz lattice solve {what}: matvecs {out.num_matvec} cycles {out.num_iter} res_norm {list(res)} vs model {list(ref)} "
          f"({res_err:.3e} of |b|) solution vs model {sol_err:.3e}, vs direct {distance:.3e} (model {model_distance:.3e})")
    assert out.success and (out.num_matvec, out.num_iter) == (info["num_matvec"], info["num_iter"])
    assert abs(res[0] - ref[0]) < 1e-8 * ref[0] and res_err < 1e-8
    assert sol_err < 1e-8
    assert distance < 2 * model_distance


@pytest.mark.parametrize("orth", ["mgs", "cgs2"])
def test_solve_follows_the_model(cuda, orth):
    import torch

    import cuddhelmholtz_amd as cd

    c = rect_case(8, 8, 4, SQUARE)
    W, _ = make(c, space_of(8, 8, 4, SQUARE))
    n = W.size()
    f = dev(c.f, cuda)
    b, z, u = (torch.zeros(n, dtype=torch.float64, device=cuda) for _ in range(3))
    W.rhs(f, b)
    out = cd.gmres(n, z, W, b, 20, 100, SOLVE_TOL, orth=orth)
    W.solution(z, u)
    check_solve(out, u.cpu().numpy(), f"gmres orth={orth}")


def test_solve_method_and_augmented_restarts(cuda):
    """(with augment: both forms stop at a relative residual of 1e-6, so their solutions agree to about that, not to the gate)"""
    import torch

    c = rect_case(8, 8, 4, SQUARE)
    W, _ = make(c, space_of(8, 8, 4, SQUARE))
    u = torch.zeros(W.size(), dtype=torch.float64, device=cuda)
    out = W.solve(dev(c.f, cuda), u, m=20, maxit=100, tol=SOLVE_TOL)
    check_solve(out, u.cpu().numpy(), "WaveHoltz.solve")
    # augmented restarts, GMRES(5): the same algorithm on the operator form, whose action agrees to the gate, takes the same path
    Wo, _ = make(c, space_of(8, 8, 4, SQUARE), sweep="operator")
    uo = torch.zeros_like(u)
    out = W.solve(dev(c.f, cuda), u, m=5, maxit=100, tol=1e-6, augment=2)
    out_o = Wo.solve(dev(c.f, cuda), uo, m=5, maxit=100, tol=1e-6, augment=2)
    print(f"waveholtz lattice solve augment=2: matvecs {out.num_matvec} (operator form {out_o.num_matvec}), solutions differ by "
          f"{wr.rel(u.cpu().numpy(), uo.cpu().numpy()):.3e}")
    assert out.success and out_o.success and out.num_iter > 1
    assert abs(out.num_matvec - out_o.num_matvec) <= 1 and wr.rel(u.cpu().numpy(), uo.cpu().numpy()) < 2e-6


def test_info_and_refusal(cuda):
    import cuddhelmholtz_amd as cd

    c = rect_case(8, 8, 4, SQUARE)
    fem = space_of(8, 8, 4, SQUARE)
    assert make(c, fem)[0].info()["sweep"] == "lattice"
    assert cd.WaveHoltz(c.omega, c.h_a, fem, stiffness="lobatto").info()["sweep"] == "operator"
    assert cd.WaveHoltz(c.omega, c.h_a, fem).info()["sweep"] == "operator"
    mesh = cd.Mesh2D.load(ROOT / "tests" / "golden" / "unstructured_square")
    ufem = cd.H1Space(mesh, cd.Basis(4))
    with pytest.raises(ValueError, match="WaveHoltz error: sweep:"):
        cd.WaveHoltz(4 * math.pi, np.ones(ufem.size()), ufem, stiffness="lobatto", sweep="lattice")


def test_waveholtz_solve_driver_lattice(cuda):
    exe = ROOT / "build" / "examples" / "waveholtz_solve"
    if not exe.exists():
        pytest.fail("build/examples/waveholtz_solve missing: run __graft_entry__.build()")
    r = subprocess.run([str(exe), "16", "4", "3.2", "20", "100", "1e-6", "--integrator", "rk4", "--coarsen", "4", "--sweep", "lattice"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("waveholtz_solve")]
    assert len(lines) == 1
    print(lines[0])
    got = dict(re.findall(r"(\S+)=(\"[^\"]*\"|\S+)", lines[0]))
    c = wr.uniform_case(16, 4)
    M = c.model("rk4", 4, 1, "lobatto")
    _, info = M.gmres(c.f, 20, 100, 1e-6)
    assert info["success"] and info["num_matvec"] == 30  # recorded
    assert int(got["success"]) == 1 and abs(int(got["num_matvec"]) - info["num_matvec"]) <= 2
    assert float(got["rel_res"]) < 1e-6
    assert (got["stiffness"], got["sweep"], got["kernel"]) == ("lobatto", "lattice", '"wave_lattice nb4"')
    assert (int(got["ndof"]), int(got["nt"]), int(got["sweeps_per_period"])) == (c.d.ndof, M.nt, 4 * M.nt)
    # the contradiction is refused
    r = subprocess.run([str(exe), "16", "4", "--sweep", "lattice", "--stiffness", "gauss"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--sweep lattice" in r.stderr
