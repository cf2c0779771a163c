"""cd.WaveHoltz on the GPU against tests/waveholtz_reference.py (pinned by tests/test_waveholtz_reference.py).

period: W(z; f) for a random z and the examples' load against the model at 1e-10 relative, the project's fp64 gate (measured
values: profiles/r24/waveholtz_tests.txt), over both integrators, a time ratio, both stiffness rules, a smooth coefficient with
the ratio given and taken from it, n_basis 3 and 5, the reference's unstructured square and the 9-dof mesh; period(None, f)
against period(0, f) and f = None against f = 0 bit for bit; action(0) = 0.

solve: 8 x 8, rk2, GMRES(20), tol 1.6e-8.  The model's residual estimate is 3.50e-8 |b| after 17 steps and 7.26e-9 |b| after 18,
so every comparison GMRES makes is a factor 2 away from tol: checked here by running the model at 2 tol and at tol / 2 and asking
for the same counts (20 matvecs in one cycle).  res_norm is compared on the scale GMRES itself uses, |b|: the last entry,
5e-8, is the norm of a difference of vectors of size 7, and eps |b| / 5e-8 = 3e-8 forbids a relative 1e-8 of that entry alone
(measured: the last entries differ by 1.7e-8 of themselves, which is 1.2e-16 of |b|; the first entries are equal).
CGS2 orthogonalises the same Krylov space to working precision, so its run is held to the same model figures.

driver: waveholtz_solve 16 4 3.2 20 100 1e-6 --integrator rk4 --coarsen 4 against the model's count with the same stiffness
rule (30 matvecs in two cycles at 1e-6; 39 at 1e-8), +- 2.
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


@functools.lru_cache(maxsize=None)
def unstructured_case():
    import oracle
    from conftest import load_unstructured_square

    xy, elems = load_unstructured_square()
    return wr.Case(oracle.Discretization(oracle.Mesh(xy, elems), 4), 4 * math.pi)


def case_and_space(mesh_name, nb, smooth=False):
    import cuddhelmholtz_amd as cd

    if mesh_name == "unstructured":
        c = unstructured_case()
        mesh = cd.Mesh2D.load(ROOT / "tests" / "golden" / "unstructured_square")
    else:
        nx = int(mesh_name)
        c = wr.uniform_case(nx, nb, smooth)
        mesh = cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0)
    fem = cd.H1Space(mesh, cd.Basis(nb))
    assert fem.size() == c.d.ndof
    return c, fem


def make(c, fem, scheme="rk2", coarsen=None, time_ratio=1, stiffness="gauss"):
    import cuddhelmholtz_amd as cd

    W = cd.WaveHoltz(c.omega, c.h_a, fem, integrator=scheme, coarsen=coarsen, time_ratio=time_ratio, stiffness=stiffness)
    info = W.info()
    ratio = wr.coefficient_ratio(c.h_a) if time_ratio == "coefficient" else time_ratio
    M = c.model(scheme, info["coarsen"], ratio, stiffness)
    assert (info["nt"], info["ratio"], info["integrator"]) == (M.nt, ratio, scheme)
    assert info["sweeps_per_period"] == M.nt * (2 if scheme == "rk2" else 4) and math.isclose(info["dt"], M.dt, rel_tol=1e-15)
    return W, M


def dev(x, cuda):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(cuda)


PERIOD_CASES = {
    # id: (mesh, n_basis, smooth a, scheme, coarsen, time_ratio, stiffness)
    "8x8-rk2-gauss": ("8", 4, False, "rk2", None, 1, "gauss"),
    "8x8-rk2-lobatto": ("8", 4, False, "rk2", None, 1, "lobatto"),
    "8x8-rk4-gauss": ("8", 4, False, "rk4", 4, 1, "gauss"),
    "8x8-rk4-lobatto": ("8", 4, False, "rk4", 4, 1, "lobatto"),
    "8x8-rk2-ratio2": ("8", 4, False, "rk2", None, 2, "gauss"),
    "8x8-smooth-a": ("8", 4, True, "rk2", None, 2, "gauss"),
    "8x8-smooth-a-coefficient": ("8", 4, True, "rk4", 4, "coefficient", "lobatto"),
    "6x6-nb3": ("6", 3, False, "rk2", None, 1, "gauss"),
    "6x6-nb5": ("6", 5, False, "rk4", 4, 1, "gauss"),
    "6x6-nb5-lobatto": ("6", 5, False, "rk2", None, 1, "lobatto"),
    "unstructured": ("unstructured", 4, False, "rk2", None, 1, "gauss"),
    "unstructured-lobatto": ("unstructured", 4, False, "rk4", 4, 1, "lobatto"),
    "2x2-nb2": ("2", 2, False, "rk2", None, 1, "gauss"),
    "2x2-nb2-rk4": ("2", 2, False, "rk4", 2, 1, "lobatto"),
}


@pytest.mark.parametrize("name", list(PERIOD_CASES))
def test_period_matches_the_model(cuda, name):
    import torch

    mesh_name, nb, smooth, scheme, coarsen, time_ratio, stiffness = PERIOD_CASES[name]
    c, fem = case_and_space(mesh_name, nb, smooth)
    W, M = make(c, fem, scheme, coarsen, time_ratio, stiffness)
    n = W.size()
    assert n == 2 * c.d.ndof
    z = np.random.default_rng(11).standard_normal(n)
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=cuda)
    W.period(dev(z, cuda), dev(c.f, cuda), out)
    torch.cuda.synchronize()
    err = wr.rel(out.cpu().numpy(), M.period(z, c.f))
    # the homogeneous march through action(): y = x - S x
    y = torch.full((n,), float("nan"), dtype=torch.float64, device=cuda)
    W.action(dev(z, cuda), y)
    torch.cuda.synchronize()
    err_action = wr.rel(y.cpu().numpy(), M.action(z))
    print(f"waveholtz period {name}: ndof={c.d.ndof} nt={M.nt} kernel={W.info()['stiffness_kernel']!r} period {err:.3e} action {err_action:.3e}")
    assert err < GATE and err_action < GATE


@pytest.mark.parametrize("scheme", ["rk2", "rk4"])
def test_absent_arguments_are_zero_arguments_bit_for_bit(cuda, scheme):
    import torch

    c, fem = case_and_space("8", 4)
    W, _ = make(c, fem, scheme)
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
    # action(0) = 0, and action(c, x, y) accumulates c (x - S x)
    W.action(zero, a)
    assert float(a.abs().max()) == 0.0
    W.action(z, a)
    y = torch.ones_like(zero)
    W.action(-0.5, z, y)
    assert wr.rel((y - 1.0).cpu().numpy(), (-0.5 * a).cpu().numpy()) < 1e-13
    # solution scales the second half by 1 / omega, in place too
    W.solution(z, b)
    want = z.clone()
    want[n // 2:] *= 1.0 / c.omega
    assert torch.equal(b, want)
    W.solution(b, b)
    want[n // 2:] *= 1.0 / c.omega
    assert torch.equal(b, want)


def test_absorbing_faces_can_be_listed(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    c, fem = case_and_space("8", 4)
    faces = np.asarray(c.d.mesh.boundary_edges[::2], dtype=np.int32)
    m, h = wr.lumped(c.d, faces)
    M = wr.Model(c.K_gauss, m, h, c.h_a, c.omega, c.nt(4), "rk4")
    W = cd.WaveHoltz(c.omega, c.h_a, fem, integrator="rk4", faces=faces)
    z = np.random.default_rng(2).standard_normal(W.size())
    out = torch.empty(W.size(), dtype=torch.float64, device=cuda)
    W.period(dev(z, cuda), dev(c.f, cuda), out)
    err = wr.rel(out.cpu().numpy(), M.period(z, c.f))
    print(f"waveholtz period 8x8-half-the-faces: {err:.3e}")
    assert err < GATE
    assert wr.rel(M.period(z, c.f), c.model("rk4", 4, 1, "gauss").period(z, c.f)) > 1e-3  # the faces matter


@functools.lru_cache(maxsize=None)
def solve_reference():
    """the model's GMRES(20) at SOLVE_TOL on 8 x 8, rk2, Gauss stiffness; and its counts at twice and half that tolerance"""
    c = wr.uniform_case(8, 4)
    M = c.model("rk2", 1, 1, "gauss")
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
    print(f"waveholtz solve {what}: matvecs {out.num_matvec} cycles {out.num_iter} res_norm {list(res)} vs model {list(ref)} ({res_err:.3e} of |b|) "
          f"solution vs model {sol_err:.3e}, vs direct {distance:.3e} (model {model_distance:.3e})")
    assert out.success and (out.num_matvec, out.num_iter) == (info["num_matvec"], info["num_iter"])
    assert abs(res[0] - ref[0]) < 1e-8 * ref[0] and res_err < 1e-8
    assert sol_err < 1e-8
    assert distance < 2 * model_distance


@pytest.mark.parametrize("orth", ["mgs", "cgs2"])
def test_solve_follows_the_model(cuda, orth):
    import torch

    import cuddhelmholtz_amd as cd

    c, fem = case_and_space("8", 4)
    W, _ = make(c, fem)
    n = W.size()
    f = dev(c.f, cuda)
    b, z, u = (torch.zeros(n, dtype=torch.float64, device=cuda) for _ in range(3))
    W.rhs(f, b)
    out = cd.gmres(n, z, W, b, 20, 100, SOLVE_TOL, orth=orth)
    W.solution(z, u)
    check_solve(out, u.cpu().numpy(), f"gmres orth={orth}")


def test_solve_method(cuda):
    import torch

    c, fem = case_and_space("8", 4)
    W, _ = make(c, fem)
    u = torch.zeros(W.size(), dtype=torch.float64, device=cuda)
    out = W.solve(dev(c.f, cuda), u, m=20, maxit=100, tol=SOLVE_TOL)
    check_solve(out, u.cpu().numpy(), "WaveHoltz.solve")


def test_waveholtz_solve_driver(cuda):
    exe = ROOT / "build" / "examples" / "waveholtz_solve"
    if not exe.exists():
        pytest.fail("build/examples/waveholtz_solve missing: run __graft_entry__.build()")
    r = subprocess.run([str(exe), "16", "4", "3.2", "20", "100", "1e-6", "--integrator", "rk4", "--coarsen", "4", "--residuals"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("waveholtz_solve")]
    assert len(lines) == 2 and lines[1].startswith("waveholtz_solve residuals:")
    print(lines[0])
    got = dict(re.findall(r"(\S+)=(\"[^\"]*\"|\S+)", lines[0]))
    c = wr.uniform_case(16, 4)
    M = c.model("rk4", 4, 1, "gauss")
    _, info = M.gmres(c.f, 20, 100, 1e-6)
    assert info["success"] and info["num_matvec"] == 30  # recorded; 39 at 1e-8
    assert int(got["success"]) == 1 and abs(int(got["num_matvec"]) - info["num_matvec"]) <= 2
    assert float(got["rel_res"]) < 1e-6
    assert (int(got["ndof"]), int(got["nt"]), int(got["sweeps_per_period"]), got["integrator"], int(got["coarsen"])) == (c.d.ndof, M.nt, 4 * M.nt, "rk4", 4)
    assert float(got["t_gmres"]) > 0 and float(got["ms_per_period"]) > 0 and float(got["us_per_sweep"]) > 0
    residuals = [float(v) for v in lines[1].split(":")[1].split()]
    assert residuals[0] == 1.0 and residuals[-1] == pytest.approx(float(got["rel_res"]), rel=1e-4)
