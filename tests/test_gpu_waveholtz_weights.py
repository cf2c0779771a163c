"""cd.WaveHoltz(..., stiffness="lobatto", sweep="lattice", cell_stiffness=beta): the lattice march on csrc/kernels/wave_weights.hip /
wave_weights_f32.hip for  -div(beta grad U) - w^2 a^2 U = f,  beta constant on each element.

period and action on meshes of 8 x 8 to 12 x 10 cells, full and holed, against tests/wave_weights_reference.py (the dense K_beta
from the product's tables and the space's node lists, pinned in tests/test_wave_weights_host.py, in waveholtz_reference.Model with
lumped()'s m and h) at 1e-10 relative, the project's fp64 gate (GATE of tests/test_gpu_waveholtz_cells.py).  beta: an inclusion of
4, a strip of 0.25, random in [0.5, 2].  rk2 and rk4 / 4, a time ratio, time_ratio="coefficient" with the ratio asserted against
the rule max(1, ceil((1 - 1e-9) max_e sqrt(beta_e) / min_{g in e} a_g)), n_basis 3 to 6, absorbing and sound-hard walls, absent f
and z_in, a repeated period bit for bit.  fp32 as tests/test_gpu_waveholtz_f32.py holds it: within GATE_FACTOR = 4 x the distance of
the float32 numpy march (waveholtz_f32_reference.Model32) from the float64 model on the same case.

beta == 1 on a holed mesh is torch.equal to the same object without the argument, which runs wave_cells: the vertices of hole-8x8
on [-1, 1]^2 are exact in binary (h = 1 / 4), so cx = cy = 1 and both kernels see the same description.

solve: the full 8 x 8 grid with a 3 x 3-cell inclusion of beta = 4, rk2 at time ratio 2, GMRES(20).  The model's residual estimate
is 1.1565e-8 |b| after 16 Krylov steps and 2.6463e-9 |b| after 17 (measured on the CPU; a factor 4.4 per step; the true residual
after the cycle is 2.6463e-9 |b| too), so a tolerance can be a factor 1.9 from both; 5.5e-9, their geometric mean, is a factor
2.1 from each.  Checked here by running the model at 1.9 tol and at tol / 1.9 and asking for the same counts (19 matvecs in one
cycle: the first residual, 17 steps, the last residual); the device, whose action agrees with the model's to 1e-10, must then give
that count exactly, res_norm to 1e-8 |b| and the solution to 1e-8.

driver: waveholtz_solve --sweep lattice --inclusion i0 j0 i1 j1 beta; its refusals exit 2.
"""
import functools
import math
import re
import subprocess

import numpy as np
import pytest

import wave_weights_reference as ww
import waveholtz_f32_reference as w32
import waveholtz_reference as wr
from test_gpu_waveholtz_cells import GATE, GATE_FACTOR, MESHES as HOLED, mask, outer_faces as holed_outer_faces
from test_gpu_waveholtz_lattice import ROOT, SQUARE, dev

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

SOLVE_TOL = 5.5e-9

MESHES = dict(HOLED)
MESHES["full-8x8"] = (8, 8, SQUARE, [])
MESHES["full-11x9"] = (11, 9, (-1.0, 1.2, 0.0, 1.5), [])


@functools.lru_cache(maxsize=None)
def case_and_space(name, nb, smooth=False):
    import cuddhelmholtz_amd as cd
    import oracle

    nx, ny, (ax, bx, ay, by), holes = MESHES[name]
    present = mask(nx, ny, *holes)
    mesh = cd.Mesh2D.grid_cells(nx, ax, bx, ny, ay, by, present) if holes else cd.Mesh2D.uniform_rect(nx, ax, bx, ny, ay, by)
    d = oracle.Discretization(oracle.Mesh(mesh.vertices(), mesh.elements()), nb)
    c = wr.Case(d, 2 * math.pi * max(nx, ny) / 10, wr.smooth_coefficient(d) if smooth else None)
    fem = cd.H1Space(mesh, cd.Basis(nb))
    assert fem.size() == d.ndof and mesh.n_elem() == int(present.sum())
    return c, fem, mesh, present


@functools.lru_cache(maxsize=None)
def beta_of(name, kind):
    """beta per element (the present cells in ascending order), read-only"""
    nx, ny, _, holes = MESHES[name]
    present = mask(nx, ny, *holes)
    grid = np.ones((ny, nx))
    if kind == "inclusion":
        grid[ny // 2 - 1: ny // 2 + 2, nx // 2 - 2: nx // 2 + 1] = 4.0
    elif kind == "strip":
        grid[:, 1:3] = 0.25
    elif kind == "random":
        grid[:] = np.random.default_rng(nx + 10 * ny).uniform(0.5, 2.0, (ny, nx))
    elif kind != "ones":
        raise KeyError(kind)
    beta = grid[present].copy()
    assert kind == "ones" or 1 < len(np.unique(beta))
    beta.setflags(write=False)
    return beta


def outer_faces(name, mesh):
    if MESHES[name][3]:
        return holed_outer_faces(name, mesh)
    # a full rectangle: the left and the lower side absorbing, the others sound-hard
    _, _, (ax, bx, ay, by), _ = MESHES[name]
    xy, edges = mesh.vertices(), mesh.edges()
    keep = [int(e) for e in mesh.boundary_edges()
            if all(abs(xy[edges[e, k]][0] - ax) < 1e-12 for k in (1, 2)) or all(abs(xy[edges[e, k]][1] - ay) < 1e-12 for k in (1, 2))]
    assert 0 < len(keep) < len(mesh.boundary_edges())
    return np.asarray(keep, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def stiffness(name, nb, kind):
    c, fem, mesh, _ = case_and_space(name, nb)
    nx, ny, (ax, bx, ay, by), _ = MESHES[name]
    K = ww.weighted_stiffness(fem, (bx - ax) / nx, (by - ay) / ny, beta_of(name, kind))
    K.setflags(write=False)
    return K


def make(name, nb, kind, smooth=False, scheme="rk2", coarsen=None, time_ratio=1, outer=False, precision="f64"):
    import cuddhelmholtz_amd as cd

    c, fem, mesh, _ = case_and_space(name, nb, smooth)
    beta = beta_of(name, kind)
    faces = outer_faces(name, mesh) if outer else None
    W = cd.WaveHoltz(c.omega, c.h_a, fem, integrator=scheme, coarsen=coarsen, time_ratio=time_ratio, stiffness="lobatto", faces=faces, sweep="lattice",
                     precision=precision, cell_stiffness=beta)
    info = W.info()
    assert info["sweep"] == "lattice" and info["precision"] == precision and info["launch"] == "sweep"
    ratio = ww.beta_ratio(c.h_a, fem.global_indices(), beta) if time_ratio == "coefficient" else time_ratio
    M = ww.model(c, stiffness(name, nb, kind), scheme, info["coarsen"], ratio, faces)
    assert (info["nt"], info["ratio"], info["integrator"]) == (M.nt, ratio, scheme)
    assert info["sweeps_per_period"] == M.nt * (2 if scheme == "rk2" else 4) and math.isclose(info["dt"], M.dt, rel_tol=1e-15)
    return W, M, c


def kernel_name(nb, f32=False):
    return f"wave_weights nb{nb}" + (" f32" if f32 else "") + ("" if nb in (4, 5) else " (run-time n_basis)")


PERIOD_CASES = {
    # id: (mesh, n_basis, beta, smooth a, scheme, coarsen, time_ratio, outer faces only, the ratio "coefficient" must give)
    "full-inclusion-rk2-ratio2": ("full-8x8", 4, "inclusion", False, "rk2", None, 2, False, None),
    "full-inclusion-rk4-coefficient": ("full-8x8", 4, "inclusion", False, "rk4", 4, "coefficient", False, 2),
    "full-strip-rk2": ("full-8x8", 4, "strip", False, "rk2", None, 1, False, None),
    "full-11x9-random-nb5-sound-hard": ("full-11x9", 5, "random", False, "rk4", 4, 2, True, None),
    "hole-strip-rk4-sound-hard": ("hole-8x8", 4, "strip", False, "rk4", 4, 1, True, None),
    "hole-random-smooth-a-coefficient": ("hole-8x8", 4, "random", True, "rk4", 4, "coefficient", False, None),
    "L-inclusion-smooth-a-coefficient": ("L-8x8", 4, "inclusion", True, "rk2", None, "coefficient", False, None),
    "two-holes-random-nb3": ("two-holes-12x10", 3, "random", False, "rk2", None, 2, True, None),
    "notch-strip-nb5": ("notch-10x8", 5, "strip", False, "rk4", 4, 1, False, None),
    "corners-random-nb6": ("corners-9x8", 6, "random", False, "rk4", 4, 2, False, None),
}


@pytest.mark.parametrize("name", list(PERIOD_CASES))
def test_period_and_action_match_the_model(cuda, name):
    import torch

    mesh_name, nb, kind, smooth, scheme, coarsen, time_ratio, outer, want_ratio = PERIOD_CASES[name]
    W, M, c = make(mesh_name, nb, kind, smooth, scheme, coarsen, time_ratio, outer)
    info = W.info()
    assert info["stiffness_kernel"] == kernel_name(nb)
    if want_ratio is not None:
        assert info["ratio"] == want_ratio
    if time_ratio == "coefficient":
        assert info["ratio"] >= wr.coefficient_ratio(c.h_a)
    n = W.size()
    assert n == 2 * c.d.ndof
    z = np.random.default_rng(11).standard_normal(n)
    out, y = (torch.full((n,), float("nan"), dtype=torch.float64, device=cuda) for _ in range(2))
    W.period(dev(z, cuda), dev(c.f, cuda), out)
    W.action(dev(z, cuda), y)
    torch.cuda.synchronize()
    want, want_action = M.period(z, c.f), M.action(z)
    err, err_action = wr.rel(out.cpu().numpy(), want), wr.rel(y.cpu().numpy(), want_action)
    # what beta changes: the same march on the plain Laplacian
    plain = wr.Model(c.K_lobatto, M.m, M.h, c.h_a, c.omega, M.nt, scheme).period(z, c.f)
    print(f"waveholtz weights period {name}: ndof={c.d.ndof} nt={M.nt} ratio={info['ratio']} kernel={info['stiffness_kernel']!r} vs model: period "
          f"{err:.3e} action {err_action:.3e}; the model against beta = 1: {wr.rel(want, plain):.3e}")
    assert np.isfinite(want).all() and np.abs(want).max() < 1e6  # a stable march
    assert err < GATE and err_action < GATE
    assert wr.rel(want, plain) > 1e-3  # beta matters


F32_CASES = ["full-inclusion-rk2-ratio2", "full-strip-rk2", "hole-strip-rk4-sound-hard", "two-holes-random-nb3", "notch-strip-nb5", "corners-random-nb6"]


@pytest.mark.parametrize("name", F32_CASES)
def test_f32_period_and_action_within_four_times_the_fp32_models_error(cuda, name):
    import torch

    mesh_name, nb, kind, smooth, scheme, coarsen, time_ratio, outer, _ = PERIOD_CASES[name]
    W64, M, c = make(mesh_name, nb, kind, smooth, scheme, coarsen, time_ratio, outer)
    W, _, _ = make(mesh_name, nb, kind, smooth, scheme, coarsen, time_ratio, outer, precision="f32")
    info, info64 = W.info(), W64.info()
    assert info["stiffness_kernel"] == kernel_name(nb, True)
    assert {k: v for k, v in info.items() if k not in ("precision", "stiffness_kernel")} == \
           {k: v for k, v in info64.items() if k not in ("precision", "stiffness_kernel")}
    M32 = w32.Model32.of(M)
    n = W.size()
    z = np.random.default_rng(11).standard_normal(n)
    out, y, out64 = (torch.full((n,), float("nan"), dtype=torch.float64, device=cuda) for _ in range(3))
    W.period(dev(z, cuda), dev(c.f, cuda), out)
    W.action(dev(z, cuda), y)
    W64.period(dev(z, cuda), dev(c.f, cuda), out64)
    torch.cuda.synchronize()
    want, want_action = M.period(z, c.f), M.action(z)
    ref, ref_action = wr.rel(M32.period(z, c.f), want), wr.rel(M32.action(z), want_action)
    err, err_action = wr.rel(out.cpu().numpy(), want), wr.rel(y.cpu().numpy(), want_action)
    print(f"waveholtz weights f32 period {name}: ndof={c.d.ndof} nt={M.nt} kernel={info['stiffness_kernel']!r} vs float64 model: period {err:.3e} "
          f"(Model32 {ref:.3e}, {err / ref:.2f} x) action {err_action:.3e} (Model32 {ref_action:.3e}, {err_action / ref_action:.2f} x)")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(y).all())
    assert 1e-8 < ref < 1e-5 and 1e-8 < ref_action < 1e-5  # an fp32 march, and a sound one
    assert err < GATE_FACTOR * ref and err_action < GATE_FACTOR * ref_action
    assert not torch.equal(out, out64)
    assert torch.equal(out, out.float().double())  # what leaves a period was a float


@pytest.mark.parametrize("scheme,precision", [("rk2", "f64"), ("rk4", "f64"), ("rk2", "f32"), ("rk4", "f32")])
def test_beta_one_gives_the_bits_of_the_cells_kernels(cuda, scheme, precision):
    import torch

    import cuddhelmholtz_amd as cd

    c, fem, mesh, _ = case_and_space("hole-8x8", 4)
    n = 2 * fem.size()
    z, f = dev(np.random.default_rng(5).standard_normal(n), cuda), dev(c.f, cuda)
    outs = {}
    for beta, kernel in ((None, "wave_cells nb4"), (np.ones(mesh.n_elem()), "wave_weights nb4")):
        W = cd.WaveHoltz(c.omega, c.h_a, fem, integrator=scheme, stiffness="lobatto", sweep="lattice", precision=precision, cell_stiffness=beta)
        assert W.info()["stiffness_kernel"] == kernel + (" f32" if precision == "f32" else "")
        out, y = (torch.full((n,), float("nan"), dtype=torch.float64, device=cuda) for _ in range(2))
        W.period(z, f, out)
        W.action(z, y)
        outs[kernel] = (out, y, {k: v for k, v in W.info().items() if k != "stiffness_kernel"})
    (a, ya, ia), (b, yb, ib) = outs.values()
    assert ia == ib
    assert torch.equal(a, b) and torch.equal(ya, yb) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


@pytest.mark.parametrize("scheme,precision", [("rk2", "f64"), ("rk4", "f64"), ("rk4", "f32")])
def test_absent_arguments_and_reproducibility_bit_for_bit(cuda, scheme, precision):
    import torch

    W, _, c = make("hole-8x8", 4, "random", scheme=scheme, time_ratio=2, precision=precision)
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
    W.period(z, f, a)
    W.period(z, f, b)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    W.action(zero, a)
    assert float(a.abs().max()) == 0.0


@functools.lru_cache(maxsize=None)
def solve_reference():
    c, fem, _, _ = case_and_space("full-8x8", 4)
    M = ww.model(c, stiffness("full-8x8", 4, "inclusion"), "rk2", 1, 2)
    z, info = M.gmres(c.f, 20, 100, SOLVE_TOL)
    around = [M.gmres(c.f, 20, 100, t)[1] for t in (1.9 * SOLVE_TOL, SOLVE_TOL / 1.9)]
    return M, z, info, around


def test_solve_with_an_inclusion_follows_the_model(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    W, _, c = make("full-8x8", 4, "inclusion", time_ratio=2)
    n = W.size()
    b, z, u = (torch.zeros(n, dtype=torch.float64, device=cuda) for _ in range(3))
    W.rhs(dev(c.f, cuda), b)
    out = cd.gmres(n, z, W, b, 20, 100, SOLVE_TOL)
    W.solution(z, u)
    M, zm, info, around = solve_reference()
    # every comparison the model's GMRES makes against tol is a factor 1.9 away from it
    for other in around:
        assert (other["num_matvec"], other["num_iter"], other["success"]) == (info["num_matvec"], info["num_iter"], True)
    assert (info["num_matvec"], info["num_iter"]) == (19, 1)
    res, ref = np.asarray(out.res_norm), np.asarray(info["res_norm"])
    res_err = float(np.abs(res - ref).max() / ref[0]) if res.shape == ref.shape else float("inf")
    direct = M.direct(c.f)
    sol_err, distance, model_distance = wr.rel(u.cpu().numpy(), M.solution(zm)), wr.rel(u.cpu().numpy(), direct), wr.rel(M.solution(zm), direct)
    print(f"waveholtz weights solve full-8x8 inclusion: matvecs {out.num_matvec} cycles {out.num_iter} (model {info['num_matvec']} / {info['num_iter']}, "
          f"counts at 1.9 tol and tol / 1.9: {[o['num_matvec'] for o in around]}) res_norm vs model {res_err:.3e} of |b|, solution vs model "
          f"{sol_err:.3e}, vs direct {distance:.3e} (model {model_distance:.3e})")
    assert out.success and info["success"]
    assert (out.num_matvec, out.num_iter) == (info["num_matvec"], info["num_iter"])
    assert abs(res[0] - ref[0]) < 1e-8 * ref[0] and res_err < 1e-8
    assert sol_err < 1e-8
    assert distance < 2 * model_distance


def test_pair_launches_and_the_operator_form_are_refused_on_the_live_path(cuda):
    import cuddhelmholtz_amd as cd

    c, fem, mesh, _ = case_and_space("full-8x8", 4)
    beta = beta_of("full-8x8", "inclusion")
    with pytest.raises(ValueError, match="launch"):
        cd.WaveHoltz(c.omega, c.h_a, fem, stiffness="lobatto", sweep="lattice", launch="pair", cell_stiffness=beta)
    with pytest.raises(ValueError, match="cell_stiffness"):
        cd.WaveHoltz(c.omega, c.h_a, fem, stiffness="lobatto", sweep="operator", cell_stiffness=beta)
    # and the objects beside it are what they were
    assert cd.WaveHoltz(c.omega, c.h_a, fem, stiffness="lobatto", sweep="lattice", launch="pair").info()["stiffness_kernel"] == "wave_pair nb4"
    assert cd.WaveHoltz(c.omega, c.h_a, fem, stiffness="lobatto", sweep="lattice").info()["stiffness_kernel"] == "wave_lattice nb4"
    for precision in ("f64", "f32"):
        W = cd.WaveHoltz(c.omega, c.h_a, fem, stiffness="lobatto", sweep="lattice", precision=precision, cell_stiffness=beta)
        assert W.info()["stiffness_kernel"] == kernel_name(4, precision == "f32")
    _, fem3, mesh3, _ = case_and_space("two-holes-12x10", 3)
    W = cd.WaveHoltz(1.0, np.ones(fem3.size()), fem3, stiffness="lobatto", sweep="lattice", cell_stiffness=np.full(mesh3.n_elem(), 0.5))
    assert W.info()["stiffness_kernel"] == "wave_weights nb3 (run-time n_basis)"


def test_waveholtz_solve_driver_with_an_inclusion(cuda):
    exe = ROOT / "build" / "examples" / "waveholtz_solve"
    if not exe.exists():
        pytest.fail("build/examples/waveholtz_solve missing: run __graft_entry__.build()")
    base = [str(exe), "16", "4", "3.2", "20", "100", "1e-6", "--integrator", "rk4", "--coarsen", "4", "--time-ratio", "2"]
    timing = ("t_rhs", "t_gmres", "ms_per_period", "us_per_sweep")
    runs = []
    for extra in (["--inclusion", "6", "5", "10", "9", "4"], ["--inclusion", "6", "5", "10", "9", "4"],
                  ["--inclusion", "6", "5", "10", "9", "4", "--void", "0", "0", "2", "1", "--inclusion", "12", "12", "14", "16", "0.5"], []):
        r = subprocess.run(base + ["--sweep", "lattice"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("waveholtz_solve")]
        assert len(lines) == 1
        print(lines[0])
        runs.append({k: v for k, v in re.findall(r"(\S+)=(\"[^\"]*\"|\S+)", lines[0]) if k not in timing})
    first, second, with_void, plain = runs
    assert first == second  # stable under repetition: the same line but for the times
    assert first["kernel"] == '"wave_weights nb4"' and int(first["success"]) == 1 and float(first["rel_res"]) < 1e-6
    assert with_void["kernel"] == '"wave_weights nb4"' and int(with_void["success"]) == 1 and int(with_void["cells"]) == 16 * 16 - 2
    assert plain["kernel"] == '"wave_lattice nb4"' and int(plain["success"]) == 1
    assert (first["ndof"], first["nt"]) == (plain["ndof"], plain["nt"]) and first["|u|"] != plain["|u|"] and with_void["|u|"] != first["|u|"]
    for bad, flag in ((["--sweep", "lattice", "--inclusion", "6", "5", "17", "9", "4"], "--inclusion"),
                      (["--sweep", "lattice", "--inclusion", "6", "5", "6", "9", "4"], "--inclusion"),
                      (["--sweep", "lattice", "--inclusion", "6", "5", "10", "9", "0"], "--inclusion"),
                      (["--sweep", "lattice", "--inclusion", "6", "5", "10", "9", "-2"], "--inclusion"),
                      (["--sweep", "lattice", "--inclusion", "6", "5", "10", "9"], "--inclusion"),
                      (["--inclusion", "6", "5", "10", "9", "4"], "--inclusion"),
                      (["--sweep", "lattice", "--launch", "pair", "--inclusion", "6", "5", "10", "9", "4"], "--launch pair")):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and flag in r.stderr and not r.stdout.strip(), (bad, r.returncode, r.stderr)
