"""DDH(integrator="rk4", coarsen=c) on the device: the local solves step with classical RK4 on a coarser grid.

Shapes: those of tests/test_gpu_ddh_time_grids.py (16 x 16 elements on [-1,1]^2, n_basis 4, omega = 2 pi 16 / 10, mesh grid nt
about 800, so coarsen 4 marches about 200 steps; blocks of 4 x 4 with that file's RATIOS put four step counts into one workgroup
of the wavefront kernels, blocks of 8 x 8 four step counts into four workgroups of kernel 1).  The reference is the numpy
restatement tests/ddh_rk.Restatement, pinned to the oracle in tests/test_ddh_rk4.py, computed once per case and shared.

  * parity of rhs / action (written slots) / postprocess, one grid and RATIOS: fp64 kernels 1, 2, 8 (and 1 at block 8) at 1e-10,
    the project's fp64 gate; fp32 kernels 1 and 5 (matrix form), the fp32 kernels that have an RK4 form, at 4 x the distance of
    the float32 restatement to the float64 one, computed here (the floor rule of tests/test_gpu_ddh_block_size.py);
  * bitwise: the full launch against ranges plus a scrambled list under RK4 with ratios; integrator="rk2" against a plan built
    without the argument;
  * selection: what auto picks under RK4 (the table of DESIGN 4.3) and what is refused (kernels 3, 4, 6, 7, 11 on request,
    kernel 5's element-lane form): a refused request raises, it never runs RK2;
  * stability: config 3's disk window on the mesh grid's ratios, coarsen 2: the growth factors are the restatement's, <= 1.05
    where RK2 gives 1e5 to 1e7;
  * physics: a varying coefficient, time_step="coefficient" on top of coarsen 4, 20 WaveHoltz iterations,
    rhs -> GMRES -> postprocess against ddh_general.fixed_point.
Every distance is printed (`pytest -s`).
"""
import math

import numpy as np
import pytest

import ddh_general as dg
import ddh_rk as rk
import ddh_time_grids as tg
from test_baseline_regime import NB, power_iteration
from test_ddh_rk4 import STABLE_COARSEN
from test_gpu_ddh_time_grids import RATIOS, entry_points
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu

NAMES = ("rhs", "action", "postprocess")
FP64_GATE = 1e-10
NX = rk.NX
COARSEN = 4
# distance of the restatement's own flow (rk4, coarsen 4, ratios 3, 2, 3, 2, 20 WaveHoltz iterations, GMRES(120) to 1e-6) to
# ddh_general.fixed_point on tests/ddh_time_grids.physics_case, measured once on the CPU with
#   python profiles/tools/ddh_rk4_restatement_flow.py 20 4        (114 matvecs; the per-subdomain RK2 oracle on the mesh grid: 5.8895e-06)
RESTATEMENT_FLOW_TO_FIXED_POINT = 5.7299e-07


def make(cd, block, precision, kernel, ratios=None, **kw):
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(NX, -1.0, 1.0, NX, -1.0, 1.0), cd.Basis(NB))
    kw.setdefault("integrator", "rk4")
    kw.setdefault("coarsen", COARSEN)
    F = cd.DDH(2 * math.pi * NX / 10, np.ones(fem.size()), fem, NX, NX, precision=precision, kernel=kernel, block=block,
               time_step="mesh" if ratios is None else np.asarray(ratios, dtype=np.int32), **kw)
    return F, fem


def product_outputs(torch, cuda, F, c):
    b, y, u = (t.cpu().numpy().astype(np.float64) for t in entry_points(torch, cuda, F, c.fh, c.lam, c.d.ndof))
    return b, y[c.written], u


GRIDS = [pytest.param(False, id="one-grid"), pytest.param(True, id="ratios")]


@pytest.mark.parametrize("with_ratios", GRIDS)
@pytest.mark.parametrize("kernel,block", [(1, 4), (2, 4), (8, 4), (1, 8)])
def test_fp64_parity_with_the_rk4_restatement(cuda, kernel, block, with_ratios):
    import torch

    import cuddhelmholtz_amd as cd

    c = rk.sweep_case(block)
    ratios = RATIOS[block] if with_ratios else None
    ref = rk.sweep_outputs(block, "rk4", COARSEN, ratios, "f64")
    F, _ = make(cd, block, "f64", kernel, ratios)
    assert F.info()["kernel"] == kernel and F.integrator() == ("rk4", COARSEN)
    assert F.info()["nt"] == rk.base_steps(c.nt_mesh, COARSEN) and F.size() == c.size
    assert list(F.time_ratios()) == list(ratios or [1] * c.n_domains)
    e = [rel(a, r) for a, r in zip(product_outputs(torch, cuda, F, c), ref)]
    for nm, x in zip(NAMES, e):
        print(f"[block {block}, rk4 coarsen {COARSEN}, ratios {list(ratios) if ratios else 1}, f64 kernel {kernel}] {nm}: vs fp64 restatement {x:.3e} "
              f"(gate {FP64_GATE:.0e})")
    assert all(np.linalg.norm(r) > 0 for r in ref)
    assert all(x <= FP64_GATE for x in e), e


@pytest.mark.parametrize("with_ratios", GRIDS)
@pytest.mark.parametrize("kernel,block,form", [(1, 4, None), (5, 4, 1), (1, 8, None)])
def test_fp32_parity_with_the_rk4_restatement(cuda, kernel, block, form, with_ratios):
    import torch

    import cuddhelmholtz_amd as cd

    c = rk.sweep_case(block)
    ratios = RATIOS[block] if with_ratios else None
    ref = rk.sweep_outputs(block, "rk4", COARSEN, ratios, "f64")
    floor = [rel(a, r) for a, r in zip(rk.sweep_outputs(block, "rk4", COARSEN, ratios, "f32"), ref)]
    F, _ = make(cd, block, "f32", kernel, ratios)
    if form is not None:
        F.set_sweep_form(form)
        assert F.sweep_form() == form
    assert F.info()["kernel"] == kernel and F.integrator() == ("rk4", COARSEN)
    e = [rel(a, r) for a, r in zip(product_outputs(torch, cuda, F, c), ref)]
    for nm, x, fl in zip(NAMES, e, floor):
        print(f"[block {block}, rk4 coarsen {COARSEN}, ratios {list(ratios) if ratios else 1}, f32 kernel {kernel}] {nm}: floor (float32 restatement vs "
              f"float64) {fl:.3e}, gate 4 x; product vs float64 restatement {x:.3e} ({x / fl:.2f} x floor)")
    for nm, x, fl in zip(NAMES, e, floor):
        assert x <= 4 * fl, (nm, x, 4 * fl)


@pytest.mark.parametrize("precision,kernel,block", [("f32", 5, 4), ("f64", 2, 4), ("f64", 8, 4), ("f32", 1, 8)])
def test_launch_partitions_are_bitwise_the_full_launch_under_rk4(cuda, precision, kernel, block):
    import torch

    import cuddhelmholtz_amd as cd

    c = rk.sweep_case(block)
    F, _ = make(cd, block, precision, kernel, RATIOS[block])
    assert F.info()["kernel"] == kernel
    nd = c.n_domains
    f = to_dev(torch, c.fh, cuda)
    lam = to_dev(torch, c.lam.astype(np.float64 if F.f64 else np.float32), cuda)
    perm = np.random.default_rng(3).permutation(nd).astype(np.int32)
    cuts = (0, 1, nd // 2 + 1, nd)
    for x, l in ((f, None), (None, lam), (f, lam)):
        full = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
        F.local_traces(0, nd, x, l, full)  # the plan's order: longest first
        assert full.abs().max().item() > 0
        ranged = torch.zeros_like(full)
        for d0, d1 in zip(cuts[:-1], cuts[1:]):
            F.local_traces(d0, d1, x, l, ranged)
        assert torch.equal(ranged, full)
        listed = torch.zeros_like(full)
        for ids in (perm[: nd // 3], perm[nd // 3:]):
            F.local_traces_listed(to_dev(torch, ids, cuda), x, l, listed)
        assert torch.equal(listed, full)


@pytest.mark.parametrize("precision,kernel", [("f32", 5), ("f64", 2)])
def test_rk2_is_bitwise_the_plan_built_without_the_argument(cuda, precision, kernel):
    import torch

    import cuddhelmholtz_amd as cd

    c = rk.sweep_case(4)
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(NX, -1.0, 1.0, NX, -1.0, 1.0), cd.Basis(NB))
    F0 = cd.DDH(c.omega, c.h_a, fem, NX, NX, precision=precision, kernel=kernel)
    F1, _ = make(cd, 4, precision, kernel, integrator="rk2", coarsen=None)
    F4, _ = make(cd, 4, precision, kernel, integrator="rk4", coarsen=1)
    assert F0.info() == F1.info() and F1.integrator() == ("rk2", 1) and F4.info() == F0.info()
    out0, out1, out4 = (entry_points(torch, cuda, F, c.fh, c.lam, c.d.ndof) for F in (F0, F1, F4))
    for nm, a, b, d in zip(NAMES, out0, out1, out4):
        assert a.abs().max().item() > 0
        assert torch.equal(a, b), nm
        assert not torch.equal(a, d), nm  # the scheme was honoured: on the same grid RK4 is another march


def test_selection_and_refusals_under_rk4(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    # what auto picks ("Runge-Kutta 4"): (precision, block) -> kernel under rk2, under rk4
    for precision, block, k2, k4 in (("f32", 4, 5, 5), ("f64", 4, 3, 2), ("f32", 8, 11, 1), ("f64", 8, 1, 1), ("f32", 2, 1, 1)):
        assert make(cd, block, precision, 0, integrator="rk2", coarsen=None)[0].info()["kernel"] == k2
        for ratios in (None, np.ones((NX // block) ** 2, dtype=np.int32)):
            F, _ = make(cd, block, precision, 0, ratios)
            assert F.info()["kernel"] == k4, (precision, block, F.info()["kernel"])
            if k4 == 5:  # the matrix form, and the element-lane forms are refused
                assert F.sweep_form() == 1
                for form in (2, 3):
                    with pytest.raises(RuntimeError):
                        F.set_sweep_form(form)
                assert F.sweep_form() == 1
    # kernels without an RK4 form on request: refused on first use, never run as RK2
    c = rk.sweep_case(4)
    for precision, kernel, block in (("f32", 3, 4), ("f64", 3, 4), ("f32", 4, 4), ("f32", 11, 8)):
        assert make(cd, block, precision, kernel, integrator="rk2", coarsen=None)[0].info()["kernel"] == kernel
        F, _ = make(cd, block, precision, kernel)
        with pytest.raises(RuntimeError):
            F.info()
        lam = to_dev(torch, rk.sweep_case(block).lam.astype(np.float64 if F.f64 else np.float32), cuda)
        y = torch.zeros_like(lam)
        with pytest.raises(RuntimeError):
            F.action(lam, y)
        assert y.abs().max().item() == 0
    # n_basis 8, blocks of 2 x 2 elements: kernels 6 and 7
    fem8 = cd.H1Space(cd.Mesh2D.uniform_rect(4, -1.0, 1.0, 4, -1.0, 1.0), cd.Basis(8))
    ones8 = np.ones(fem8.size())

    def ddh8(precision, kernel, **kw):
        return cd.DDH(2 * math.pi * 4 / 10, ones8, fem8, 4, 4, precision=precision, kernel=kernel, **kw)

    assert ddh8("f32", 0).info()["kernel"] == 7 and ddh8("f64", 0).info()["kernel"] == 6  # today's choices
    assert ddh8("f32", 0, integrator="rk4").info()["kernel"] == 1 and ddh8("f64", 0, integrator="rk4").info()["kernel"] == 1
    for precision, kernel in (("f32", 7), ("f32", 6), ("f64", 6)):
        F = ddh8(precision, kernel, integrator="rk4")
        with pytest.raises(RuntimeError):
            F.info()
        lam = torch.ones(F.size(), dtype=F.trace_dtype, device=cuda)
        y = torch.zeros_like(lam)
        with pytest.raises(RuntimeError):
            F.action(lam, y)
        assert ddh8(precision, kernel).info()["kernel"] == kernel
    # 8,192 subdomains: the size at which auto takes kernel 5's element-lane form on an RK2 plan
    nx, ny = 512, 256
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, ny, -1.0, 1.0), cd.Basis(4))
    F = cd.DDH(16 * math.pi, np.ones(fem.size()), fem, nx, ny, integrator="rk4")
    assert F.info()["kernel"] == 5 and F.info()["n_domains"] == 8192 and F.sweep_form() == 1
    with pytest.raises(RuntimeError):
        F.set_sweep_form(2)


def test_product_is_stable_on_the_disk_window_on_the_mesh_grids_ratios(cuda):
    """config 3's disk window (tests/test_baseline_regime.py: |T| ~ 1e7 with RK2 on the mesh grid), ratios all 1, RK4"""
    import torch

    import cuddhelmholtz_amd as cd

    w, O, _ = tg.stability_window()
    ref = rk.stability_growth_rk4(STABLE_COARSEN)
    assert all(r <= 1.05 for r in ref)
    mesh = cd.Mesh2D.uniform_rect(w.nw, w.x0, w.x1, w.nw, w.y0, w.y1)
    fem = cd.H1Space(mesh, cd.Basis(NB))
    F = cd.DDH(w.omega, w.h_a, fem, w.nw, w.nw, precision="f64", kernel=2, integrator="rk4", coarsen=STABLE_COARSEN)
    assert F.info()["kernel"] == 2 and list(F.time_ratios()) == [1, 1, 1, 1] and F.info()["nt"] == 5120 // STABLE_COARSEN
    nd, tt = F.info()["n_domains"], F.trace_dtype

    def T(v):
        lam = torch.from_numpy(np.ascontiguousarray(v)).to(cuda).to(tt)
        out = torch.zeros_like(lam)
        F.local_traces(0, nd, None, lam, out)
        return out.double().cpu().numpy()

    got = power_iteration(T, F.size(), tg.STABILITY_STEPS, seed=1)
    print(f"config 3 disk window, rk4 coarsen {STABLE_COARSEN}, ratios all 1, f64 kernel 2: " + " ".join(f"{r:.9f}" for r in got)
          + " (restatement " + " ".join(f"{r:.9f}" for r in ref) + ")")
    assert all(g <= 1.05 for g in got)
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-9 * r, (got, ref)


def test_physics_rk4_on_coefficient_grids_converges_to_the_exact_local_solve_fixed_point(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    d, omega, h_a, fh, labels, n_domains, O, ratios = tg.physics_case()
    assert list(ratios) == [3, 2, 3, 2]
    want = dg.fixed_point(O.t, O.G, d.ndof, fh)
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(8, -1.0, 1.0, 8, -1.0, 1.0), cd.Basis(NB))
    F = cd.DDH(omega, h_a, fem, 8, 8, precision="f64", time_step="coefficient", integrator="rk4", coarsen=COARSEN)
    assert list(F.time_ratios()) == [3, 2, 3, 2] and F.info()["kernel"] == 2 and F.info()["nt"] == rk.base_steps(O.t.nt, COARSEN)
    F.set_wh_iters(20)
    n = F.size()
    f = to_dev(torch, fh, cuda)
    b = torch.zeros(n, dtype=F.trace_dtype, device=cuda)
    lam = torch.zeros_like(b)
    u = torch.zeros(2 * d.ndof, dtype=torch.float64, device=cuda)
    F.rhs(f, b)
    out = cd.gmres(n, lam, F, b, 120, 30, 1e-6)
    assert out.success, out.res_norm[-1] / out.res_norm[0]
    F.postprocess(lam, f, u)
    e = rel(u.cpu().numpy(), want)
    gate = 2 * RESTATEMENT_FLOW_TO_FIXED_POINT
    print(f"[8x8, a from 0.4 to 1, rk4 coarsen {COARSEN}, ratios {[int(r) for r in ratios]}, f64, 20 WaveHoltz iterations] {out.num_matvec} matvecs, "
          f"distance to the exact-local-solve fixed point {e:.4e} (the restatement's flow {RESTATEMENT_FLOW_TO_FIXED_POINT:.4e}, gate 2 x)")
    assert e <= gate, (e, gate)
