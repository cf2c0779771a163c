"""DDH kernel 5's element-lane form with the time loop on register pairs (v_pk_fma_f32): every half of a pair
runs the chain of fp32 FMAs the unpacked loop ran for that node, so rhs, action and postprocess are bitwise those of the
commit before.  The expected outputs were recorded once with that commit's library on an MI355X by
profiles/tools/record_element_lane_parent.py (which builds its inputs with this module's functions) into
tests/golden/element_lane_parent/*.npz; the comparisons are np.array_equal, not tolerances.

  (a) 8 x 8 elements, a = 1, test_gpu_ddh_mfma_layout.case(8): 4 subdomains, exactly one wavefront;
  (b) 16 x 32 elements on the square, h_x != h_y so Bx != By (a swapped pair orientation or coefficient pair shows), a smooth
      coefficient with values in [1, 1.5] (every per-node constant differs between the halves of a pair; the local solves stay
      non-expansive), launched as the ranges (0, 13), (13, 14), (14, 32) so that padding rows occur;
  (c) the plan of (b) under form 3 (the other copy of a shared node publishes) and holding issue priority: the fixture of (b).
postprocess adds the contributions of the 2 or 4 subdomains that share a dof atomically, in fp64, in whatever order the
device takes them.  The summands are fp32 values, so a sum of up to four of them is exact in fp64, and then independent of
the order, as long as their exponents lie within 29 bits of each other (53 - 24); a summand smaller than that beside its
neighbours' would be rounded away in one order and not in another.  ASSUMED here: the copies of a shared dof carry values
of like magnitude (they are partition-of-unity shares of one smooth field).  The recording tool checks that two runs of the
parent's library agree bitwise before it writes a fixture; a mismatch in postprocess alone, on shared dofs alone, would
point at this assumption and not at the kernel.
"""
import math
from pathlib import Path

import numpy as np
import pytest

import oracle
import test_gpu_ddh_element_lane as E
import test_gpu_ddh_mfma_layout as L
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

FIXTURES = Path(__file__).resolve().parent / "golden" / "element_lane_parent"
NAMES = ("rhs", "action", "postprocess")
RANGES_B = ((0, 13), (13, 14), (14, 32))
NX_B, NY_B = 16, 32


def smooth_coefficient(x, y):
    """in [1, 1.5], no symmetry about an element's or a subdomain's centre lines"""
    return 1.25 + 0.25 * np.sin(2.3 * x + 0.4) * np.cos(1.7 * y - 0.9)


def outputs_a(cd, torch, cuda, form=2):
    """case (a): the entry points rhs, action, postprocess on L.case(8), kernel 5 in the element-lane form"""
    F, _ = E.make(cd, 8, form)
    assert F.info()["kernel"] == 5 and F.sweep_form() == form and F.info()["n_domains"] == 4
    return E.outputs(torch, cuda, F, L.case(8))


def plan_b(cd):
    """case (b): (the plan on form 2, its sources f, its traces lambda) -- fixed seeds, nothing drawn from the device"""
    omega = 2 * math.pi * NX_B / 10
    d = oracle.Discretization(oracle.Mesh.uniform_rect(NX_B, -1.0, 1.0, NY_B, -1.0, 1.0), 4)
    h_a = d.nodal(smooth_coefficient)
    assert h_a.min() >= 1.0 and h_a.max() <= 1.5 and h_a.max() - h_a.min() > 0.4
    fh = np.concatenate([oracle.linear_functional(d, oracle.gaussians(omega)), 0.1 * oracle.linear_functional(d, oracle.mass_poly)])
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(NX_B, -1.0, 1.0, NY_B, -1.0, 1.0), cd.Basis(4))
    assert fem.size() == d.ndof
    F = cd.DDH(omega, h_a, fem, NX_B, NY_B, precision="f32")
    F.set_sweep_form(2)
    assert F.info()["kernel"] == 5 and F.sweep_form() == 2 and F.info()["n_domains"] == RANGES_B[-1][1]
    lam = np.random.default_rng(11).standard_normal(F.size()).astype(np.float32)
    return F, fem, fh, lam


def outputs_b(torch, cuda, F, fem, fh, lam_h):
    """rhs, action and postprocess as DDH forms them (traces of f; lambda - traces of lambda; the local solutions), one
    launch per range of RANGES_B"""
    f, lam = to_dev(torch, fh, cuda), to_dev(torch, lam_h, cuda)
    b = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
    y = torch.zeros_like(b)
    u = torch.zeros(2 * fem.size(), dtype=torch.float64, device=cuda)
    for d0, d1 in RANGES_B:
        F.local_traces(d0, d1, f, None, b)
        F.local_traces(d0, d1, None, lam, y)
        F.local_solution(d0, d1, lam, f, u, False)
    y.mul_(-1.0).add_(lam)
    return b.cpu().numpy(), y.cpu().numpy(), u.cpu().numpy()


def expected(name):
    with np.load(FIXTURES / f"{name}.npz") as z:
        return tuple(z[n] for n in NAMES)


def check(out, ref, what):
    for nm, a, r in zip(NAMES, out, ref):
        assert a.dtype == r.dtype and a.shape == r.shape, (what, nm, a.dtype, r.dtype, a.shape, r.shape)
        assert np.abs(r).max() > 0, (what, nm)
        differ = int(np.count_nonzero(a != r))
        print(f"[{what}] {nm}: {a.size} values, {differ} differ from the parent's, max |difference| {np.abs(a.astype(np.float64) - r).max():.3e}")
        assert np.array_equal(a, r), (what, nm, differ)


def test_one_wavefront_is_bitwise_the_parent(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    check(outputs_a(cd, torch, cuda), expected("case_a"), "8x8, a=1")


@pytest.fixture(scope="module")
def case_b(cuda):
    import cuddhelmholtz_amd as cd

    return plan_b(cd)


def test_rectangles_and_smooth_coefficient_are_bitwise_the_parent(cuda, case_b):
    import torch

    check(outputs_b(torch, cuda, *case_b), expected("case_b"), "16x32, smooth a, ranges")


def test_other_copy_and_issue_priority_are_bitwise_the_parent(cuda, case_b):
    import torch

    F = case_b[0]
    try:
        F.set_sweep_form(3)
        assert F.sweep_form() == 3 and F.info()["kernel"] == 5
        check(outputs_b(torch, cuda, *case_b), expected("case_b"), "16x32, form 3")
        F.set_sweep_form(2)
        F.set_wave_priority(True)
        check(outputs_b(torch, cuda, *case_b), expected("case_b"), "16x32, form 2, issue priority")
        F.set_sweep_form(3)
        check(outputs_b(torch, cuda, *case_b), expected("case_b"), "16x32, form 3, issue priority")
    finally:
        F.set_wave_priority(False)
        F.set_sweep_form(2)
