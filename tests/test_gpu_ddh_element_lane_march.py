"""The two ways in which the element-lane march of kernel 5 with the sources in the first pass only carries the velocity (DESIGN
4.3, "Scaled velocity"): march 1, q itself, and march 2, q / (2 hm) with the midpoint update folded into the head of the first
sweep's chains, 1 / m of it in each of the m copies of a shared node (DDH.set_march / cuddh_hip_ddh_plan_set_march).  The inputs
of tests/test_gpu_ddh_mfma_layout.py's case and the helpers of tests/test_gpu_ddh_element_lane_forcing.py.

  * parity: rhs / action / postprocess at 8 x 8 and 16 x 16 elements with form 2, order 2, forcing 2 and march 2 set against the
    fp64 oracle, gated as a new summation order is: below 2 x PARENT5 against the oracle, and below 2 x PARENT5 plus march 1's own
    distance between the two marches of one plan.  At 8 x 8 the plan is 2 x 2 subdomains: every subdomain touches the domain
    boundary and every multiplicity pattern occurs.  A wrong multiplicity or coefficient is wrong by O(1);
  * a coefficient that is not constant, smooth in [0.5, 1], at 8 x 8: march 2 against the fp64 oracle within 2 x the distance
    march 1 reaches in the same test (on the CPU the fp32 oracle gives |T lam| / |lam| = 0.96 to 0.99 over four applications
    of T on this case and stands 2.7e-7 / 5.4e-7 from the fp64 oracle in action / rhs: stable);
  * set_wh_iters 1, 2 and 5 at 8 x 8: each within 2 x PARENT5 of the oracle run with that count (the error is rounding that the
    passes accumulate, so fewer passes stay below the bound of five);
  * bitwise properties of march 2 at 32 x 32 elements (64 subdomains), with and without x: a repeated run, ranges of lengths 13,
    1, 13, 2 and the rest, a shuffled list cut at an odd place, a launch that holds issue priority, form 3 against form 2 (the
    owner rule: the copies of every shared node stay bit-equal under the 1 / m heads), and action(2 lambda) == 2 action(lambda);
  * today's march is still there: a forced (2, 2, 2) plan with march auto or 1 gives bit for bit what it gave before set_march
    was called and reports 1, and march 2 differs from it somewhere;
  * selection (plans only): auto is 2 exactly where form, order and forcing are auto and auto gave forcing 2; 2 is refused where
    forcing 2 is.
Every distance is printed (`pytest -s`).
"""
import numpy as np
import pytest

import oracle
import test_gpu_ddh_element_lane as E
import test_gpu_ddh_element_lane_chains as CH
import test_gpu_ddh_element_lane_forcing as FO
import test_gpu_ddh_mfma_layout as L
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu

NAMES = ("rhs", "action", "postprocess")


def _make(cd, nx, march, h_a=None):
    """form 2, order 2 and forcing 2 forced, and the march"""
    if h_a is None:
        F, _ = E.make(cd, nx, 2)
    else:
        import math

        fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(4))
        F = cd.DDH(2 * math.pi * nx / 10, h_a, fem, nx, nx, precision="f32")
        F.set_sweep_form(2)
    F.set_chain_order(2)
    F.set_forcing(2)
    assert F.info()["kernel"] == 5 and F.sweep_form() == 2 and F.chain_order() == 2 and F.forcing() == 2 and F.march() == 1
    F.set_march(march)
    assert F.march() == march and F.sweep_form() == 2 and F.chain_order() == 2 and F.forcing() == 2
    return F


def _both_marches(torch, cuda, cd, nx, c, h_a=None):
    F = _make(cd, nx, 2, h_a)
    out2 = E.outputs(torch, cuda, F, c)
    F.set_march(1)
    assert F.sweep_form() == 2 and F.chain_order() == 2 and F.forcing() == 2 and F.march() == 1
    return out2, E.outputs(torch, cuda, F, c)


@pytest.mark.parametrize("nx", [8, 16])
def test_scaled_march_vs_fp64_oracle_and_todays_march(cuda, nx):
    import torch

    import cuddhelmholtz_amd as cd

    c = L.case(nx)
    ref = L.oracle_outputs(c)
    out2, out1 = _both_marches(torch, cuda, cd, nx, c)
    e2 = tuple(rel(a, r) for a, r in zip(out2, ref))
    e1 = tuple(rel(a, r) for a, r in zip(out1, ref))
    e21 = tuple(float(np.linalg.norm(a - b) / np.linalg.norm(r)) for a, b, r in zip(out2, out1, ref))
    for i, nm in enumerate(NAMES):
        print(f"[{nx}x{nx}, a=1] {nm}: march 2 vs fp64 oracle {e2[i]:.4e} (parent's kernel 5 {E.PARENT5[nx][i]:.3e}, gate 2 x), "
              f"march 1 vs oracle {e1[i]:.4e}, march 2 vs march 1 {e21[i]:.4e}")
    for i, nm in enumerate(NAMES):
        assert e2[i] < 2 * E.PARENT5[nx][i], (nm, e2[i], E.PARENT5[nx][i])
        assert e21[i] < 2 * E.PARENT5[nx][i] + e1[i], (nm, e21[i], e1[i])


def smooth_coefficient(x, y):
    """in [0.5, 1]"""
    return 0.75 + 0.25 * np.sin(2.0 * x + 0.5) * np.cos(3.0 * y - 0.25)


def coefficient_case(nx):
    """L.case with smooth_coefficient, lumped-projected as bench.py projects its coefficient"""
    omega, d, _, fh, _, _, _ = L.case(nx)
    h_a = oracle.diag_inv_mass(d) * oracle.linear_functional(d, smooth_coefficient)
    assert 0.5 <= h_a.min() and h_a.max() <= 1.0 and h_a.max() - h_a.min() > 0.3
    O = oracle.DDH(d, nx, nx, omega, h_a, np.float64)
    n = O.size
    lam = np.random.default_rng(7).standard_normal(n)
    used = np.unique(O.t.B[O.t.B >= 0])
    lam[np.setdiff1d(np.arange(n), np.concatenate([used, used + O.t.n_lambda]))] = 0.0
    written = np.unique(O.t.B[:, 1, :][O.t.B[:, 1, :] >= 0])
    written = np.concatenate([written, written + O.t.n_lambda])
    return omega, d, h_a, fh, O, lam, written


def test_scaled_march_with_a_coefficient_that_is_not_constant(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 8
    c = coefficient_case(nx)
    ref = L.oracle_outputs(c)
    out2, out1 = _both_marches(torch, cuda, cd, nx, c, h_a=c[2])
    e2 = tuple(rel(a, r) for a, r in zip(out2, ref))
    e1 = tuple(rel(a, r) for a, r in zip(out1, ref))
    for i, nm in enumerate(NAMES):
        print(f"[8x8, smooth a in [0.5, 1]] {nm}: march 2 vs fp64 oracle {e2[i]:.4e}, march 1 vs oracle {e1[i]:.4e} (gate: 2 x march 1)")
    for i, nm in enumerate(NAMES):
        assert e1[i] < 1e-4, (nm, e1[i])  # march 1 has digits here, so twice its distance is a gate
        assert e2[i] < 2 * e1[i], (nm, e2[i], e1[i])


@pytest.mark.parametrize("wh_iters", [1, 2, 5])
def test_scaled_march_with_another_number_of_waveholtz_iterations(cuda, wh_iters):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 8
    c = L.case(nx)
    oracle.ddh_set_wh_iters(wh_iters)
    try:
        ref = L.oracle_outputs(c)
    finally:
        oracle.ddh_set_wh_iters(5)
    F = _make(cd, nx, 2)
    F.set_wh_iters(wh_iters)
    out2 = E.outputs(torch, cuda, F, c)
    e2 = tuple(rel(a, r) for a, r in zip(out2, ref))
    for i, nm in enumerate(NAMES):
        print(f"[8x8, a=1, {wh_iters} WaveHoltz iterations] {nm}: march 2 vs fp64 oracle {e2[i]:.4e} (gate 2 x {E.PARENT5[nx][i]:.3e})")
    for i, nm in enumerate(NAMES):
        assert e2[i] < 2 * E.PARENT5[nx][i], (nm, e2[i], E.PARENT5[nx][i])


def test_scaled_march_launch_partitions_owner_rule_and_scaling_are_bitwise(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 32  # 8 x 8 subdomains
    c = L.case(nx)
    F = _make(cd, nx, 2)
    nd = F.info()["n_domains"]
    assert nd == 64
    f = to_dev(torch, c[3], cuda)
    lam = to_dev(torch, c[5].astype(np.float32), cuda)
    perm = np.random.default_rng(3).permutation(nd).astype(np.int32)
    cut = (nd // 3) | 1
    assert cut % 4 and (nd - cut) % 4
    for x, l in ((f, None), (None, lam), (f, lam)):  # sources only, traces only (the form without x), both
        plain = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
        F.local_traces(0, nd, x, l, plain)
        assert plain.abs().max().item() > 0
        again = torch.zeros_like(plain)
        F.local_traces(0, nd, x, l, again)
        assert torch.equal(again, plain)
        ranged = torch.zeros_like(plain)
        for d0, d1 in ((0, 13), (13, 14), (14, 27), (27, 29), (29, nd)):  # lengths 13, 1, 13, 2, nd - 29: every tail shape
            F.local_traces(d0, d1, x, l, ranged)
        assert torch.equal(ranged, plain)
        listed = torch.zeros_like(plain)
        for ids in (perm[:cut], perm[cut:]):
            F.local_traces_listed(to_dev(torch, ids, cuda), x, l, listed)
        assert torch.equal(listed, plain)
        F.set_wave_priority(True)
        held = torch.zeros_like(plain)
        F.local_traces(0, nd // 2 - 1, x, l, held)
        F.local_traces_listed(to_dev(torch, np.arange(nd // 2 - 1, nd, dtype=np.int32), cuda), x, l, held)
        F.set_wave_priority(False)
        assert torch.equal(held, plain)
        # the owner rule: the other copy of every shared node publishes, same bits
        F.set_sweep_form(3)
        assert F.sweep_form() == 3 and F.chain_order() == 2 and F.forcing() == 2 and F.march() == 2
        other = torch.zeros_like(plain)
        F.local_traces(0, nd, x, l, other)
        F.set_sweep_form(2)
        assert torch.equal(other, plain)

    y1, y2 = torch.zeros_like(lam), torch.zeros_like(lam)
    F.action(lam, y1)
    F.action(2.0 * lam, y2)  # I - T is linear; scaling by 2 is exact in fp32
    assert y1.abs().max().item() > 0 and torch.equal(y2, 2.0 * y1)


def test_todays_march_is_still_there(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 8
    c = L.case(nx)
    f = to_dev(torch, c[3], cuda)
    lam = to_dev(torch, c[5].astype(np.float32), cuda)
    for form in (2, 3):
        F, _ = E.make(cd, nx, form)
        F.set_chain_order(2)
        F.set_forcing(2)
        assert F.sweep_form() == form and F.chain_order() == 2 and F.forcing() == 2 and F.march() == 1
        before = FO._traces(torch, cuda, F, f, lam)
        F.set_march(1)
        assert F.march() == 1
        asked = FO._traces(torch, cuda, F, f, lam)
        F.set_march(0)
        assert F.march() == 1
        auto = FO._traces(torch, cuda, F, f, lam)
        for a, b, d in zip(before, asked, auto):
            assert torch.equal(a, b) and torch.equal(a, d)
        F.set_march(2)
        assert F.march() == 2 and F.forcing() == 2 and F.chain_order() == 2 and F.sweep_form() == form
        scaled = FO._traces(torch, cuda, F, f, lam)
        differ = [int((a != b).sum().item()) for a, b in zip(before, scaled)]
        print(f"[8x8, form {form}] entries in which marches 1 and 2 differ (sources only, traces only, both): {differ} of {before[0].numel()}")
        assert any(differ)  # the switch does something
    # forcing 1: the march is idle, whatever is stored
    F, _ = E.make(cd, nx, 2)
    F.set_chain_order(2)
    assert F.forcing() == 1 and F.march() == 0
    every = FO._traces(torch, cuda, F, f, lam)
    F.set_march(2)
    assert F.forcing() == 1 and F.march() == 0
    for a, b in zip(every, FO._traces(torch, cuda, F, f, lam)):
        assert torch.equal(a, b)


def test_selection_of_the_march(cuda):
    import cuddhelmholtz_amd as cd

    F = CH._ddh(cd, 256, 512)  # 8,192 subdomains, all auto: the element-lane form, the paired chains, the first pass only, scaled
    assert F.info()["kernel"] == 5 and F.info()["n_domains"] == E.AUTO_MIN_DOMAINS
    assert F.sweep_form() == 2 and F.chain_order() == 2 and F.forcing() == 2 and F.march() == 2
    F.set_march(1)
    assert F.forcing() == 2 and F.march() == 1
    F.set_march(0)
    assert F.march() == 2
    F.set_forcing(2)  # the forcing auto gives, but asked for: its bits stay
    assert F.forcing() == 2 and F.march() == 1
    F.set_forcing(1)
    assert F.forcing() == 1 and F.march() == 0
    F.set_forcing(0)
    assert F.forcing() == 2 and F.march() == 2
    F.set_chain_order(2)  # the same for the order
    assert F.chain_order() == 2 and F.forcing() == 1 and F.march() == 0
    F.set_chain_order(0)
    F.set_sweep_form(2)  # forced: pinned, nothing to choose
    assert F.sweep_form() == 2 and F.chain_order() == 1 and F.forcing() == 0 and F.march() == 0
    F.set_chain_order(2)
    F.set_forcing(2)
    assert F.forcing() == 2 and F.march() == 1
    F.set_march(2)
    assert F.march() == 2
    F.set_sweep_form(3)
    assert F.sweep_form() == 3 and F.chain_order() == 2 and F.forcing() == 2 and F.march() == 2
    for bad in (-1, 3):
        with pytest.raises(RuntimeError):
            F.set_march(bad)
        with pytest.raises(RuntimeError):
            F.set_forcing(bad)
    assert F.march() == 2 and F.forcing() == 2  # a refusal leaves the plan as it was
    F.set_sweep_form(0), F.set_chain_order(0), F.set_forcing(0), F.set_march(0)
    assert F.sweep_form() == 2 and F.chain_order() == 2 and F.forcing() == 2 and F.march() == 2  # auto for all four again
    F.set_sweep_form(1)
    assert F.sweep_form() == 1 and F.forcing() == 0 and F.march() == 0
    F.set_march(2)  # accepted on the matrix form: takes effect with forcing 2
    assert F.march() == 0

    F = CH._ddh(cd, 256, 256)  # 4,096 subdomains: the matrix form
    assert F.info()["kernel"] == 5 and F.sweep_form() == 1 and F.chain_order() == 0 and F.forcing() == 0 and F.march() == 0


def test_refusals_of_the_scaled_march(cuda):
    import cuddhelmholtz_amd as cd

    ratios = np.ones(16, dtype=np.int32)  # the refusing plans of test_refusals_of_the_first_pass_only
    ratios[::7] = 2
    plans = {
        "n_basis 8": lambda: CH._ddh(cd, 16, 16, nb=8),
        "fp64": lambda: CH._ddh(cd, 16, 16, precision="f64"),
        "kernel 3": lambda: CH._ddh(cd, 16, 16, kernel=3),
        "time_step": lambda: CH._ddh(cd, 16, 16, time_step=ratios),
        "kernel 13": lambda: CH._ddh(cd, 16, 16, kernel=13),
        "rk4": lambda: CH._ddh(cd, 16, 16, integrator="rk4"),
    }
    for what, make in plans.items():
        F = make()
        assert F.march() == 0, what
        with pytest.raises(RuntimeError):
            F.set_march(2)
            pytest.fail(f"march 2 was accepted by the {what} plan")
        assert F.march() == 0, what
        F.set_march(1)  # 0 and 1 are accepted by every plan
        F.set_march(0)
        assert F.march() == 0, what
    F = CH._ddh(cd, 16, 16)
    assert F.info()["kernel"] == 5
    for bad in (-1, 3):
        with pytest.raises(RuntimeError):
            F.set_march(bad)
    F.set_march(2)  # a kernel-5 plan with tables, one grid, RK2: accepted below the threshold too
    assert F.sweep_form() == 1 and F.march() == 0
