"""What the scaled march of kernel 5's element-lane form carries as the velocity ("Carried head"): head 1, qs = q / (2 hm),
whose product with the head coefficient alpha / m opens the first sweep's chain in every step, and head 2, that product itself, so
that the chain opens on the state and the multiplication is gone (DDH.set_head / cuddh_hip_ddh_plan_set_head).  Everything here
runs head 2 on plans forced to (form, order, forcing, march) = (2, 2, 2, 2); the helpers are those of
tests/test_gpu_ddh_element_lane_march.py and tests/test_gpu_ddh_element_lane_rectangles.py.

  * parity: rhs / action / postprocess at 8 x 8 elements (4 subdomains in one wavefront: every multiplicity 1, 2, 4 and trace nodes
    on every side) and at 16 x 16 with a = 1 against the fp64 oracle, below 2 x PARENT5, the gate of every new summation order;
  * a smooth coefficient in [0.5, 1] at 8 x 8: within 2 x the distance head 1 reaches in the same test;
  * set_wh_iters 1, 2 and 5 at 8 x 8, each below 2 x PARENT5 of the oracle run with that count.  With one iteration nothing is
    parked and the interior pairs, which have no Hi, carry 2 qs: the same gates;
  * `rect` (hy = hx / 2) and `tall` (hy = 2 hx) of tests/ddh_metric_cases.py, 6 subdomains and so a wavefront with padding rows:
    relative l2 and max norm <= 4 x the fp32 oracle's own distance to the fp64 oracle, that file's rule;
  * bitwise at 32 x 32 elements (64 subdomains), sources only, traces only and both: a repeated run, ranges of lengths 13, 1, 13, 2
    and the rest, a shuffled list cut at an odd place, a launch that holds issue priority, form 3 against form 2 (the copies of a
    shared node carry one Y: alpha / m is the same float in all of them), and action(2 lambda) == 2 action(lambda), since doubling
    is exact in every step of the linear march;
  * set_head(1) gives bit for bit what the march gave before the attribute existed: the traces of the build before it, recorded
    on an MI355X in tests/golden/ddh_head/march2_before_8x8.npz by profiles/tools/record_element_lane_head_parent.py, for forms 2
    and 3; head 2 differs from them somewhere;
  * selection (plans only): auto is 2 wherever march 2 is in effect, forced or not; head() is 0 elsewhere; 2 is refused where
    march 2 is; -1 and 3 always; a refusal leaves the plan as it was.
Every distance is printed (`pytest -s`).
"""
from pathlib import Path

import numpy as np
import pytest

import ddh_metric_cases as mc
import oracle
import test_gpu_ddh_element_lane as E
import test_gpu_ddh_element_lane_chains as CH
import test_gpu_ddh_element_lane_forcing as FO
import test_gpu_ddh_element_lane_march as M
import test_gpu_ddh_element_lane_rectangles as RE
import test_gpu_ddh_mfma_layout as L
from ddh_metric_cases import FLOOR_FACTOR
from test_gpu_ddh_metrics import entry_points
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu

NAMES = ("rhs", "action", "postprocess")
GOLDEN = Path(__file__).parent / "golden" / "ddh_head" / "march2_before_8x8.npz"


def _make(cd, nx, head, h_a=None):
    """(2, 2, 2, 2) forced, and the head"""
    F = M._make(cd, nx, 2, h_a)
    assert F.head() == 2  # auto carries the head under a forced march 2 too
    F.set_head(head)
    assert F.head() == head and (F.sweep_form(), F.chain_order(), F.forcing(), F.march()) == (2, 2, 2, 2)
    return F


def _both_heads(torch, cuda, cd, nx, c, h_a=None):
    F = _make(cd, nx, 2, h_a)
    out2 = E.outputs(torch, cuda, F, c)
    F.set_head(1)
    assert F.head() == 1 and F.march() == 2
    return out2, E.outputs(torch, cuda, F, c)


@pytest.mark.parametrize("nx", [8, 16])
def test_carried_head_vs_fp64_oracle(cuda, nx):
    import torch

    import cuddhelmholtz_amd as cd

    c = L.case(nx)
    ref = L.oracle_outputs(c)
    out2, out1 = _both_heads(torch, cuda, cd, nx, c)
    e2 = tuple(rel(a, r) for a, r in zip(out2, ref))
    e1 = tuple(rel(a, r) for a, r in zip(out1, ref))
    e21 = tuple(float(np.linalg.norm(a - b) / np.linalg.norm(r)) for a, b, r in zip(out2, out1, ref))
    for i, nm in enumerate(NAMES):
        print(f"[{nx}x{nx}, a=1] {nm}: head 2 vs fp64 oracle {e2[i]:.4e} (parent's kernel 5 {E.PARENT5[nx][i]:.3e}, gate 2 x), "
              f"head 1 vs oracle {e1[i]:.4e}, head 2 vs head 1 {e21[i]:.4e}")
    for i, nm in enumerate(NAMES):
        assert e2[i] < 2 * E.PARENT5[nx][i], (nm, e2[i], E.PARENT5[nx][i])
        assert e21[i] > 0, nm


def test_carried_head_with_a_coefficient_that_is_not_constant(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 8
    c = M.coefficient_case(nx)
    ref = L.oracle_outputs(c)
    out2, out1 = _both_heads(torch, cuda, cd, nx, c, h_a=c[2])
    e2 = tuple(rel(a, r) for a, r in zip(out2, ref))
    e1 = tuple(rel(a, r) for a, r in zip(out1, ref))
    for i, nm in enumerate(NAMES):
        print(f"[8x8, smooth a in [0.5, 1]] {nm}: head 2 vs fp64 oracle {e2[i]:.4e}, head 1 vs oracle {e1[i]:.4e} (gate: 2 x head 1)")
    for i, nm in enumerate(NAMES):
        assert e1[i] < 1e-4, (nm, e1[i])  # head 1 has digits here, so twice its distance is a gate
        assert e2[i] < 2 * e1[i], (nm, e2[i], e1[i])


@pytest.mark.parametrize("wh_iters", [1, 2, 5])
def test_carried_head_with_another_number_of_waveholtz_iterations(cuda, wh_iters):
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
        print(f"[8x8, a=1, {wh_iters} WaveHoltz iterations] {nm}: head 2 vs fp64 oracle {e2[i]:.4e} (gate 2 x {E.PARENT5[nx][i]:.3e})")
    for i, nm in enumerate(NAMES):
        assert e2[i] < 2 * E.PARENT5[nx][i], (nm, e2[i], E.PARENT5[nx][i])


@pytest.mark.parametrize("family", ["rect", "tall"])
def test_carried_head_on_rectangles_vs_oracle(cuda, family):
    import torch

    import cuddhelmholtz_amd as cd

    c = mc.case(family, RE.NB, RE.BLOCK)
    missed = []
    for variant in ((2, 2, 2, 2), (3, 2, 2, 2)):
        F = RE.make(cd, c, variant)
        assert F.head() == 2 and F.info()["n_domains"] == 6
        row = RE.distances(entry_points(torch, cuda, F, c), c.ref, c.floor)
        assert RE.settings(F) == variant and F.head() == 2
        for nm, (e2, r2, emax, rmax), (fl2, fmax) in zip(NAMES, row, c.floor):
            print(f"[{c.name}] {variant} head 2 {nm}: vs fp64 oracle l2 {e2:.3e}, floor {fl2:.3e}, ratio {r2:.2f}; max {emax:.3e}, floor {fmax:.3e}, "
                  f"ratio {rmax:.2f} (gate {FLOOR_FACTOR:.0f})")
            if not (e2 <= FLOOR_FACTOR * fl2 and emax <= FLOOR_FACTOR * fmax):
                missed.append((variant, nm, e2, emax))
    assert not missed, missed


def test_carried_head_launch_partitions_owner_rule_and_scaling_are_bitwise(cuda):
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
        assert (F.sweep_form(), F.chain_order(), F.forcing(), F.march(), F.head()) == (3, 2, 2, 2, 2)
        other = torch.zeros_like(plain)
        F.local_traces(0, nd, x, l, other)
        F.set_sweep_form(2)
        assert torch.equal(other, plain)

    y1, y2 = torch.zeros_like(lam), torch.zeros_like(lam)
    F.action(lam, y1)
    F.action(2.0 * lam, y2)  # I - T is linear; scaling by 2 is exact in fp32, in Y = fma(alpha / m, z, Y) as anywhere
    assert y1.abs().max().item() > 0 and torch.equal(y2, 2.0 * y1)


def test_head_1_is_the_march_as_it_was(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 8
    c = L.case(nx)
    f = to_dev(torch, c[3], cuda)
    lam = to_dev(torch, c[5].astype(np.float32), cuda)
    golden = np.load(GOLDEN)
    for form in (2, 3):
        F, _ = E.make(cd, nx, form)
        F.set_chain_order(2)
        F.set_forcing(2)
        F.set_march(2)
        assert (F.sweep_form(), F.chain_order(), F.forcing(), F.march(), F.head()) == (form, 2, 2, 2, 2)
        carried = FO._traces(torch, cuda, F, f, lam)
        F.set_head(1)
        assert F.head() == 1 and F.march() == 2
        multiplied = FO._traces(torch, cuda, F, f, lam)
        for i, t in enumerate(multiplied):
            before = golden[f"form{form}_{i}"]
            assert before.dtype == np.float32 and np.abs(before).max() > 0
            assert np.array_equal(t.cpu().numpy().view(np.uint32), before.view(np.uint32)), (form, i)
        F.set_head(0)
        assert F.head() == 2
        for a, b in zip(carried, FO._traces(torch, cuda, F, f, lam)):
            assert torch.equal(a, b)
        differ = [int((a != b).sum().item()) for a, b in zip(multiplied, carried)]
        print(f"[8x8, form {form}] entries in which heads 1 and 2 differ (sources only, traces only, both): {differ} of {multiplied[0].numel()}")
        assert all(differ)  # the switch does something, in the form with x and in the action form
    # march 1: the head is idle, whatever is stored
    F, _ = E.make(cd, nx, 2)
    F.set_chain_order(2)
    F.set_forcing(2)
    assert F.march() == 1 and F.head() == 0
    plain = FO._traces(torch, cuda, F, f, lam)
    F.set_head(2)
    assert F.march() == 1 and F.head() == 0
    for a, b in zip(plain, FO._traces(torch, cuda, F, f, lam)):
        assert torch.equal(a, b)


def test_selection_of_the_head(cuda):
    import cuddhelmholtz_amd as cd

    F = CH._ddh(cd, 256, 512)  # 8,192 subdomains, all auto
    assert F.info()["kernel"] == 5 and F.info()["n_domains"] == E.AUTO_MIN_DOMAINS
    assert RE.settings(F) == (2, 2, 2, 2) and F.head() == 2
    F.set_head(1)
    assert RE.settings(F) == (2, 2, 2, 2) and F.head() == 1
    F.set_head(0)
    assert F.head() == 2
    F.set_march(1)
    assert F.march() == 1 and F.head() == 0
    F.set_march(2)  # asked for: the head is carried all the same
    assert F.march() == 2 and F.head() == 2
    F.set_march(0)
    F.set_forcing(2)  # the forcing auto gives, but asked for: march 1, nothing to carry
    assert F.forcing() == 2 and F.march() == 1 and F.head() == 0
    F.set_forcing(0)
    F.set_sweep_form(2)
    RE.force(F, (2, 2, 2, 2))
    assert F.head() == 2
    F.set_sweep_form(3)
    assert RE.settings(F) == (3, 2, 2, 2) and F.head() == 2
    for bad in (-1, 3):
        with pytest.raises(RuntimeError):
            F.set_head(bad)
    assert RE.settings(F) == (3, 2, 2, 2) and F.head() == 2  # a refusal leaves the plan as it was
    F.set_head(1)
    for bad in (-1, 3):
        with pytest.raises(RuntimeError):
            F.set_head(bad)
    assert F.head() == 1
    F.set_sweep_form(0), F.set_chain_order(0), F.set_forcing(0), F.set_march(0), F.set_head(0)
    assert RE.settings(F) == (2, 2, 2, 2) and F.head() == 2  # auto for all five again
    F.set_sweep_form(1)
    assert F.sweep_form() == 1 and F.march() == 0 and F.head() == 0
    F.set_head(2)  # accepted on the matrix form: takes effect with march 2
    assert F.head() == 0

    F = CH._ddh(cd, 256, 256)  # 4,096 subdomains: the matrix form
    assert F.info()["kernel"] == 5 and F.sweep_form() == 1 and F.march() == 0 and F.head() == 0


def test_refusals_of_the_carried_head(cuda):
    import cuddhelmholtz_amd as cd

    ratios = np.ones(16, dtype=np.int32)  # the refusing plans of test_refusals_of_the_scaled_march
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
        assert F.head() == 0, what
        with pytest.raises(RuntimeError):
            F.set_head(2)
            pytest.fail(f"head 2 was accepted by the {what} plan")
        assert F.head() == 0, what
        F.set_head(1)  # 0 and 1 are accepted by every plan
        F.set_head(0)
        assert F.head() == 0, what
    F = CH._ddh(cd, 16, 16)
    assert F.info()["kernel"] == 5
    for bad in (-1, 3):
        with pytest.raises(RuntimeError):
            F.set_head(bad)
    F.set_head(2)  # a kernel-5 plan with tables, one grid, RK2: accepted below the threshold too
    assert F.sweep_form() == 1 and F.head() == 0
