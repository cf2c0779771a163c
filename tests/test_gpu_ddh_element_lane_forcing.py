"""The two places at which the element-lane march of kernel 5 applies the trace sources ("Sources in the first pass
only"): forcing 1, in both half steps of every WaveHoltz pass, and forcing 2, in the first pass only, the later passes running a
time loop without source terms and adding what the first returned (DDH.set_forcing / cuddh_hip_ddh_plan_set_forcing).  a = 1
and the inputs of tests/test_gpu_ddh_mfma_layout.py's case throughout; the helpers of tests/test_gpu_ddh_element_lane_chains.py.

  * parity: rhs / action / postprocess at 8 x 8 and 16 x 16 elements with form 2, order 2 and forcing 2 set against the fp64
    oracle, gated as a new summation order is: below 2 x PARENT5 against the oracle, and below 2 x PARENT5 plus forcing 1's own
    distance between the two forcings of one plan (triangle inequality).  A lost or doubled r is wrong by O(1);
  * one WaveHoltz iteration: forcing 2 is forcing 1 bit for bit (the first pass is the same loop);
  * bitwise properties of forcing 2 at 32 x 32 elements (64 subdomains): a repeated run, ranges of lengths 13, 1, 13, 2 and the
    rest, a shuffled list cut at an odd place, a launch that holds issue priority, form 3 against form 2 (the owner rule),
    with and without x, and action(2 lambda) == 2 action(lambda);
  * today's schedule is still there: with a forced form or order, forcing auto and 1 report 1 and give the traces the plan gave
    before any forcing was set, and 1 and 2 differ somewhere at 8 x 8;
  * selection (plans only): auto is 2 exactly where form and order are auto and auto gave the paired chains, and 2 is refused
    where the plan cannot take the paired chains.
Every distance is printed (`pytest -s`).
"""
import numpy as np
import pytest

import test_gpu_ddh_element_lane as E
import test_gpu_ddh_element_lane_chains as CH
import test_gpu_ddh_mfma_layout as L
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu


def _make(cd, nx, forcing):
    """form 2 and order 2 forced, and the forcing"""
    F, _ = E.make(cd, nx, 2)
    F.set_chain_order(2)
    assert F.info()["kernel"] == 5 and F.sweep_form() == 2 and F.chain_order() == 2 and F.forcing() == 1
    F.set_forcing(forcing)
    assert F.forcing() == forcing
    return F


@pytest.mark.parametrize("nx", [8, 16])
def test_first_pass_only_vs_fp64_oracle_and_every_pass(cuda, nx):
    import torch

    import cuddhelmholtz_amd as cd

    c = L.case(nx)
    ref = L.oracle_outputs(c)
    F = _make(cd, nx, 2)
    out2 = E.outputs(torch, cuda, F, c)
    F.set_forcing(1)
    assert F.sweep_form() == 2 and F.chain_order() == 2 and F.forcing() == 1
    out1 = E.outputs(torch, cuda, F, c)
    names = ("rhs", "action", "postprocess")
    e2 = tuple(rel(a, r) for a, r in zip(out2, ref))
    e1 = tuple(rel(a, r) for a, r in zip(out1, ref))
    e21 = tuple(float(np.linalg.norm(a - b) / np.linalg.norm(r)) for a, b, r in zip(out2, out1, ref))
    for i, nm in enumerate(names):
        print(f"[{nx}x{nx}, a=1] {nm}: forcing 2 vs fp64 oracle {e2[i]:.4e} (parent's kernel 5 {E.PARENT5[nx][i]:.3e}, gate 2 x), "
              f"forcing 1 vs oracle {e1[i]:.4e}, forcing 2 vs forcing 1 {e21[i]:.4e}")
    for i, nm in enumerate(names):
        assert e2[i] < 2 * E.PARENT5[nx][i], (nm, e2[i], E.PARENT5[nx][i])
        assert e21[i] < 2 * E.PARENT5[nx][i] + e1[i], (nm, e21[i], e1[i])


def _traces(torch, cuda, F, f, lam):
    """the local traces of sources only, traces only (the form without x), both"""
    nd = F.info()["n_domains"]
    out = []
    for x, l in ((f, None), (None, lam), (f, lam)):
        t = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
        F.local_traces(0, nd, x, l, t)
        assert t.abs().max().item() > 0
        out.append(t)
    return out


def test_one_waveholtz_iteration_is_bitwise_the_same_in_both(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 8
    c = L.case(nx)
    f = to_dev(torch, c[3], cuda)
    lam = to_dev(torch, c[5].astype(np.float32), cuda)
    F = _make(cd, nx, 2)
    F.set_wh_iters(1)
    first = _traces(torch, cuda, F, f, lam)
    F.set_forcing(1)
    every = _traces(torch, cuda, F, f, lam)
    for a, b in zip(first, every):
        assert torch.equal(a, b)


def test_first_pass_only_launch_partitions_owner_rule_and_scaling_are_bitwise(cuda):
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
        assert F.sweep_form() == 3 and F.chain_order() == 2 and F.forcing() == 2
        other = torch.zeros_like(plain)
        F.local_traces(0, nd, x, l, other)
        F.set_sweep_form(2)
        assert torch.equal(other, plain)

    y1, y2 = torch.zeros_like(lam), torch.zeros_like(lam)
    F.action(lam, y1)
    F.action(2.0 * lam, y2)  # I - T is linear; scaling by 2 is exact in fp32
    assert y1.abs().max().item() > 0 and torch.equal(y2, 2.0 * y1)


def test_the_sources_in_every_pass_are_still_there(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 8
    c = L.case(nx)
    f = to_dev(torch, c[3], cuda)
    lam = to_dev(torch, c[5].astype(np.float32), cuda)
    for form, order in ((2, 2), (3, 2), (None, 2)):  # a forced form with the paired chains asked for, a forced order alone
        F, _ = E.make(cd, nx, form)
        F.set_chain_order(order)
        if form is None:  # 4 subdomains: the order waits on the matrix form, and so does the forcing
            assert F.sweep_form() == 1 and F.chain_order() == 0 and F.forcing() == 0
            continue
        assert F.sweep_form() == form and F.chain_order() == 2 and F.forcing() == 1
        before = _traces(torch, cuda, F, f, lam)
        F.set_forcing(1)
        assert F.forcing() == 1
        every = _traces(torch, cuda, F, f, lam)
        F.set_forcing(0)
        assert F.forcing() == 1
        auto = _traces(torch, cuda, F, f, lam)
        for a, b, d in zip(before, every, auto):
            assert torch.equal(a, b) and torch.equal(a, d)
        F.set_forcing(2)
        assert F.forcing() == 2
        first = _traces(torch, cuda, F, f, lam)
        differ = [int((a != b).sum().item()) for a, b in zip(before, first)]
        print(f"[8x8, form {form}] entries in which forcings 1 and 2 differ (sources only, traces only, both): {differ} of {before[0].numel()}")
        assert any(differ)  # the switch does something
    # the pinned chains: the forcing is idle, whatever is stored
    F, _ = E.make(cd, nx, 2)
    assert F.chain_order() == 1 and F.forcing() == 0
    pinned = _traces(torch, cuda, F, f, lam)
    F.set_forcing(2)
    assert F.chain_order() == 1 and F.forcing() == 0
    for a, b in zip(pinned, _traces(torch, cuda, F, f, lam)):
        assert torch.equal(a, b)


def test_selection_of_the_forcing(cuda):
    import cuddhelmholtz_amd as cd

    F = CH._ddh(cd, 256, 512)  # 8,192 subdomains: auto takes the element-lane form, the paired chains and the first pass only
    assert F.info()["kernel"] == 5 and F.info()["n_domains"] == E.AUTO_MIN_DOMAINS
    assert F.sweep_form() == 2 and F.chain_order() == 2 and F.forcing() == 2
    F.set_forcing(1)
    assert F.chain_order() == 2 and F.forcing() == 1
    F.set_forcing(0)
    assert F.forcing() == 2
    F.set_sweep_form(2)  # forced: pinned, nothing to choose
    assert F.sweep_form() == 2 and F.chain_order() == 1 and F.forcing() == 0
    F.set_chain_order(2)  # a forced form and order keep their bits
    assert F.chain_order() == 2 and F.forcing() == 1
    F.set_forcing(2)
    assert F.forcing() == 2
    F.set_sweep_form(3)
    assert F.sweep_form() == 3 and F.chain_order() == 2 and F.forcing() == 2
    F.set_forcing(0)
    assert F.forcing() == 1
    F.set_sweep_form(0)
    assert F.sweep_form() == 2 and F.chain_order() == 2 and F.forcing() == 1  # the order is still asked for
    F.set_chain_order(0)
    assert F.sweep_form() == 2 and F.chain_order() == 2 and F.forcing() == 2  # auto for all three again
    for bad in (-1, 3):
        with pytest.raises(RuntimeError):
            F.set_forcing(bad)
    assert F.forcing() == 2  # a refusal leaves the plan as it was
    F.set_sweep_form(1)
    assert F.sweep_form() == 1 and F.forcing() == 0
    F.set_forcing(2)  # accepted on the matrix form: takes effect with the paired chains
    assert F.forcing() == 0
    F.set_sweep_form(3)
    F.set_chain_order(2)
    assert F.forcing() == 2

    F = CH._ddh(cd, 256, 256)  # 4,096 subdomains: the matrix form
    assert F.info()["kernel"] == 5 and F.sweep_form() == 1 and F.chain_order() == 0 and F.forcing() == 0


def test_refusals_of_the_first_pass_only(cuda):
    import cuddhelmholtz_amd as cd

    ratios = np.ones(16, dtype=np.int32)  # the refusing plans of test_refusals_of_the_paired_chains
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
        assert F.forcing() == 0, what
        with pytest.raises(RuntimeError):
            F.set_forcing(2)
            pytest.fail(f"forcing 2 was accepted by the {what} plan")
        assert F.forcing() == 0, what
        F.set_forcing(1)  # 0 and 1 are accepted by every plan
        F.set_forcing(0)
        assert F.forcing() == 0, what
    F = CH._ddh(cd, 16, 16)
    assert F.info()["kernel"] == 5
    for bad in (-1, 3):
        with pytest.raises(RuntimeError):
            F.set_forcing(bad)
    F.set_forcing(2)  # a kernel-5 plan with tables, one grid, RK2: accepted below the threshold too
    assert F.sweep_form() == 1 and F.forcing() == 0
