"""The two summation orders of the element-lane form's in-lane products ("The paired chains"): order 1, pinned, the
chains of the node-by-node loop bit for bit, and order 2, paired, in which both halves of a register pair meet every term
at the same place (DDH.set_chain_order / cuddh_hip_ddh_plan_set_chain_order).  a = 1 and the inputs of
tests/test_gpu_ddh_mfma_layout.py's case throughout.

  * parity: rhs / action / postprocess at 8 x 8 and 16 x 16 elements with form 2 and order 2 forced against the fp64 oracle,
    gated as tests/test_gpu_ddh_element_lane.py gates a new summation order: below 2 x PARENT5 against the oracle, and below
    2 x PARENT5 plus the pinned order's own distance between the two orders of one plan (triangle inequality).  A crossed
    op_sel or a wrong coefficient pair is wrong by O(1);
  * bitwise properties of order 2 at 32 x 32 elements (64 subdomains): a repeated run, ranges of lengths 13, 1, 13, 2 and the
    rest, a shuffled list cut at an odd place, a launch that holds issue priority, form 3 against form 2 (the owner rule),
    with and without x, and action(2 lambda) == 2 action(lambda);
  * the pinned order is still there: form 2 forced with order auto or 1 reports order 1 and gives the traces the plan gave
    before any order was set, and orders 1 and 2 differ somewhere at 8 x 8;
  * selection (plans only): auto is paired exactly where auto chose the form, a forced form is pinned unless order 2 is asked
    for, and order 2 is refused where the plan cannot take it.
Every distance is printed (`pytest -s`).
"""
import math

import numpy as np
import pytest

import test_gpu_ddh_element_lane as E
import test_gpu_ddh_mfma_layout as L
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nx", [8, 16])
def test_paired_chains_vs_fp64_oracle_and_pinned_chains(cuda, nx):
    import torch

    import cuddhelmholtz_amd as cd

    c = L.case(nx)
    ref = L.oracle_outputs(c)
    F, _ = E.make(cd, nx, 2)
    F.set_chain_order(2)
    assert F.info()["kernel"] == 5 and F.sweep_form() == 2 and F.chain_order() == 2
    out2 = E.outputs(torch, cuda, F, c)
    F.set_chain_order(1)
    assert F.sweep_form() == 2 and F.chain_order() == 1
    out1 = E.outputs(torch, cuda, F, c)
    names = ("rhs", "action", "postprocess")
    e2 = tuple(rel(a, r) for a, r in zip(out2, ref))
    e1 = tuple(rel(a, r) for a, r in zip(out1, ref))
    e21 = tuple(float(np.linalg.norm(a - b) / np.linalg.norm(r)) for a, b, r in zip(out2, out1, ref))
    for i, nm in enumerate(names):
        print(f"[{nx}x{nx}, a=1] {nm}: paired chains vs fp64 oracle {e2[i]:.4e} (parent's kernel 5 {E.PARENT5[nx][i]:.3e}, gate 2 x), "
              f"pinned chains vs oracle {e1[i]:.4e}, paired vs pinned {e21[i]:.4e}")
    for i, nm in enumerate(names):
        assert e2[i] < 2 * E.PARENT5[nx][i], (nm, e2[i], E.PARENT5[nx][i])
        assert e21[i] < 2 * E.PARENT5[nx][i] + e1[i], (nm, e21[i], e1[i])


def test_paired_chains_launch_partitions_owner_rule_and_scaling_are_bitwise(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 32  # 8 x 8 subdomains
    c = L.case(nx)
    F, _ = E.make(cd, nx, 2)
    F.set_chain_order(2)
    nd = F.info()["n_domains"]
    assert nd == 64 and F.sweep_form() == 2 and F.chain_order() == 2
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
        assert F.sweep_form() == 3 and F.chain_order() == 2
        other = torch.zeros_like(plain)
        F.local_traces(0, nd, x, l, other)
        F.set_sweep_form(2)
        assert torch.equal(other, plain)

    y1, y2 = torch.zeros_like(lam), torch.zeros_like(lam)
    F.action(lam, y1)
    F.action(2.0 * lam, y2)  # I - T is linear; scaling by 2 is exact in fp32
    assert y1.abs().max().item() > 0 and torch.equal(y2, 2.0 * y1)


def test_the_pinned_chains_are_still_there(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 8
    c = L.case(nx)
    f = to_dev(torch, c[3], cuda)
    lam = to_dev(torch, c[5].astype(np.float32), cuda)
    F, _ = E.make(cd, nx, 2)
    nd = F.info()["n_domains"]

    def traces():
        out = []
        for x, l in ((f, None), (None, lam), (f, lam)):
            t = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
            F.local_traces(0, nd, x, l, t)
            assert t.abs().max().item() > 0
            out.append(t)
        return out

    assert F.sweep_form() == 2 and F.chain_order() == 1  # a forced form under order auto: pinned
    before = traces()
    F.set_chain_order(1)
    assert F.chain_order() == 1
    pinned = traces()
    F.set_chain_order(0)
    assert F.chain_order() == 1
    auto = traces()
    for a, b, d in zip(before, pinned, auto):
        assert torch.equal(a, b) and torch.equal(a, d)
    F.set_chain_order(2)
    assert F.chain_order() == 2
    paired = traces()
    differ = [int((a != b).sum().item()) for a, b in zip(before, paired)]
    print(f"[8x8] entries in which orders 1 and 2 differ (sources only, traces only, both): {differ} of {before[0].numel()}")
    assert any(differ)  # the switch does something


def _ddh(cd, nx, ny, nb=4, **kw):
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, ny, -1.0, 1.0), cd.Basis(nb))
    return cd.DDH(2 * math.pi * nx / 10, np.ones(fem.size()), fem, nx, ny, **kw)


def test_selection_of_the_chain_order(cuda):
    import cuddhelmholtz_amd as cd

    F = _ddh(cd, 256, 512)  # 8,192 subdomains: auto takes the element-lane form, and with it the paired chains
    assert F.info()["kernel"] == 5 and F.info()["n_domains"] == E.AUTO_MIN_DOMAINS
    assert F.sweep_form() == 2 and F.chain_order() == 2
    F.set_sweep_form(2)  # forced: pinned
    assert F.sweep_form() == 2 and F.chain_order() == 1
    F.set_chain_order(2)
    assert F.chain_order() == 2
    F.set_sweep_form(3)
    assert F.sweep_form() == 3 and F.chain_order() == 2
    F.set_chain_order(0)
    assert F.chain_order() == 1
    F.set_sweep_form(0)
    assert F.sweep_form() == 2 and F.chain_order() == 2  # auto for both again
    F.set_chain_order(1)
    assert F.sweep_form() == 2 and F.chain_order() == 1
    for bad in (-1, 3):
        with pytest.raises(RuntimeError):
            F.set_chain_order(bad)
    assert F.chain_order() == 1  # a refusal leaves the plan as it was
    F.set_sweep_form(1)
    assert F.sweep_form() == 1 and F.chain_order() == 0
    F.set_chain_order(2)  # accepted on the matrix form: takes effect when the form becomes 2 or 3
    assert F.chain_order() == 0
    F.set_sweep_form(2)
    assert F.chain_order() == 2

    F = _ddh(cd, 256, 256)  # 4,096 subdomains: the matrix form
    assert F.info()["kernel"] == 5 and F.sweep_form() == 1 and F.chain_order() == 0


def test_refusals_of_the_paired_chains(cuda):
    import cuddhelmholtz_amd as cd

    ratios = np.ones(16, dtype=np.int32)  # an explicit array is honoured, not collapsed to the one grid a = 1 would give
    ratios[::7] = 2
    plans = {
        "n_basis 8": lambda: _ddh(cd, 16, 16, nb=8),
        "fp64": lambda: _ddh(cd, 16, 16, precision="f64"),
        "kernel 3": lambda: _ddh(cd, 16, 16, kernel=3),
        "time_step": lambda: _ddh(cd, 16, 16, time_step=ratios),
        "kernel 13": lambda: _ddh(cd, 16, 16, kernel=13),
        "rk4": lambda: _ddh(cd, 16, 16, integrator="rk4"),
    }
    for what, make in plans.items():
        F = make()
        assert F.chain_order() == 0, what
        with pytest.raises(RuntimeError):
            F.set_chain_order(2)
            pytest.fail(f"order 2 was accepted by the {what} plan")
        assert F.chain_order() == 0, what
        F.set_chain_order(1)  # 0 and 1 are accepted by every plan, as forms 0 and 1 are
        F.set_chain_order(0)
        assert F.chain_order() == 0, what
    F = _ddh(cd, 16, 16)
    assert F.info()["kernel"] == 5
    for bad in (-1, 3):
        with pytest.raises(RuntimeError):
            F.set_chain_order(bad)
    F.set_chain_order(2)  # a kernel-5 plan with tables, one grid, RK2: accepted below the threshold too
    assert F.sweep_form() == 1 and F.chain_order() == 0
