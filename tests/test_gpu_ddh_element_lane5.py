"""DDH kernel 12 (ddh_element_lane_kernel<5, ..>): n_basis 5, block 4, fp32; lane = one element with its 25 nodes in
registers, one subdomain per 16-lane row, four subdomains per wavefront, assembly by DPP row shifts.

Shapes: 8 x 8 elements (2 x 2 subdomains: a cross point, exactly one wavefront, nt 1250) and 12 x 8 (3 x 2: rectangular
elements, so gx != gz, a subdomain with three neighbours, one full wavefront and a tail of two, nt 1251) on [-1,1]^2, a = 1,
omega = 2 pi nx / 10, inputs and oracle of tests/test_gpu_ddh_block_size.Case, computed once per shape and shared.

  * parity: rhs, action (on the written slots) and postprocess of kernel 12 and of kernel 1 (f32) against OracleDDH(float64);
    the gate per entry point is 4 x the distance of OracleDDH(float32) to it on the same inputs, computed here (the rule of
    tests/test_gpu_ddh_block_size.py), and kernel 12 against kernel 1 is within the sum of the two gates;
  * launch partitions, 20 x 20 elements (25 subdomains: full wavefronts and a tail of one): local_traces over [0, n), over
    ranges of lengths 13, 1, 7 and 4, local_traces_listed in a shuffled order cut at an odd place, the same while holding
    issue priority, and a repeat are bitwise equal, with x only, with lambda only and with both; the y contributions of
    subdomains that share no dof are bitwise equal from one listed launch and from one launch each;
  * copies: with the owner rule turned round (DDH.set_owner_rule: the last copy of a node shared by 2 or 4 elements
    publishes, not the first) traces and y contributions are bitwise the same;
  * refusals and auto: kernel 12 is refused at n_basis 4, at n_basis 5 with block 2, in f64, with two distinct time-step
    ratios and with integrator "rk4"; auto below AUTO_MIN_DOMAINS subdomains is kernel 1, from there on 12, and an auto plan
    that would be 12 runs on kernel 1 with RK4 and with per-subdomain time steps.
Every distance is printed (`pytest -s`).
"""
import math

import numpy as np
import pytest

import test_gpu_ddh_block_size as B
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu

AUTO_MIN_DOMAINS = 64  # ELEMENT_LANE5_MIN_DOMAINS of csrc/src/ddh_resolve.cpp
SHAPES = {(8, 8): (272, 1250), (12, 8): (476, 1251)}  # (nx, ny) -> (traces, time steps per period)


@pytest.mark.parametrize("nx,ny", list(SHAPES))
def test_fp32_kernel_12_and_kernel_1_vs_oracle(cuda, nx, ny):
    import torch

    import cuddhelmholtz_amd as cd

    c = B.case(nx, ny, 5, 4, True)
    F12, _ = B.make(cd, c, "f32", 12)
    F1, _ = B.make(cd, c, "f32", 1)
    i12 = F12.info()
    assert i12["kernel"] == 12 and F1.info()["kernel"] == 1
    assert (F12.size(), i12["nt"], i12["nel1d"], i12["mx_dof"], i12["mx_fdof"]) == (*SHAPES[nx, ny], 4, 289, 64)
    assert c.O64.size == F12.size() and c.O64.t.nt == i12["nt"]
    out12, out1 = B.entry_points(torch, cuda, F12, c), B.entry_points(torch, cuda, F1, c)
    e12 = tuple(rel(a, r) for a, r in zip(out12, c.ref))
    e1 = tuple(rel(a, r) for a, r in zip(out1, c.ref))
    e121 = tuple(float(np.linalg.norm(a - b) / np.linalg.norm(r)) for a, b, r in zip(out12, out1, c.ref))
    for i, nm in enumerate(B.NAMES):
        print(f"[{nx}x{ny}, n_basis 5, block 4, f32] {nm}: floor (fp32 oracle vs fp64 oracle) {c.floor[i]:.3e}, gate 4 x; kernel 12 vs fp64 "
              f"oracle {e12[i]:.3e} ({e12[i] / c.floor[i]:.2f} x floor), kernel 1 {e1[i]:.3e} ({e1[i] / c.floor[i]:.2f} x floor), "
              f"kernel 12 vs kernel 1 {e121[i]:.3e}")
    for i, nm in enumerate(B.NAMES):
        gate = 4 * c.floor[i]
        assert e12[i] <= gate, (nm, "kernel 12", e12[i], gate)
        assert e1[i] <= gate, (nm, "kernel 1", e1[i], gate)
        assert e121[i] <= 2 * gate, (nm, "kernel 12 vs kernel 1", e121[i], 2 * gate)


NX = 20  # 5 x 5 subdomains


def plan_20(cd, torch, cuda):
    """kernel 12 on 20 x 20 elements with fixed random sources and traces: (F, fem, f, lam, n_domains)"""
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(NX, -1.0, 1.0, NX, -1.0, 1.0), cd.Basis(5))
    F = cd.DDH(2 * math.pi * NX / 10, np.ones(fem.size()), fem, NX, NX, precision="f32", kernel=12, block=4)
    info = F.info()
    assert info["kernel"] == 12 and info["n_domains"] == 25
    rng = np.random.default_rng(11)
    f = to_dev(torch, rng.standard_normal(2 * fem.size()), cuda)
    lam = to_dev(torch, rng.standard_normal(F.size()).astype(np.float32), cuda)
    return F, fem, f, lam, 25


def apart_subdomains(F, nd):
    """every other subdomain in both directions: no two share a dof, so every entry of u gets one add and the atomics' order cannot matter"""
    ndx = NX // 4
    apart = np.array([s for s in range(nd) if (s % ndx) % 2 == 0 and (s // ndx) % 2 == 0], dtype=np.int32)
    gI = F.table("gI").reshape(nd, F.info()["mx_dof"])
    touched = np.concatenate([gI[s] for s in apart])
    assert touched.min() >= 0 and np.unique(touched).size == touched.size
    return apart


def test_kernel_12_launch_partitions_are_bitwise_the_full_launch(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    F, fem, f, lam, nd = plan_20(cd, torch, cuda)
    perm = np.random.default_rng(3).permutation(nd).astype(np.int32)
    cut = 9
    assert cut % 4 and (nd - cut) % 4 == 0
    for x, l in ((f, None), (None, lam), (f, lam)):  # sources only, traces only (the form without x), both
        plain = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
        F.local_traces(0, nd, x, l, plain)
        assert plain.abs().max().item() > 0 and torch.isfinite(plain).all()
        again = torch.zeros_like(plain)
        F.local_traces(0, nd, x, l, again)
        assert torch.equal(again, plain)
        ranged = torch.zeros_like(plain)
        for d0, d1 in ((0, 13), (13, 14), (14, 21), (21, nd)):  # lengths 13, 1, 7, 4
            F.local_traces(d0, d1, x, l, ranged)
        assert torch.equal(ranged, plain)
        for high in (False, True):
            F.set_wave_priority(high)
            listed = torch.zeros_like(plain)
            for ids in (perm[:cut], perm[cut:]):
                F.local_traces_listed(to_dev(torch, ids, cuda), x, l, listed)
            F.set_wave_priority(False)
            assert torch.equal(listed, plain), high

    apart = np.random.default_rng(5).permutation(apart_subdomains(F, nd)).astype(np.int32)
    assert apart.size == 9
    n = fem.size()
    for x in (f, None):
        together = torch.zeros(2 * n, dtype=torch.float64, device=cuda)
        F.local_solution_listed(to_dev(torch, apart, cuda), lam, x, together, True)
        assert together.abs().max().item() > 0
        single = torch.zeros_like(together)
        for s in apart:
            F.local_solution(int(s), int(s) + 1, lam, x, single, False)
        assert torch.equal(single, together)


def test_kernel_12_published_result_does_not_depend_on_the_owning_copy(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    F, fem, f, lam, nd = plan_20(cd, torch, cuda)
    apart = apart_subdomains(F, nd)

    def published(last):
        F.set_owner_rule(last)
        out = []
        for x, l in ((f, None), (None, lam), (f, lam)):
            t = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
            F.local_traces(0, nd, x, l, t)
            assert t.abs().max().item() > 0
            out.append(t)
        for x in (f, None):
            u = torch.zeros(2 * fem.size(), dtype=torch.float64, device=cuda)
            F.local_solution_listed(to_dev(torch, apart, cuda), lam, x, u, True)
            assert u.abs().max().item() > 0
            out.append(u)
        return out

    first, last = published(False), published(True)
    F.set_owner_rule(False)
    for a, b in zip(first, last):
        assert torch.equal(a, b)


def test_refusals_and_auto_selection(cuda):
    import cuddhelmholtz_amd as cd

    def ddh(nb, nx, block, precision, kernel, **kw):
        fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(nb))
        return cd.DDH(2 * math.pi * nx / 10, np.ones(fem.size()), fem, nx, nx, precision=precision, kernel=kernel, block=block, **kw)

    assert ddh(5, 8, 4, "f32", 12).info()["kernel"] == 12
    # the plan is made on first use, and refuses there
    for args, kw in (((4, 8, 4, "f32", 12), {}), ((5, 8, 2, "f32", 12), {}), ((5, 8, 4, "f64", 12), {}),
                     ((5, 8, 4, "f32", 12), {"time_step": np.array([1, 2, 1, 1])}), ((5, 8, 4, "f32", 12), {"integrator": "rk4"})):
        with pytest.raises(RuntimeError):
            ddh(*args, **kw).info()
    # auto: kernel 1 below the threshold, and at every size where kernel 12 has no form
    assert ddh(5, 8, 4, "f32", 0).info()["kernel"] == 1
    assert ddh(5, 8, 4, "f64", 0).info()["kernel"] == 1
    nx = 4 * math.isqrt(AUTO_MIN_DOMAINS - 1)
    assert (nx // 4) ** 2 < AUTO_MIN_DOMAINS <= (nx // 4 + 1) ** 2
    assert ddh(5, nx, 4, "f32", 0).info()["kernel"] == 1
    nx += 4
    assert ddh(5, nx, 4, "f32", 0).info()["kernel"] == 12
    F = ddh(5, nx, 4, "f32", 0, integrator="rk4")
    assert F.info()["kernel"] == 1 and F.integrator() == ("rk4", 4)
    ratios = np.ones((nx // 4) ** 2, dtype=np.int32)
    ratios[0] = 2
    assert ddh(5, nx, 4, "f32", 0, time_step=ratios).info()["kernel"] == 1
    # the owner-rule switch exists on kernel 12 as on kernel 11, and on no other
    ddh(5, 8, 4, "f32", 12).set_owner_rule(True)
    with pytest.raises(RuntimeError):
        ddh(5, 8, 4, "f32", 1).set_owner_rule(True)
