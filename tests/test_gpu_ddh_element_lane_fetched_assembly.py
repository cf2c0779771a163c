"""How the carried march of kernel 5's element-lane form (head 2) forms the neighbour sums of its sweeps ("Assembly over the
LDS pipe"): assembly 1, one copy of a shared node forms the sum with DPP and the other takes it, and assembly 2, every copy fetches the
other copy's partial sum with ds_swizzle_b32 (the LDS pipe) and adds it itself (DDH.set_assembly / cuddh_hip_ddh_plan_set_assembly).  a + b and
b + a are one float, so EVERYTHING here is bit for bit: assembly 2 is compared with assembly 1 of the same plan, never with a
tolerance.  Plans are forced to (form, order, forcing, march) = (2, 2, 2, 2), where auto gives head 2; the helpers are those of
tests/test_gpu_ddh_element_lane_head.py and tests/test_gpu_ddh_element_lane_rectangles.py.

  * rhs / action / postprocess at 8 x 8 elements (four subdomains, one wavefront, a cross point), 16 x 16 (four wavefronts) and
    12 x 8 (six subdomains: the second wavefront's missing rows recompute its first subdomain and publish nothing);
  * the same on `square`, `rect` and `tall` of tests/ddh_metric_cases.py (8 x 12, six subdomains), and there also against the fp64
    oracle under that file's fp32 rule; on the smooth coefficient of the march tests against the fp64 oracle under the rule of the
    head tests (twice the distance head 1 reaches);
  * launch partitions on six subdomains: the ranges [0, 3) and [3, 6) and a caller's list against the whole launch; a list in
    permuted order gives every subdomain the bits it had, so what a lane without a neighbour fetches never reaches a result;
  * form 3 (the other owner) and a launch that holds issue priority;
  * auto at 256 x 512 elements is the forced variant, whichever assembly auto takes; selection and refusals on real plans.
"""
import numpy as np
import pytest

import ddh_metric_cases as mc
import test_gpu_ddh_element_lane as E
import test_gpu_ddh_element_lane_chains as CH
import test_gpu_ddh_element_lane_head as H
import test_gpu_ddh_element_lane_march as M
import test_gpu_ddh_element_lane_rectangles as RE
import test_gpu_ddh_mfma_layout as L
from ddh_metric_cases import FLOOR_FACTOR
from test_gpu_ddh_element_lane_forcing import _traces
from test_gpu_ddh_metrics import entry_points
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu

NAMES = ("rhs", "action", "postprocess")
AUTO = 2  # DDH_ASSEMBLY_AUTO of csrc/src/ddh_resolve.cpp: what auto takes from ELEMENT_LANE_MIN_DOMAINS subdomains on


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def with_assembly(F, assembly, form=2):
    F.set_assembly(assembly)
    assert F.assembly() == assembly and F.head() == 2 and RE.settings(F) == (form, 2, 2, 2)
    return F


def forced(cd, nx, ny=None):
    """(2, 2, 2, 2) forced on nx x ny elements, a = 1: head 2 by auto, and below the threshold the DPP assembly"""
    F, fem = E.make(cd, nx, 2, ny=ny)
    RE.force(F, (2, 2, 2, 2))
    assert F.head() == 2 and F.assembly() == 1
    return F, fem


def three_outputs(torch, cuda, F, ndof, f, lam):
    b = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
    F.rhs(f, b)
    y = torch.zeros_like(b)
    F.action(lam, y)
    u = torch.zeros(2 * ndof, dtype=torch.float64, device=cuda)
    F.postprocess(lam, f, u)
    return b.cpu().numpy(), y.cpu().numpy(), u.cpu().numpy()


@pytest.mark.parametrize("nx, ny", [(8, 8), (16, 16), (12, 8)])
def test_fetched_assembly_is_bitwise_the_dpp_assembly(cuda, nx, ny):
    import torch

    import cuddhelmholtz_amd as cd

    F, fem = forced(cd, nx, ny)
    assert F.info()["n_domains"] == (nx // 4) * (ny // 4)
    rng = np.random.default_rng(21)
    f = to_dev(torch, rng.standard_normal(2 * fem.size()), cuda)
    lam = to_dev(torch, rng.standard_normal(F.size()).astype(np.float32), cuda)
    dpp = three_outputs(torch, cuda, with_assembly(F, 1), fem.size(), f, lam)
    fetched = three_outputs(torch, cuda, with_assembly(F, 2), fem.size(), f, lam)
    for nm, a, b in zip(NAMES, dpp, fetched):
        assert np.isfinite(a).all() and np.abs(a).max() > 0, nm
        assert np.array_equal(bits(a), bits(b)), (nm, int((bits(a) != bits(b)).sum()), a.size)


@pytest.mark.parametrize("family", RE.PARITY_FAMILIES)
def test_fetched_assembly_on_the_metric_families(cuda, family):
    import torch

    import cuddhelmholtz_amd as cd

    c = mc.case(family, RE.NB, RE.BLOCK)
    missed = []
    for variant in ((2, 2, 2, 2), (3, 2, 2, 2)):
        F = RE.make(cd, c, variant)
        assert F.head() == 2 and F.info()["n_domains"] == 6
        dpp = entry_points(torch, cuda, with_assembly(F, 1, variant[0]), c)
        fetched = entry_points(torch, cuda, with_assembly(F, 2, variant[0]), c)
        for nm, a, b in zip(NAMES, dpp, fetched):
            assert np.array_equal(bits(a), bits(b)), (variant, nm)
        for nm, (e2, r2, emax, rmax), (fl2, fmax) in zip(NAMES, RE.distances(fetched, c.ref, c.floor), c.floor):
            print(f"[{c.name}] {variant} assembly 2 {nm}: vs fp64 oracle l2 {e2:.3e}, floor {fl2:.3e}, ratio {r2:.2f}; max {emax:.3e}, floor {fmax:.3e}, "
                  f"ratio {rmax:.2f} (gate {FLOOR_FACTOR:.0f})")
            if not (e2 <= FLOOR_FACTOR * fl2 and emax <= FLOOR_FACTOR * fmax):
                missed.append((variant, nm, e2, emax))
    assert not missed, missed


def test_fetched_assembly_with_a_coefficient_that_is_not_constant(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 8
    c = M.coefficient_case(nx)
    ref = L.oracle_outputs(c)
    F = H._make(cd, nx, 2, c[2])
    dpp = E.outputs(torch, cuda, with_assembly(F, 1), c)
    fetched = E.outputs(torch, cuda, with_assembly(F, 2), c)
    F.set_head(1)
    assert F.head() == 1 and F.assembly() == 0
    e1 = tuple(rel(a, r) for a, r in zip(E.outputs(torch, cuda, F, c), ref))
    e2 = tuple(rel(a, r) for a, r in zip(fetched, ref))
    for i, nm in enumerate(NAMES):
        print(f"[8x8, smooth a in [0.5, 1]] {nm}: head 2 with assembly 2 vs fp64 oracle {e2[i]:.4e}, head 1 vs oracle {e1[i]:.4e} (gate: 2 x head 1)")
    for i, nm in enumerate(NAMES):
        assert np.array_equal(bits(dpp[i]), bits(fetched[i])), nm
        assert e1[i] < 1e-4, (nm, e1[i])
        assert e2[i] < 2 * e1[i], (nm, e2[i], e1[i])


def test_launch_partitions_lists_owner_rule_and_priority_are_bitwise(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    F, fem = forced(cd, 12, 8)
    nd = F.info()["n_domains"]
    assert nd == 6
    rng = np.random.default_rng(22)
    f = to_dev(torch, rng.standard_normal(2 * fem.size()), cuda)
    lam = to_dev(torch, rng.standard_normal(F.size()).astype(np.float32), cuda)
    dpp = _traces(torch, cuda, with_assembly(F, 1), f, lam)  # sources only, traces only (the form without x), both: each not zero
    with_assembly(F, 2)
    plain = _traces(torch, cuda, F, f, lam)
    for a, b in zip(dpp, plain):
        assert torch.equal(a, b)
    perm = np.array([4, 1, 5, 0, 3, 2], dtype=np.int32)
    for full, (x, l) in zip(plain, ((f, None), (None, lam), (f, lam))):
        ranged = torch.zeros_like(full)
        F.local_traces(0, 3, x, l, ranged)  # one wavefront with a missing row
        F.local_traces(3, nd, x, l, ranged)
        assert torch.equal(ranged, full)
        listed = torch.zeros_like(full)
        for ids in (perm[:5], perm[5:]):  # a caller's list, cut so that both wavefronts of the first launch have other row mates
            F.local_traces_listed(to_dev(torch, ids, cuda), x, l, listed)
        assert torch.equal(listed, full)
        # the whole launch in permuted order: every subdomain shares its wavefront with other subdomains, in other rows, and gets
        # the bits it had
        permuted = torch.zeros_like(full)
        F.local_traces_listed(to_dev(torch, perm, cuda), x, l, permuted)
        assert torch.equal(permuted, full)
    F.set_wave_priority(True)
    held = _traces(torch, cuda, F, f, lam)
    F.set_wave_priority(False)
    for a, b in zip(plain, held):
        assert torch.equal(a, b)
    # form 3: the other copy of every shared node publishes, same bits, with either assembly
    F.set_sweep_form(3)
    assert RE.settings(F) == (3, 2, 2, 2) and F.head() == 2 and F.assembly() == 2
    other = _traces(torch, cuda, F, f, lam)
    F.set_wave_priority(True)
    other_held = _traces(torch, cuda, F, f, lam)
    F.set_wave_priority(False)
    F.set_sweep_form(2)
    for a, b, c3 in zip(plain, other, other_held):
        assert torch.equal(a, b) and torch.equal(a, c3)


def test_auto_on_many_subdomains_is_the_forced_variant_and_selection(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    F = CH._ddh(cd, 256, 512)  # 8,192 subdomains, 2,048 wavefronts, all auto
    assert F.info()["kernel"] == 5 and F.info()["n_domains"] == E.AUTO_MIN_DOMAINS
    assert RE.settings(F) == (2, 2, 2, 2) and F.head() == 2 and F.assembly() == AUTO
    lam = to_dev(torch, np.random.default_rng(11).standard_normal(F.size()).astype(np.float32), cuda)
    auto = torch.zeros_like(lam)
    F.action(lam, auto)
    assert torch.isfinite(auto).all().item() and auto.abs().max().item() > 0 and (auto != lam).any().item()
    for assembly in (2, 1):
        F.set_assembly(assembly)
        assert F.assembly() == assembly and RE.settings(F) == (2, 2, 2, 2) and F.head() == 2
        out = torch.zeros_like(lam)
        F.action(lam, out)
        assert torch.equal(out, auto), assembly
    # selection: 2 goes idle with the head and comes back with it; where head 2 is not in effect it is refused
    F.set_assembly(2)
    F.set_head(1)
    assert F.head() == 1 and F.assembly() == 0
    with pytest.raises(RuntimeError):
        F.set_assembly(2)
    assert F.head() == 1 and F.assembly() == 0
    F.set_head(0)
    assert F.head() == 2 and F.assembly() == 2  # stored before: back with the head
    for bad in (-1, 3):
        with pytest.raises(RuntimeError):
            F.set_assembly(bad)
    assert F.assembly() == 2  # a refusal leaves the plan as it was
    F.set_assembly(0)
    assert F.assembly() == AUTO
    F.set_sweep_form(1)
    assert F.head() == 0 and F.assembly() == 0
    with pytest.raises(RuntimeError):
        F.set_assembly(2)  # the matrix form

    G = CH._ddh(cd, 16, 16)  # 16 subdomains: the matrix form under auto
    assert G.sweep_form() == 1 and G.assembly() == 0
    with pytest.raises(RuntimeError):
        G.set_assembly(2)
    G.set_assembly(1)  # 0 and 1 are accepted by every plan
    G.set_assembly(0)
    for what, make in {"fp64": lambda: CH._ddh(cd, 16, 16, precision="f64"), "kernel 13": lambda: CH._ddh(cd, 16, 16, kernel=13)}.items():
        P = make()
        assert P.assembly() == 0, what
        with pytest.raises(RuntimeError):
            P.set_assembly(2)
        assert P.assembly() == 0, what
