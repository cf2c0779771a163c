"""DDH kernel 5's element-lane form in the orders, forcings and marches that auto takes, on elements with hx != hy.

The parity tests of the paired chains (order 2), of the sources in the first pass only (forcing 2) and of the scaled velocity
(march 2) run on square elements.  There the in-lane sweep z' = Dg w + sum Bx(k, j) w(j, l) + sum By(l, j) w(k, j) has Bx == By
bit for bit and a symmetric node weight W(k, l) = gamma_k beta_l, so Bx and By exchanged (in element_lane_pair_product, in the
source-free loop of wh_march_pairs_once, in the 2 (1 - hm Hi) q^ / m heads of wh_march_pairs_scaled), a transposed W in the
per-dof constants, or xi and eta mixed up in the 1 / m heads are exact identities and pass.  tests/test_gpu_ddh_metrics.py runs
kernel 5 on rectangles as a forced form, which resolves to (order 1, forcing 1, march 0): the oldest variant only.  Here a
variant is (form, order, forcing, march), set on a (5, form) plan with set_chain_order, set_forcing and set_march, the four
getters asserted after every setter, on the cases of tests/ddh_metric_cases.py: `square`, `rect` (hy = hx / 2, g00 < g11) and
`tall` (hy = 2 hx, g00 > g11), n_basis 4, 8 x 12 elements in 6 subdomains (one full row group of a wavefront and a tail of 2),
coefficient alpha_disk.

  (a) parity: (2,2,1,0), (2,2,2,1), (2,2,2,2) and (3,2,2,2) on the three families: rhs, action on the written slots and
      postprocess into pre-filled buffers against the fp64 oracle, relative l2 and max norm <= FLOOR_FACTOR (4) x the fp32
      oracle's own distance to the fp64 oracle on that case: the fp32 rule of tests/test_gpu_ddh_metrics.py, nothing new;
  (b) (2,2,2,1) and (2,2,2,2) on swapped_rect (the rect inputs by index on the tall mesh): within the gate of that mesh's own
      reference and at least 100 gates from rect's.  The fp64 references lie 3.5e5 gates apart
      (tests/test_ddh_metric_cases.py), so the gate of (a) does separate the two anisotropies for what the device computes;
  (c) bitwise on rect and tall, for (2,2,1,0), (2,2,2,1) and (2,2,2,2), sources only, traces only and both: a repeated run,
      [0, 3) + [3, 6), a permuted list cut after five, a launch that holds issue priority, form 3 against form 2 (the owner
      rule: on rectangles the copies of a shared node meet different Bx and By rows and, under march 2, the 1 / m heads, and
      must still hold one sum), and action(2 lambda) == 2 action(lambda);
  (d) 256 x 512 elements on [-1, 1]^2 (8,192 subdomains, hx = 2 hy), everything auto, resolves to (2,2,2,2); one action of it
      is bit for bit that of the same plan with all four settings forced to (2,2,2,2), and not zero: what auto launches on many
      wavefronts of rectangular elements is the forced variant that (a) compares.  No oracle at this size.

Every distance, floor and ratio is printed (`pytest -s`).  Measured on one MI355X:
(a) per output `distance (ratio)` in relative l2, then in max norm; floor = fp32 oracle vs fp64 oracle; gate: ratio <= 4.
  8x12 n_basis 4 block 4 square: floors l2 4.41e-07 / 2.85e-07 / 4.56e-07; max 5.67e-07 / 4.28e-07 / 9.16e-07
    variant    rhs                               action                            postprocess
    (2,2,1,0)  4.71e-07 (1.07) 5.58e-07 (0.98) 2.88e-07 (1.01) 3.99e-07 (0.93) 5.06e-07 (1.11) 1.05e-06 (1.15)
    (2,2,2,1)  5.10e-07 (1.16) 6.19e-07 (1.09) 2.68e-07 (0.94) 2.65e-07 (0.62) 4.99e-07 (1.10) 8.88e-07 (0.97)
    (2,2,2,2)  4.75e-07 (1.08) 5.21e-07 (0.92) 2.82e-07 (0.99) 3.36e-07 (0.79) 5.20e-07 (1.14) 1.10e-06 (1.20)
    (3,2,2,2)  4.75e-07 (1.08) 5.21e-07 (0.92) 2.82e-07 (0.99) 3.36e-07 (0.79) 5.20e-07 (1.14) 1.10e-06 (1.20)
  8x12 n_basis 4 block 4 rect: floors l2 5.24e-07 / 3.81e-07 / 5.46e-07; max 9.90e-07 / 6.15e-07 / 1.08e-06
    variant    rhs                               action                            postprocess
    (2,2,1,0)  5.88e-07 (1.12) 1.05e-06 (1.07) 4.05e-07 (1.06) 5.12e-07 (0.83) 5.90e-07 (1.08) 1.24e-06 (1.15)
    (2,2,2,1)  5.06e-07 (0.96) 8.60e-07 (0.87) 4.08e-07 (1.07) 8.31e-07 (1.35) 5.91e-07 (1.08) 1.02e-06 (0.95)
    (2,2,2,2)  5.61e-07 (1.07) 7.30e-07 (0.74) 3.90e-07 (1.02) 7.14e-07 (1.16) 5.90e-07 (1.08) 1.07e-06 (0.99)
    (3,2,2,2)  5.61e-07 (1.07) 7.30e-07 (0.74) 3.90e-07 (1.02) 7.14e-07 (1.16) 5.90e-07 (1.08) 1.07e-06 (0.99)
  8x12 n_basis 4 block 4 tall: floors l2 4.81e-07 / 3.30e-07 / 5.15e-07; max 7.14e-07 / 4.46e-07 / 7.53e-07
    variant    rhs                               action                            postprocess
    (2,2,1,0)  7.54e-07 (1.57) 8.45e-07 (1.18) 3.51e-07 (1.06) 4.49e-07 (1.01) 6.49e-07 (1.26) 9.12e-07 (1.21)
    (2,2,2,1)  8.16e-07 (1.70) 6.50e-07 (0.91) 3.62e-07 (1.10) 4.08e-07 (0.91) 6.49e-07 (1.26) 6.53e-07 (0.87)
    (2,2,2,2)  7.55e-07 (1.57) 7.75e-07 (1.09) 3.59e-07 (1.09) 7.21e-07 (1.61) 6.04e-07 (1.17) 5.52e-07 (0.73)
    (3,2,2,2)  7.55e-07 (1.57) 7.75e-07 (1.09) 3.59e-07 (1.09) 7.21e-07 (1.61) 6.04e-07 (1.17) 5.52e-07 (0.73)
(b) swapped_rect: floors l2 5.45e-07 / 2.97e-07 / 4.91e-07; max 7.22e-07 / 3.88e-07 / 7.18e-07; to its own reference as in (a), then the
    relative l2 distance to the rect case's reference in fp32 gates of the rect case (rhs / action / postprocess; 100 is asserted)
    (2,2,2,1)  6.01e-07 (1.10) 6.62e-07 (0.92) 3.84e-07 (1.29) 7.13e-07 (1.84) 6.19e-07 (1.26) 8.15e-07 (1.13)   466148 / 347441 / 559805
    (2,2,2,2)  7.45e-07 (1.37) 8.23e-07 (1.14) 3.54e-07 (1.19) 6.24e-07 (1.61) 5.91e-07 (1.20) 7.64e-07 (1.06)   466148 / 347441 / 559805

No cell misses a gate and no fault was found; no kernel source changed.  The largest ratio of (a) is 1.70 ((2,2,2,1), rhs, l2, tall),
then 1.61 ((2,2,2,2) and (3,2,2,2), action, max norm, tall); on rect 1.35, on square 1.20; the largest of (b) is 1.84 ((2,2,2,1),
action, max norm).  Form 3 gives the bits of form 2 in every row, as (c) asserts trace by trace.  The distances of (b) to the other
mesh's reference are those of the two fp64 references to the digit: the device error is six orders below them.
"""
import numpy as np
import pytest

import ddh_metric_cases as mc
import test_gpu_ddh_element_lane as E
import test_gpu_ddh_element_lane_chains as CH
from ddh_metric_cases import FLOOR_FACTOR, NAMES
from test_gpu_ddh_element_lane_forcing import _traces
from test_gpu_ddh_metrics import entry_points, plan
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

NB, BLOCK = 4, 4
PARITY_FAMILIES = ("square", "rect", "tall")
# (sweep form, chain order, forcing, march): every pass forced, the first pass only with q, with q / (2 hm), and its other owner
PARITY_VARIANTS = ((2, 2, 1, 0), (2, 2, 2, 1), (2, 2, 2, 2), (3, 2, 2, 2))
BITWISE_VARIANTS = ((2, 2, 1, 0), (2, 2, 2, 1), (2, 2, 2, 2))
SWAPPED_VARIANTS = ((2, 2, 2, 1), (2, 2, 2, 2))


def settings(F):
    return F.sweep_form(), F.chain_order(), F.forcing(), F.march()


def force(F, variant):
    """the three setters on a plan whose form is forced (the pinned chains), with what the getters report after each"""
    form, order, forcing, march = variant
    assert F.info()["kernel"] == 5 and settings(F) == (form, 1, 0, 0)
    F.set_chain_order(order)
    assert settings(F) == (form, order, 1, 0)  # the paired chains: the sources in every pass until asked otherwise
    F.set_forcing(forcing)
    assert settings(F) == (form, order, forcing, 1 if forcing == 2 else 0)  # the first pass only: q itself until asked otherwise
    F.set_march(march)
    assert settings(F) == variant
    return F


def make(cd, c, variant):
    return force(plan(cd, c, "f32", (5, variant[0])), variant)


def distances(got, ref, floor):
    """per output: (relative l2, its ratio to the floor, max norm, its ratio to the floor)"""
    return [(mc.rel(g, r), mc.rel(g, r) / fl2, mc.rel_max(g, r), mc.rel_max(g, r) / fmax) for g, r, (fl2, fmax) in zip(got, ref, floor)]


# ------------------------------------------------------------------ (a) parity
@pytest.mark.parametrize("family", PARITY_FAMILIES)
def test_paired_first_pass_and_scaled_marches_vs_oracle(cuda, family):
    import torch

    import cuddhelmholtz_amd as cd

    c = mc.case(family, NB, BLOCK)
    print(f"[{c.name}] floors l2 " + " / ".join(f"{fl2:.2e}" for fl2, _ in c.floor) + "; max " + " / ".join(f"{fmax:.2e}" for _, fmax in c.floor))
    missed, ran = [], 0
    for variant in PARITY_VARIANTS:
        F = make(cd, c, variant)
        info = F.info()
        assert (info["nt"], info["n_domains"], info["nel1d"]) == (c.O64.t.nt, 6, BLOCK) and F.size() == c.O64.size, variant
        row = distances(entry_points(torch, cuda, F, c), c.ref, c.floor)
        assert settings(F) == variant
        ran += 1
        for nm, (e2, r2, emax, rmax), (fl2, fmax) in zip(NAMES, row, c.floor):
            print(f"[{c.name}] {variant} {nm}: vs fp64 oracle l2 {e2:.3e}, floor {fl2:.3e}, ratio {r2:.2f}; max {emax:.3e}, floor {fmax:.3e}, "
                  f"ratio {rmax:.2f} (gate {FLOOR_FACTOR:.0f})")
            if not (e2 <= FLOOR_FACTOR * fl2 and emax <= FLOOR_FACTOR * fmax):
                missed.append((variant, nm, e2, emax))
        print(f"row [{family}] {variant} " + " ".join(f"{e2:.2e} ({r2:.2f}) {emax:.2e} ({rmax:.2f})" for e2, r2, emax, rmax in row))
    assert ran == len(PARITY_VARIANTS)
    assert not missed, missed


# ------------------------------------------------------------------ (b) the two anisotropies
@pytest.mark.parametrize("variant", SWAPPED_VARIANTS, ids=["-".join(map(str, v)) for v in SWAPPED_VARIANTS])
def test_the_two_anisotropies_are_told_apart_on_the_device(cuda, variant):
    """the rect case's coefficient, sources and traces by index on the mesh with hy = 2 hx, not hx / 2: the kernel follows that
    mesh's own reference within the gate and lies more than 100 fp32 gates from the rect case's reference.  Bx for By, gamma for
    beta or xi for eta somewhere in the march would compute (part of) the other mesh's operator."""
    import torch

    import cuddhelmholtz_amd as cd

    r, s = mc.case("rect", NB, BLOCK), mc.swapped_rect(NB, BLOCK)
    F = make(cd, s, variant)
    assert F.info()["nt"] == s.O64.t.nt
    got = entry_points(torch, cuda, F, s)
    missed = []
    for nm, g, (e2, r2, emax, rmax), other, (fl2, fmax), (rfl2, _) in zip(NAMES, got, distances(got, s.ref, s.floor), r.ref, s.floor, r.floor):
        e_other = mc.rel(g, other)
        print(f"[{s.name}, the rect inputs, {variant}] {nm}: vs its own reference l2 {e2:.3e} (floor {fl2:.3e}, ratio {r2:.2f}), max {emax:.3e} "
              f"(floor {fmax:.3e}, ratio {rmax:.2f}); vs the rect case's {e_other:.3e} = {e_other / (FLOOR_FACTOR * rfl2):.0f} fp32 gates")
        if not (e2 <= FLOOR_FACTOR * fl2 and emax <= FLOOR_FACTOR * fmax and e_other >= 100 * FLOOR_FACTOR * rfl2):
            missed.append((nm, e2, emax, e_other))
    assert not missed, missed


# ------------------------------------------------------------------ (c) bitwise properties
@pytest.mark.parametrize("variant", BITWISE_VARIANTS, ids=["-".join(map(str, v)) for v in BITWISE_VARIANTS])
@pytest.mark.parametrize("family", ["rect", "tall"])
def test_launch_partitions_owner_rule_and_scaling_are_bitwise_on_rectangles(cuda, family, variant):
    import torch

    import cuddhelmholtz_amd as cd

    c = mc.case(family, NB, BLOCK)
    F = make(cd, c, variant)
    nd = F.info()["n_domains"]
    assert nd == 6
    f = to_dev(torch, np.array(c.fh), cuda)
    lam = to_dev(torch, c.lam.astype(np.float32), cuda)
    perm = np.random.default_rng(3).permutation(nd).astype(np.int32)
    plain = _traces(torch, cuda, F, f, lam)  # sources only, traces only (the form without x), both: each not zero
    for a, b in zip(plain, _traces(torch, cuda, F, f, lam)):
        assert torch.equal(a, b)
    for full, (x, l) in zip(plain, ((f, None), (None, lam), (f, lam))):
        ranged = torch.zeros_like(full)
        F.local_traces(0, 3, x, l, ranged)
        F.local_traces(3, nd, x, l, ranged)
        assert torch.equal(ranged, full)
        listed = torch.zeros_like(full)
        for ids in (perm[:5], perm[5:]):
            F.local_traces_listed(to_dev(torch, ids, cuda), x, l, listed)
        assert torch.equal(listed, full)
    F.set_wave_priority(True)
    held = _traces(torch, cuda, F, f, lam)
    F.set_wave_priority(False)
    for a, b in zip(plain, held):
        assert torch.equal(a, b)
    # the owner rule: the other copy of every shared node publishes, same bits
    F.set_sweep_form(3)
    assert settings(F) == (3,) + variant[1:]
    other = _traces(torch, cuda, F, f, lam)
    F.set_sweep_form(2)
    assert settings(F) == variant
    for a, b in zip(plain, other):
        assert torch.equal(a, b)

    y1, y2 = torch.zeros_like(lam), torch.zeros_like(lam)
    F.action(lam, y1)
    F.action(2.0 * lam, y2)  # I - T is linear; scaling by 2 is exact in fp32
    assert y1.abs().max().item() > 0 and torch.equal(y2, 2.0 * y1)


# ------------------------------------------------------------------ (d) what auto launches
def test_auto_launches_the_forced_variant_on_many_rectangular_subdomains(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    F = CH._ddh(cd, 256, 512)  # [-1, 1]^2: hx = 2 hy; 8,192 subdomains, 2,048 wavefronts
    assert F.info()["kernel"] == 5 and F.info()["n_domains"] == E.AUTO_MIN_DOMAINS
    assert settings(F) == (2, 2, 2, 2)
    lam = to_dev(torch, np.random.default_rng(11).standard_normal(F.size()).astype(np.float32), cuda)
    auto = torch.zeros_like(lam)
    F.action(lam, auto)
    assert settings(F) == (2, 2, 2, 2)
    F.set_sweep_form(2)
    force(F, (2, 2, 2, 2))
    forced = torch.zeros_like(lam)
    F.action(lam, forced)
    assert torch.isfinite(auto).all().item() and auto.abs().max().item() > 0 and (auto != lam).any().item()
    assert torch.equal(forced, auto)
