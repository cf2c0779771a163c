"""Which kernel, sweep form and chain order a DDH plan runs after a sequence of setters, through real plans ("Which
kernel a DDH plan runs: resolved once").  The literals are those of the comments in include/cuddh_hip.h; tests/test_ddh_resolve.py
asserts the same rule without a GPU.

Shapes, four subdomains each, a = 1, omega = 2 pi nx / 10 on [-1,1]^2: 8 x 8 elements at n_basis 4 and at n_basis 5 (blocks of
4 x 4), 4 x 4 elements at n_basis 8 (blocks of 2 x 2), 16 x 16 elements at n_basis 4 with block 8, and two label-built plans
(8 x 8 elements at n_basis 4 in 4 x 4 blocks; 6 x 6 at n_basis 5 in 3 x 3 blocks).  A plan is created with its time grids and
its integrator (the integrator is set first), so a walk is: the creation arguments, the state expected after creation -- or
None where creation is refused -- and then setter calls, each with the state expected after it; a refused call must raise and
leave (kernel, sweep form, chain order) as they were.  Every plan that is valid at the end of its walk runs its local solves
once (one WaveHoltz iteration): the traces are finite, not all zero, and bitwise the same from one launch over all subdomains
and from two launches over a half each -- what a plan runs is a property of the plan, never of a launch."""
import math

import numpy as np
import pytest

from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

GRIDS = np.array([1, 2, 1, 1], dtype=np.int32)
REFUSED = "refused"
# shape -> (n_basis, elements per side, block or None for the reference's, label block or None)
SHAPES = {"nb4": (4, 8, None, None), "nb5": (5, 8, 4, None), "nb8": (8, 4, None, None), "nb4 block 8": (4, 16, 8, None),
          "labels nb4": (4, 8, None, 4), "labels nb5": (5, 6, None, 3)}

# (shape, precision, kernel, creation keywords, state after creation or None, [(setter, argument, state after or REFUSED)])
WALKS = [
    # ---- n_basis 4, 4 x 4 blocks
    ("nb4", "f32", 0, {}, (5, 1, 0),
     [("set_sweep_form", 2, (5, 2, 1)), ("set_chain_order", 2, (5, 2, 2)), ("set_chain_order", 0, (5, 2, 1)), ("set_sweep_form", 3, (5, 3, 1)),
      ("set_chain_order", 2, (5, 3, 2)), ("set_chain_order", 1, (5, 3, 1)), ("set_sweep_form", 4, REFUSED), ("set_chain_order", 3, REFUSED),
      ("set_owner_rule", True, REFUSED), ("set_sweep_form", 0, (5, 1, 0))]),
    ("nb4", "f32", 0, {}, (5, 1, 0),  # the other order: the chain order first, on a form-1 plan, in effect once the form is 2
     [("set_chain_order", 2, (5, 1, 0)), ("set_sweep_form", 2, (5, 2, 2)), ("set_sweep_form", 1, (5, 1, 0)), ("set_sweep_form", 3, (5, 3, 2))]),
    ("nb4", "f64", 0, {}, (3, 0, 0),
     [("set_sweep_form", 2, REFUSED), ("set_sweep_form", 1, (3, 0, 0)), ("set_chain_order", 2, REFUSED), ("set_chain_order", 1, (3, 0, 0)),
      ("set_owner_rule", False, REFUSED)]),
    ("nb4", "f32", 1, {}, (1, 0, 0), [("set_sweep_form", 2, REFUSED), ("set_owner_rule", True, REFUSED)]),
    ("nb4", "f32", 2, {}, (2, 0, 0), []),
    ("nb4", "f32", 3, {}, (3, 0, 0), [("set_sweep_form", 3, REFUSED), ("set_chain_order", 2, REFUSED)]),
    ("nb4", "f32", 4, {}, (4, 0, 0), []),
    ("nb4", "f32", 5, {}, (5, 1, 0), [("set_sweep_form", 2, (5, 2, 1))]),
    ("nb4", "f64", 8, {}, (8, 0, 0), [("set_sweep_form", 2, REFUSED)]),
    ("nb4", "f32", 13, {}, (13, 0, 0), [("set_sweep_form", 2, REFUSED), ("set_chain_order", 2, REFUSED), ("set_owner_rule", True, (13, 0, 0))]),
    ("nb4", "f32", 8, {}, None, []),
    ("nb4", "f64", 5, {}, None, []),
    ("nb4", "f64", 13, {}, None, []),
    ("nb4", "f32", 6, {}, None, []),
    ("nb4", "f32", 11, {}, None, []),
    ("nb4", "f32", 12, {}, None, []),
    # time grids
    ("nb4", "f32", 0, {"time_step": GRIDS}, (5, 1, 0),
     [("set_sweep_form", 2, REFUSED), ("set_sweep_form", 3, REFUSED), ("set_chain_order", 2, REFUSED), ("set_sweep_form", 1, (5, 1, 0))]),
    ("nb4", "f32", 3, {"time_step": GRIDS}, (3, 0, 0), []),
    ("nb4", "f32", 13, {"time_step": GRIDS}, (13, 0, 0), [("set_owner_rule", True, (13, 0, 0)), ("set_sweep_form", 2, REFUSED)]),
    # RK4, alone and with time grids behind it
    ("nb4", "f32", 0, {"integrator": "rk4"}, (5, 1, 0), [("set_sweep_form", 2, REFUSED), ("set_chain_order", 2, REFUSED)]),
    ("nb4", "f64", 0, {"integrator": "rk4"}, (2, 0, 0), []),
    ("nb4", "f64", 0, {"integrator": "rk4", "time_step": GRIDS}, (2, 0, 0), []),
    ("nb4", "f32", 0, {"integrator": "rk4", "time_step": GRIDS}, (5, 1, 0), [("set_sweep_form", 2, REFUSED)]),
    ("nb4", "f32", 2, {"integrator": "rk4"}, (2, 0, 0), []),
    ("nb4", "f64", 8, {"integrator": "rk4"}, (8, 0, 0), []),
    ("nb4", "f32", 3, {"integrator": "rk4"}, None, []),
    ("nb4", "f32", 4, {"integrator": "rk4"}, None, []),
    ("nb4", "f32", 13, {"integrator": "rk4"}, None, []),
    # ---- n_basis 5, 4 x 4 blocks: auto stays on kernel 1 below 64 subdomains
    ("nb5", "f32", 0, {}, (1, 0, 0), [("set_owner_rule", True, REFUSED), ("set_sweep_form", 2, REFUSED)]),
    ("nb5", "f32", 12, {}, (12, 0, 0), [("set_owner_rule", True, (12, 0, 0)), ("set_sweep_form", 2, REFUSED), ("set_chain_order", 2, REFUSED)]),
    ("nb5", "f32", 13, {}, (13, 0, 0), [("set_owner_rule", True, (13, 0, 0))]),
    ("nb5", "f32", 13, {"time_step": GRIDS}, (13, 0, 0), []),
    ("nb5", "f32", 1, {"integrator": "rk4", "time_step": GRIDS}, (1, 0, 0), []),
    ("nb5", "f64", 12, {}, None, []),
    ("nb5", "f64", 13, {}, None, []),
    ("nb5", "f32", 11, {}, None, []),
    ("nb5", "f32", 5, {}, None, []),
    ("nb5", "f32", 12, {"time_step": GRIDS}, None, []),
    ("nb5", "f32", 12, {"integrator": "rk4"}, None, []),
    ("nb5", "f32", 13, {"integrator": "rk4"}, None, []),
    # ---- n_basis 8, 2 x 2 blocks
    ("nb8", "f32", 0, {}, (7, 0, 0), [("set_sweep_form", 2, REFUSED), ("set_owner_rule", True, REFUSED)]),
    ("nb8", "f64", 0, {}, (6, 0, 0), []),
    ("nb8", "f32", 6, {}, (6, 0, 0), []),
    ("nb8", "f32", 7, {}, (7, 0, 0), []),
    ("nb8", "f32", 1, {}, (1, 0, 0), []),
    ("nb8", "f64", 7, {}, None, []),
    ("nb8", "f32", 5, {}, None, []),
    ("nb8", "f32", 0, {"time_step": GRIDS}, (1, 0, 0), []),
    ("nb8", "f64", 0, {"time_step": GRIDS}, (1, 0, 0), []),
    ("nb8", "f32", 0, {"integrator": "rk4"}, (1, 0, 0), []),
    ("nb8", "f32", 6, {"time_step": GRIDS}, None, []),
    ("nb8", "f32", 7, {"time_step": GRIDS}, None, []),
    ("nb8", "f32", 6, {"integrator": "rk4"}, None, []),
    ("nb8", "f32", 7, {"integrator": "rk4"}, None, []),
    # ---- n_basis 4, 8 x 8 blocks
    ("nb4 block 8", "f32", 0, {}, (11, 0, 0), [("set_owner_rule", True, (11, 0, 0)), ("set_sweep_form", 2, REFUSED), ("set_chain_order", 2, REFUSED)]),
    ("nb4 block 8", "f64", 0, {}, (1, 0, 0), [("set_owner_rule", True, REFUSED)]),
    ("nb4 block 8", "f32", 11, {}, (11, 0, 0), []),
    ("nb4 block 8", "f32", 11, {"time_step": GRIDS}, (11, 0, 0), [("set_owner_rule", True, (11, 0, 0))]),
    ("nb4 block 8", "f32", 0, {"time_step": GRIDS}, (11, 0, 0), []),
    ("nb4 block 8", "f32", 0, {"integrator": "rk4"}, (1, 0, 0), [("set_owner_rule", True, REFUSED)]),
    ("nb4 block 8", "f32", 0, {"integrator": "rk4", "time_step": GRIDS}, (1, 0, 0), []),
    ("nb4 block 8", "f64", 11, {}, None, []),
    ("nb4 block 8", "f32", 5, {}, None, []),
    ("nb4 block 8", "f32", 13, {}, None, []),
    ("nb4 block 8", "f32", 11, {"integrator": "rk4"}, None, []),
    # ---- label-built plans
    ("labels nb4", "f32", 0, {}, (9, 0, 0), [("set_sweep_form", 2, REFUSED), ("set_chain_order", 2, REFUSED), ("set_owner_rule", True, REFUSED)]),
    ("labels nb4", "f64", 10, {}, (10, 0, 0), []),
    ("labels nb4", "f32", 9, {"integrator": "rk4", "time_ratios": GRIDS}, (9, 0, 0), []),
    ("labels nb4", "f32", 0, {"time_ratios": GRIDS}, (9, 0, 0), []),
    ("labels nb4", "f32", 10, {"integrator": "rk4"}, (10, 0, 0), []),
    ("labels nb5", "f32", 0, {}, (10, 0, 0), []),
    ("labels nb5", "f32", 9, {}, None, []),
    ("labels nb4", "f32", 5, {}, None, []),
    ("labels nb4", "f32", 1, {}, None, []),
    ("labels nb5", "f32", 0, {"integrator": "rk4", "time_ratios": GRIDS}, (10, 0, 0), []),
]


def block_labels(nx, block):
    e = np.arange(nx * nx)
    return ((e % nx) // block + (nx // block) * ((e // nx) // block)).astype(np.int32)


def create(cd, shape, precision, kernel, kw):
    nb, nx, block, label_block = SHAPES[shape]
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(nb))
    omega, h_a = 2 * math.pi * nx / 10, np.ones(fem.size())
    if label_block:
        return fem, cd.DDH.from_labels(omega, h_a, fem, block_labels(nx, label_block), precision=precision, kernel=kernel, **kw)
    return fem, cd.DDH(omega, h_a, fem, nx, nx, precision=precision, kernel=kernel, block=block, **kw)


def state(F):
    return F.info()["kernel"], F.sweep_form(), F.chain_order()


def walk_id(w):
    shape, precision, kernel, kw, _, steps = w
    return f"{shape} {precision} kernel {kernel} {'+'.join(sorted(kw)) or 'plain'} {len(steps)} steps"


@pytest.mark.parametrize("walk", WALKS, ids=[f"{i:02d} {walk_id(w)}" for i, w in enumerate(WALKS)])
def test_setter_walk(cuda, walk):
    import torch

    import cuddhelmholtz_amd as cd

    shape, precision, kernel, kw, created, steps = walk
    if created is None:  # ValueError: from_labels refuses a kernel that is none of 0, 9, 10 before anything runs; else on first use
        with pytest.raises((RuntimeError, ValueError)):
            create(cd, shape, precision, kernel, kw)[1].info()
        return
    fem, F = create(cd, shape, precision, kernel, kw)
    assert F.info()["n_domains"] == 4
    assert state(F) == created
    assert F.integrator()[0] == kw.get("integrator", "rk2")
    grids = kw.get("time_step", kw.get("time_ratios"))
    assert list(F.time_ratios()) == ([1] * 4 if grids is None else list(grids))
    now = created
    for setter, arg, after in steps:
        if after == REFUSED:
            with pytest.raises(RuntimeError):
                getattr(F, setter)(arg)
            assert state(F) == now, (setter, arg)
        else:
            getattr(F, setter)(arg)
            assert state(F) == after, (setter, arg)
            now = after

    F.set_wh_iters(1)
    rng = np.random.default_rng(7)
    f = to_dev(torch, rng.standard_normal(2 * fem.size()), cuda)
    lam = to_dev(torch, rng.standard_normal(F.size()).astype(np.float64 if F.f64 else np.float32), cuda)
    full = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
    F.local_traces(0, 4, f, lam, full)
    halves = torch.zeros_like(full)
    F.local_traces(0, 2, f, lam, halves)
    F.local_traces(2, 4, f, lam, halves)
    assert torch.isfinite(full).all() and full.abs().max().item() > 0
    assert torch.equal(halves, full)
    assert state(F) == now
    # the operator's action takes the same plan
    y = torch.zeros_like(lam)
    F.action(lam, y)
    assert torch.isfinite(y).all() and y.abs().max().item() > 0
