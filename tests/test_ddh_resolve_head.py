"""What the scaled march of DDH kernel 5's element-lane form carries as the velocity (head: 0 auto, 1 q / (2 hm), multiplied by the
head coefficient of the first sweep's chain in every step, 2 that product itself): the rule of csrc/src/ddh_resolve.cpp (ddh_head,
ddh_head_accepted) through cuddh_ddh_resolve_head.  Host code: no GPU.  The literals are those of the comment of
cuddh_hip_ddh_plan_set_head in include/cuddh_hip.h; tests/test_gpu_ddh_element_lane_head.py asserts the same through real plans.
The plans and requests are those tests/test_ddh_resolve_march.py walks.

Unlike form, order, forcing and march, auto is 2 wherever the march in effect is 2, forced or not: a plan with everything auto and
the same plan forced to (2, 2, 2, 2) are compared bit for bit (tests/test_gpu_ddh_element_lane_rectangles.py), so they run one
kernel.  Only an explicit 1 keeps the bits march 2 had before."""
import ctypes as C
from dataclasses import dataclass, replace

import pytest

import test_ddh_resolve as R
import test_ddh_resolve_march as RM
from cuddhelmholtz_amd._native import lib

FORCING = RM.FORCING
MARCH = RM.MARCH
HEAD = 6  # setting
REFUSED = None


@dataclass(frozen=True)
class Plan(RM.Plan):
    head: int = 0


def _march_plan(p):
    return RM.Plan(**{k: v for k, v in vars(p).items() if k != "head"})


def resolve(p, setting=0):
    """(kernel, form, order, forcing, march, head) in effect, or REFUSED"""
    out = (C.c_int * 6)(-7, -7, -7, -7, -7, -7)
    err = lib.cuddh_ddh_resolve_head(p.nb, p.nel, p.nd, p.f64, p.mx_elems, p.request, p.facts, p.kernel, p.grids, p.rk4, p.form, p.order,
                                     p.forcing, p.march, p.head, setting, out)
    assert err in (0, 1)
    if err:
        assert tuple(out) == (0, 0, 0, 0, 0, 0)
        return REFUSED
    # the first five are cuddh_ddh_resolve_march's: the head changes nothing of what the other four report
    assert tuple(out[:5]) == RM.resolve(_march_plan(p), setting if setting != HEAD else 0)
    assert out[5] == (0 if out[4] != 2 else 1 if p.head == 1 else 2)  # the whole rule
    return tuple(out)


def create(**kw):
    p = Plan(**kw)
    state = resolve(p)
    return (None, REFUSED) if state is REFUSED else (replace(p, kernel=state[0]), state)


def set_option(p, setting=0, **kw):
    """a setter: (plan after, state after), the plan unchanged where the call is refused"""
    q = replace(p, **kw)
    state = resolve(q, setting)
    return (p, REFUSED) if state is REFUSED else (replace(q, kernel=state[0]), state)


NB4 = R.NB4


def test_auto_carries_the_head_wherever_the_scaled_march_is_in_effect():
    assert create(**NB4, nd=8192)[1] == (5, 2, 2, 2, 2, 2)
    assert create(**NB4, nd=65536)[1] == (5, 2, 2, 2, 2, 2)
    assert create(**NB4, nd=8191)[1] == (5, 1, 0, 0, 0, 0)
    assert create(**NB4, nd=4096)[1] == (5, 1, 0, 0, 0, 0)
    assert create(**NB4, nd=8192, facts=R.ALL & ~R.LANE)[1] == (5, 1, 0, 0, 0, 0)


@pytest.mark.parametrize("nd", [4, 8192, 65536])
def test_a_forced_march_2_carries_the_head_too_and_only_head_1_keeps_its_bits(nd):
    p, _ = create(**NB4, nd=nd)
    for form in (2, 3):
        q, s = set_option(p, R.FORM, form=form)
        assert s == (5, form, 1, 0, 0, 0)
        assert set_option(q, HEAD, head=2)[1] == (5, form, 1, 0, 0, 0)  # accepted, idle
        q, s = set_option(q, R.ORDER, order=2)
        assert s == (5, form, 2, 1, 0, 0)
        q, s = set_option(q, FORCING, forcing=2)
        assert s == (5, form, 2, 2, 1, 0)  # march 1: nothing to carry
        assert set_option(q, HEAD, head=2)[1] == (5, form, 2, 2, 1, 0)
        q, s = set_option(q, MARCH, march=2)
        assert s == (5, form, 2, 2, 2, 2)  # forced (form, 2, 2, 2), head auto: carried
        assert set_option(q, HEAD, head=2)[1] == (5, form, 2, 2, 2, 2)
        r, s = set_option(q, HEAD, head=1)
        assert s == (5, form, 2, 2, 2, 1)  # the bits of march 2 as they were
        assert set_option(r, HEAD, head=0)[1] == (5, form, 2, 2, 2, 2)
        assert set_option(r, MARCH, march=1)[1] == (5, form, 2, 2, 1, 0)  # idle again without march 2
        assert set_option(r, FORCING, forcing=1)[1] == (5, form, 2, 1, 0, 0)
    if nd >= 8192:
        q, s = set_option(p, HEAD, head=1)
        assert s == (5, 2, 2, 2, 2, 1)  # everything else auto
        assert set_option(q, HEAD, head=0)[1] == (5, 2, 2, 2, 2, 2)
        assert set_option(p, HEAD, head=2)[1] == (5, 2, 2, 2, 2, 2)
        assert set_option(p, MARCH, march=1)[1] == (5, 2, 2, 2, 1, 0)
        assert set_option(p, MARCH, march=2)[1] == (5, 2, 2, 2, 2, 2)
        assert set_option(p, FORCING, forcing=2)[1] == (5, 2, 2, 2, 1, 0)  # a forced forcing keeps march 1, so no head


def test_head_2_waits_where_march_2_is_not_in_effect():
    p, s = create(**NB4)
    assert s == (5, 1, 0, 0, 0, 0)
    p, s = set_option(p, HEAD, head=2)  # accepted and idle on the matrix form, as march 2 is
    assert s == (5, 1, 0, 0, 0, 0) and p.head == 2
    p, s = set_option(p, R.FORM, form=2)
    assert s == (5, 2, 1, 0, 0, 0)
    p, s = set_option(p, R.ORDER, order=2)
    assert s == (5, 2, 2, 1, 0, 0)
    p, s = set_option(p, FORCING, forcing=2)
    assert s == (5, 2, 2, 2, 1, 0)
    p, s = set_option(p, MARCH, march=2)
    assert s == (5, 2, 2, 2, 2, 2)
    # and stays, idle, when the plan takes time grids or RK4 afterwards; set again there it is refused
    for later in (dict(grids=1), dict(rk4=1)):
        q, s = set_option(replace(p, form=0), **later)
        assert s == (5, 1, 0, 0, 0, 0) and q.head == 2
        assert set_option(q, HEAD, head=2)[1] is REFUSED
        assert set_option(q, HEAD, head=1)[1] == (5, 1, 0, 0, 0, 0)


def test_head_2_is_refused_exactly_where_march_2_is():
    plans = [dict(**NB4, facts=R.ALL & ~R.LANE), dict(**NB4, f64=1), dict(**NB4, request=3), dict(**NB4, request=13), dict(**R.NB5, request=12),
             dict(**R.NB8), dict(**R.BLOCK8), dict(**NB4, request=1), dict(nb=4, nel=0, mx_elems=16), dict(**NB4), dict(**NB4, nd=8192),
             dict(**NB4, grids=1), dict(**NB4, rk4=1), dict(**NB4, nd=8192, grids=1), dict(**R.NB5, nd=64)]
    refused = 0
    for kw in plans:
        p, s = create(**kw)
        assert s is not REFUSED, kw
        march_2 = RM.set_option(_march_plan(p), MARCH, march=2)[1]
        q, t = set_option(p, HEAD, head=2)
        assert (t is REFUSED) == (march_2 is REFUSED), kw
        if t is REFUSED:
            refused += 1
            assert q == p  # a refusal leaves the plan as it was
        for head in (0, 1):  # accepted by every plan
            assert set_option(p, HEAD, head=head)[1] is not REFUSED, kw
        for bad in (-1, 3):
            assert set_option(p, HEAD, head=bad)[1] is REFUSED, kw
            assert set_option(p, MARCH, march=bad)[1] is REFUSED, kw  # set_march(3) stays refused
    assert 0 < refused < len(plans)


def test_a_stored_value_outside_the_range_is_refused_whatever_is_set():
    p, _ = create(**NB4, nd=8192)
    for bad in (-1, 3):
        assert resolve(replace(p, head=bad)) is REFUSED
        assert resolve(replace(p, head=bad), R.FORM) is REFUSED
        assert resolve(replace(p, head=bad), MARCH) is REFUSED
        assert resolve(replace(p, march=bad), HEAD) is REFUSED
        assert resolve(replace(p, forcing=bad), HEAD) is REFUSED
