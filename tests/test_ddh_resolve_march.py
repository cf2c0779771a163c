"""How the element-lane march of DDH kernel 5 carries the velocity (march: 0 auto, 1 as wh_march_pairs_once does, 2 scaled, with the
midpoint update folded into the sweep): the rule of csrc/src/ddh_resolve.cpp (ddh_march, ddh_march_accepted) through
cuddh_ddh_resolve_march.  Host code: no GPU.  The literals are those of the comment of cuddh_hip_ddh_plan_set_march in
include/cuddh_hip.h; tests/test_gpu_ddh_element_lane_march.py asserts the same through real plans.  The plans and requests are
those tests/test_ddh_resolve_forcing.py walks."""
import ctypes as C
from dataclasses import dataclass, replace

import pytest

import test_ddh_resolve as R
import test_ddh_resolve_forcing as RF
from cuddhelmholtz_amd._native import lib

FORCING = RF.FORCING
MARCH = 5  # setting
REFUSED = None


@dataclass(frozen=True)
class Plan(RF.Plan):
    march: int = 0


def _forcing_plan(p):
    return RF.Plan(**{k: v for k, v in vars(p).items() if k != "march"})


def resolve(p, setting=0):
    """(kernel, form, order, forcing, march) in effect, or REFUSED"""
    out = (C.c_int * 5)(-7, -7, -7, -7, -7)
    err = lib.cuddh_ddh_resolve_march(p.nb, p.nel, p.nd, p.f64, p.mx_elems, p.request, p.facts, p.kernel, p.grids, p.rk4, p.form, p.order,
                                      p.forcing, p.march, setting, out)
    assert err in (0, 1)
    if err:
        assert tuple(out) == (0, 0, 0, 0, 0)
        return REFUSED
    # the first four are cuddh_ddh_resolve_forcing's: the march changes nothing of what form, order and forcing report
    assert tuple(out[:4]) == RF.resolve(_forcing_plan(p), setting if setting != MARCH else 0)
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


def test_auto_takes_the_scaled_march_where_everything_is_auto():
    assert create(**NB4, nd=8192)[1] == (5, 2, 2, 2, 2)
    assert create(**NB4, nd=65536)[1] == (5, 2, 2, 2, 2)
    assert create(**NB4, nd=8191)[1] == (5, 1, 0, 0, 0)
    assert create(**NB4, nd=4096)[1] == (5, 1, 0, 0, 0)
    assert create(**NB4, nd=8192, facts=R.ALL & ~R.LANE)[1] == (5, 1, 0, 0, 0)


@pytest.mark.parametrize("nd", [4, 8192, 65536])
def test_a_forced_form_order_or_forcing_keeps_todays_march(nd):
    p, _ = create(**NB4, nd=nd)
    for form in (2, 3):
        q, s = set_option(p, R.FORM, form=form)
        assert s == (5, form, 1, 0, 0)  # pinned chains: no forcing 2, no march
        q, s = set_option(q, R.ORDER, order=2)
        assert s == (5, form, 2, 1, 0)  # forcing 1: the scaled march is not built for it
        assert set_option(q, MARCH, march=2)[1] == (5, form, 2, 1, 0)  # accepted, idle
        q, s = set_option(q, FORCING, forcing=2)
        assert s == (5, form, 2, 2, 1)  # forced (form, 2, 2): today's march
        assert set_option(q, MARCH, march=1)[1] == (5, form, 2, 2, 1)
        assert set_option(q, MARCH, march=0)[1] == (5, form, 2, 2, 1)
        r, s = set_option(q, MARCH, march=2)
        assert s == (5, form, 2, 2, 2)  # explicit 2
        assert set_option(r, FORCING, forcing=1)[1] == (5, form, 2, 1, 0)  # and idle again without forcing 2
    if nd >= 8192:
        assert set_option(p, R.ORDER, order=2)[1] == (5, 2, 2, 1, 0)  # the order auto gives, but asked for
        assert set_option(p, R.ORDER, order=1)[1] == (5, 2, 1, 0, 0)
        q, s = set_option(p, FORCING, forcing=2)  # the forcing auto gives, but asked for
        assert s == (5, 2, 2, 2, 1)
        assert set_option(q, FORCING, forcing=0)[1] == (5, 2, 2, 2, 2)
        q, s = set_option(p, MARCH, march=1)
        assert s == (5, 2, 2, 2, 1)
        assert set_option(q, MARCH, march=0)[1] == (5, 2, 2, 2, 2)
        assert set_option(p, MARCH, march=2)[1] == (5, 2, 2, 2, 2)


def test_march_2_waits_where_forcing_2_is_not_in_effect():
    p, s = create(**NB4)
    assert s == (5, 1, 0, 0, 0)
    p, s = set_option(p, MARCH, march=2)  # accepted and idle on the matrix form, as forcing 2 is
    assert s == (5, 1, 0, 0, 0) and p.march == 2
    p, s = set_option(p, R.FORM, form=2)
    assert s == (5, 2, 1, 0, 0)
    p, s = set_option(p, R.ORDER, order=2)
    assert s == (5, 2, 2, 1, 0)
    p, s = set_option(p, FORCING, forcing=2)
    assert s == (5, 2, 2, 2, 2)
    # and stays, idle, when the plan takes time grids or RK4 afterwards; set again there it is refused
    for later in (dict(grids=1), dict(rk4=1)):
        q, s = set_option(replace(p, form=0), **later)
        assert s == (5, 1, 0, 0, 0) and q.march == 2
        assert set_option(q, MARCH, march=2)[1] is REFUSED


def test_march_2_is_refused_exactly_where_forcing_2_is():
    plans = [dict(**NB4, facts=R.ALL & ~R.LANE), dict(**NB4, f64=1), dict(**NB4, request=3), dict(**NB4, request=13), dict(**R.NB5, request=12),
             dict(**R.NB8), dict(**R.BLOCK8), dict(**NB4, request=1), dict(nb=4, nel=0, mx_elems=16), dict(**NB4), dict(**NB4, nd=8192),
             dict(**NB4, grids=1), dict(**NB4, rk4=1), dict(**NB4, nd=8192, grids=1), dict(**R.NB5, nd=64)]
    refused = 0
    for kw in plans:
        p, s = create(**kw)
        assert s is not REFUSED, kw
        forcing_2 = RF.set_option(_forcing_plan(p), FORCING, forcing=2)[1]
        q, t = set_option(p, MARCH, march=2)
        assert (t is REFUSED) == (forcing_2 is REFUSED), kw
        if t is REFUSED:
            refused += 1
            assert q == p  # a refusal leaves the plan as it was
        for march in (0, 1):  # accepted by every plan
            assert set_option(p, MARCH, march=march)[1] is not REFUSED, kw
        for bad in (-1, 3):
            assert set_option(p, MARCH, march=bad)[1] is REFUSED, kw
            assert set_option(p, FORCING, forcing=bad)[1] is REFUSED, kw  # set_forcing(3) stays refused
    assert 0 < refused < len(plans)


def test_a_stored_value_outside_the_range_is_refused_whatever_is_set():
    p, _ = create(**NB4, nd=8192)
    for bad in (-1, 3):
        assert resolve(replace(p, march=bad)) is REFUSED
        assert resolve(replace(p, march=bad), R.FORM) is REFUSED
        assert resolve(replace(p, forcing=bad), MARCH) is REFUSED
