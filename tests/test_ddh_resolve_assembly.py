"""How the carried march of DDH kernel 5's element-lane form (head 2) forms the neighbour sums of its sweeps (assembly: 0 auto, 1 DPP on
the vector pipe, 2 fetched both ways over the LDS pipe): the rule of csrc/src/ddh_resolve.cpp (ddh_assembly, ddh_assembly_accepted)
through cuddh_ddh_resolve_assembly.  Host code: no GPU.  The literals are those of the comment of cuddh_hip_ddh_plan_set_assembly in
include/cuddh_hip.h; tests/test_gpu_ddh_element_lane_fetched_assembly.py asserts the same through real plans.  The plans and requests are
those tests/test_ddh_resolve_head.py walks.

Unlike the head, 2 is accepted only where head 2 is IN EFFECT when it is set: the two assemblies give the same bits, so there is
nothing for a stored 2 to wait for, and a caller that asks for it on a plan that cannot run it is told so.  A stored 2 goes idle,
and comes back, with the head."""
import ctypes as C
from dataclasses import dataclass, replace

import pytest

import test_ddh_resolve as R
import test_ddh_resolve_head as RH
from cuddhelmholtz_amd._native import lib

FORCING, MARCH, HEAD = RH.FORCING, RH.MARCH, RH.HEAD
ASSEMBLY = 7  # setting
REFUSED = None
AUTO = 2  # DDH_ASSEMBLY_AUTO of csrc/src/ddh_resolve.cpp: what auto takes from ELEMENT_LANE_MIN_DOMAINS subdomains on
MIN_DOMAINS = 8192


@dataclass(frozen=True)
class Plan(RH.Plan):
    assembly: int = 0


def _head_plan(p):
    return RH.Plan(**{k: v for k, v in vars(p).items() if k != "assembly"})


def resolve(p, setting=0):
    """(kernel, form, order, forcing, march, head, assembly) in effect, or REFUSED"""
    out = (C.c_int * 7)(*([-7] * 7))
    err = lib.cuddh_ddh_resolve_assembly(p.nb, p.nel, p.nd, p.f64, p.mx_elems, p.request, p.facts, p.kernel, p.grids, p.rk4, p.form, p.order,
                                         p.forcing, p.march, p.head, p.assembly, setting, out)
    assert err in (0, 1)
    if err:
        assert tuple(out) == (0,) * 7
        return REFUSED
    # the first six are cuddh_ddh_resolve_head's: the assembly changes nothing of what the others report
    assert tuple(out[:6]) == RH.resolve(_head_plan(p), setting if setting != ASSEMBLY else 0)
    auto = AUTO if p.nd >= MIN_DOMAINS else 1
    assert out[6] == (0 if out[5] != 2 else p.assembly if p.assembly != 0 else auto)  # the whole rule
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


def test_what_auto_takes():
    assert create(**NB4, nd=8192)[1] == (5, 2, 2, 2, 2, 2, AUTO)
    assert create(**NB4, nd=65536)[1] == (5, 2, 2, 2, 2, 2, AUTO)
    assert create(**NB4, nd=8191)[1] == (5, 1, 0, 0, 0, 0, 0)
    assert create(**NB4, nd=8192, facts=R.ALL & ~R.LANE)[1] == (5, 1, 0, 0, 0, 0, 0)
    # below the threshold head 2 is in effect only where it is forced: auto stays with DPP there, whatever it takes above
    p, _ = create(**NB4, nd=4)
    p, s = set_option(p, R.FORM, form=2)
    p, s = set_option(p, R.ORDER, order=2)
    p, s = set_option(p, FORCING, forcing=2)
    p, s = set_option(p, MARCH, march=2)
    assert s == (5, 2, 2, 2, 2, 2, 1)


@pytest.mark.parametrize("nd", [4, 8192, 65536])
def test_2_is_accepted_only_where_head_2_is_in_effect(nd):
    p, _ = create(**NB4, nd=nd)
    for form in (2, 3):
        q, s = set_option(p, R.FORM, form=form)
        assert s == (5, form, 1, 0, 0, 0, 0)
        r, t = set_option(q, ASSEMBLY, assembly=2)
        assert t is REFUSED and r == q  # a refusal leaves the plan as it was
        q, s = set_option(q, R.ORDER, order=2)
        assert set_option(q, ASSEMBLY, assembly=2)[1] is REFUSED
        q, s = set_option(q, FORCING, forcing=2)
        assert s == (5, form, 2, 2, 1, 0, 0)
        assert set_option(q, ASSEMBLY, assembly=2)[1] is REFUSED
        assert set_option(q, ASSEMBLY, assembly=1)[1] == (5, form, 2, 2, 1, 0, 0)  # 0 and 1 are accepted by every plan, idle here
        q, s = set_option(q, MARCH, march=2)
        assert s[:6] == (5, form, 2, 2, 2, 2) and s[6] in (1, 2)
        one, s = set_option(q, HEAD, head=1)
        assert s == (5, form, 2, 2, 2, 1, 0)
        assert set_option(one, ASSEMBLY, assembly=2)[1] is REFUSED  # head 1 has the DPP assembly alone
        two, s = set_option(q, ASSEMBLY, assembly=2)
        assert s == (5, form, 2, 2, 2, 2, 2)
        assert set_option(two, ASSEMBLY, assembly=1)[1] == (5, form, 2, 2, 2, 2, 1)
        assert set_option(two, ASSEMBLY, assembly=0)[1] == set_option(q, ASSEMBLY, assembly=0)[1]
        # stored, it goes idle with the head and comes back with it
        idle, s = set_option(two, HEAD, head=1)
        assert s == (5, form, 2, 2, 2, 1, 0) and idle.assembly == 2
        assert set_option(idle, HEAD, head=0)[1] == (5, form, 2, 2, 2, 2, 2)
        assert set_option(two, MARCH, march=1)[1] == (5, form, 2, 2, 1, 0, 0)
    if nd >= MIN_DOMAINS:
        q, s = set_option(p, ASSEMBLY, assembly=2)
        assert s == (5, 2, 2, 2, 2, 2, 2)  # everything else auto
        assert set_option(q, ASSEMBLY, assembly=1)[1] == (5, 2, 2, 2, 2, 2, 1)
        assert set_option(q, ASSEMBLY, assembly=0)[1] == (5, 2, 2, 2, 2, 2, AUTO)
    else:
        assert set_option(p, ASSEMBLY, assembly=2)[1] is REFUSED  # the matrix form


def test_2_is_refused_on_every_plan_without_head_2_and_values_out_of_range_on_all():
    plans = [dict(**NB4, facts=R.ALL & ~R.LANE), dict(**NB4, f64=1), dict(**NB4, request=3), dict(**NB4, request=13), dict(**R.NB5, request=12),
             dict(**R.NB8), dict(**R.BLOCK8), dict(**NB4, request=1), dict(nb=4, nel=0, mx_elems=16), dict(**NB4), dict(**NB4, nd=8192),
             dict(**NB4, grids=1), dict(**NB4, rk4=1), dict(**NB4, nd=8192, grids=1), dict(**R.NB5, nd=64)]
    accepted = 0
    for kw in plans:
        p, s = create(**kw)
        assert s is not REFUSED, kw
        q, t = set_option(p, ASSEMBLY, assembly=2)
        assert (t is REFUSED) == (s[5] != 2), kw
        if t is REFUSED:
            assert q == p
        else:
            accepted += 1
        for assembly in (0, 1):
            assert set_option(p, ASSEMBLY, assembly=assembly)[1] is not REFUSED, kw
        for bad in (-1, 3):
            assert set_option(p, ASSEMBLY, assembly=bad)[1] is REFUSED, kw
            assert resolve(replace(p, assembly=bad)) is REFUSED, kw  # stored, whatever is set
            assert resolve(replace(p, assembly=bad), HEAD) is REFUSED, kw
            assert resolve(replace(p, head=bad), ASSEMBLY) is REFUSED, kw
    assert accepted == 1  # the plan auto gives the carried head
