"""Which kernel, sweep form and chain order a DDH plan runs: the rule of csrc/src/ddh_resolve.cpp through cuddh_ddh_resolve.  Host
code: no GPU.  The literals are those of the comments in include/cuddh_hip.h (cuddh_hip_ddh_plan_create and the setters);
tests/test_gpu_ddh_plan_resolution.py asserts the same through real plans."""
import ctypes as C
from dataclasses import dataclass, replace

import pytest

from cuddhelmholtz_amd._native import lib

S, U, I, DENSE, SEP8, LANE = (1 << c for c in range(1, 7))  # facts: 1 << check
ALL = S | U | I | DENSE | SEP8 | LANE
FORM, ORDER, OWNER = 1, 2, 3  # setting
REFUSED = None


@dataclass(frozen=True)
class Plan:
    """the integers a plan holds; `kernel` 0 until created"""
    nb: int = 4
    nel: int = 4
    nd: int = 4
    f64: int = 0
    mx_elems: int = 0
    request: int = 0
    facts: int = ALL
    kernel: int = 0
    grids: int = 0
    rk4: int = 0
    form: int = 0
    order: int = 0


def call(p, setting=0):
    """(kernel, form in effect, order in effect) or REFUSED, and the checks"""
    out = (C.c_int * 4)(-7, -7, -7, -7)
    err = lib.cuddh_ddh_resolve(p.nb, p.nel, p.nd, p.f64, p.mx_elems, p.request, p.facts, p.kernel, p.grids, p.rk4, p.form, p.order, setting, out)
    assert err in (0, 1)
    if err:
        assert tuple(out[:3]) == (0, 0, 0)
        return REFUSED, out[3]
    return tuple(out[:3]), out[3]


def resolve(p, setting=0):
    return call(p, setting)[0]


def create(**kw):
    """the plan after creation: (plan with its kernel, state), or (None, REFUSED)"""
    p = Plan(**kw)
    state = resolve(p)
    return (None, REFUSED) if state is REFUSED else (replace(p, kernel=state[0]), state)


def set_option(p, setting=0, **kw):
    """a setter: (plan after, state after), the plan unchanged where the call is refused"""
    q = replace(p, **kw)
    state = resolve(q, setting)
    return (p, REFUSED) if state is REFUSED else (replace(q, kernel=state[0]), state)


def checks(p):
    """the checks plan creation runs, in order"""
    c, out = call(p)[1], []
    if c < 0:
        return REFUSED
    while c:
        out.append(1 << (c & 15))
        c >>= 4
    return out


NB4 = dict(nb=4, nel=4)
NB5 = dict(nb=5, nel=4)
NB8 = dict(nb=8, nel=2)
BLOCK8 = dict(nb=4, nel=8)


def test_auto_n_basis_4():
    assert create(**NB4)[1] == (5, 1, 0)
    assert create(**NB4, f64=1)[1] == (3, 0, 0)
    assert create(**NB4, facts=ALL & ~DENSE)[1] == (3, 0, 0)
    assert create(**NB4, facts=S)[1] == (3, 0, 0)
    assert create(**NB4, facts=0)[1] == (1, 0, 0)
    assert create(**NB4, facts=ALL & ~S)[1] == (1, 0, 0)
    assert create(**NB4, f64=1, facts=0)[1] == (1, 0, 0)


def test_sweep_form_and_chain_order_under_auto():
    assert create(**NB4, nd=8192)[1] == (5, 2, 2)
    assert create(**NB4, nd=8191)[1] == (5, 1, 0)
    assert create(**NB4, nd=8192, facts=ALL & ~LANE)[1] == (5, 1, 0)
    assert create(**NB4, nd=65536)[1] == (5, 2, 2)


@pytest.mark.parametrize("nd", [4, 8192])
def test_forced_forms(nd):
    p, _ = create(**NB4, nd=nd)
    p, s = set_option(p, FORM, form=2)
    assert s == (5, 2, 1)  # a forced form keeps the pinned chains
    p, s = set_option(p, ORDER, order=2)
    assert s == (5, 2, 2)
    p, s = set_option(p, FORM, form=3)
    assert s == (5, 3, 2)
    p, s = set_option(p, ORDER, order=0)
    assert s == (5, 3, 1)
    p, s = set_option(p, FORM, form=1)
    assert s == (5, 1, 0)
    assert set_option(p, FORM, form=4)[1] is REFUSED and set_option(p, FORM, form=-1)[1] is REFUSED
    assert set_option(p, ORDER, order=3)[1] is REFUSED and set_option(p, ORDER, order=-1)[1] is REFUSED
    p, s = set_option(p, FORM, form=0)
    assert s == ((5, 2, 2) if nd >= 8192 else (5, 1, 0))


def test_forced_form_needs_kernel_5_and_its_tables():
    for kw in (dict(**NB4, facts=ALL & ~LANE), dict(**NB4, f64=1), dict(**NB4, request=3), dict(**NB4, request=13), dict(**NB5, request=12),
               dict(**NB8), dict(**BLOCK8), dict(**NB4, request=1), dict(nb=4, nel=0, mx_elems=16)):
        p, s = create(**kw)
        assert s is not REFUSED, kw
        for form in (2, 3):
            assert set_option(p, FORM, form=form)[1] is REFUSED, kw
        for form in (0, 1):
            assert set_option(p, FORM, form=form)[1] == s, kw
        assert set_option(p, ORDER, order=2)[1] is REFUSED, kw
        for order in (0, 1):
            assert set_option(p, ORDER, order=order)[1] == s, kw


def test_chain_order_2_on_a_form_1_plan_takes_effect_with_the_form():
    p, _ = create(**NB4)
    p, s = set_option(p, ORDER, order=2)
    assert s == (5, 1, 0) and p.order == 2
    assert set_option(p, FORM, form=2)[1] == (5, 2, 2)
    # and stays, idle, when the plan takes time grids or RK4 afterwards; set again there it is refused
    for later in (dict(grids=1), dict(rk4=1)):
        q, s = set_option(p, **later)
        assert s == (5, 1, 0) and q.order == 2
        assert set_option(q, ORDER, order=2)[1] is REFUSED
        assert set_option(q, ORDER, order=1)[1] == (5, 1, 0)


def test_n_basis_5():
    assert create(**NB5, nd=64)[1] == (12, 0, 0)
    assert create(**NB5, nd=63)[1] == (1, 0, 0)
    for fact in (S, U, I, LANE):
        assert create(**NB5, nd=64, facts=ALL & ~fact)[1] == (1, 0, 0)
        for request in (12, 13):
            assert create(**NB5, request=request, facts=ALL & ~fact)[1] is REFUSED
    assert create(**NB5, nd=64, f64=1)[1] == (1, 0, 0)
    for request in (12, 13):
        for nd in (1, 4, 64, 100000):
            assert create(**NB5, nd=nd, request=request)[1] == (request, 0, 0)
        assert create(**NB5, request=request, f64=1)[1] is REFUSED


def test_n_basis_8():
    assert create(**NB8)[1] == (7, 0, 0)
    assert create(**NB8, facts=ALL & ~SEP8)[1] == (6, 0, 0)
    assert create(**NB8, facts=S)[1] == (6, 0, 0)
    assert create(**NB8, f64=1)[1] == (6, 0, 0)
    assert create(**NB8, facts=0)[1] == (1, 0, 0)
    assert create(**NB8, request=6)[1] == (6, 0, 0) and create(**NB8, request=6, f64=1)[1] == (6, 0, 0)
    assert create(**NB8, request=7)[1] == (7, 0, 0)
    assert create(**NB8, request=7, f64=1)[1] is REFUSED
    assert create(**NB8, request=7, facts=ALL & ~SEP8)[1] is REFUSED
    assert create(**NB8, request=6, facts=0)[1] is REFUSED


def test_blocks_of_8_at_n_basis_4():
    assert create(**BLOCK8)[1] == (11, 0, 0)
    assert create(**BLOCK8, request=11)[1] == (11, 0, 0)
    assert create(**BLOCK8, f64=1)[1] == (1, 0, 0)
    for fact in (S, U, I, LANE):
        assert create(**BLOCK8, facts=ALL & ~fact)[1] == (1, 0, 0)
        assert create(**BLOCK8, request=11, facts=ALL & ~fact)[1] is REFUSED
    assert create(**BLOCK8, request=11, f64=1)[1] is REFUSED


HOME = {2: [NB4], 3: [NB4], 4: [NB4], 5: [NB4], 6: [NB8], 7: [NB8], 8: [NB4], 11: [BLOCK8], 12: [NB5], 13: [NB4, NB5]}
SHAPES = [NB4, NB5, NB8, BLOCK8, dict(nb=4, nel=2), dict(nb=6, nel=3), dict(nb=3, nel=4), dict(nb=10, nel=3), dict(nb=2, nel=16)]


@pytest.mark.parametrize("request_", sorted(HOME))
def test_every_kernel_is_refused_on_a_shape_not_its_own(request_):
    for shape in SHAPES:
        for f64 in (0, 1):
            p = Plan(**shape, f64=f64, request=request_)
            at_home = shape in HOME[request_] and f64 == {5: 0, 7: 0, 8: 1, 11: 0, 12: 0, 13: 0}.get(request_, f64)
            assert (resolve(p) == (request_, 1 if request_ == 5 else 0, 0)) if at_home else (resolve(p) is REFUSED), (shape, f64)
            assert (checks(p) is REFUSED) == (not at_home)
    # kernel 1 runs every shape of at most 1024 element nodes, and no other
    for shape in SHAPES:
        assert create(**shape, request=1)[1] == (1, 0, 0)
    for shape in (dict(nb=1, nel=4), dict(nb=11, nel=1), dict(nb=4, nel=0), dict(nb=4, nel=17), dict(nb=9, nel=4), dict(nb=10, nel=4)):
        for request in (0, 1):
            assert create(**shape, request=request)[1] is REFUSED
    for request in (-1, 9, 10, 14):
        assert create(**NB4, request=request)[1] is REFUSED


def test_label_built_plans():
    fits = dict(nb=4, nel=0, mx_elems=16)
    assert create(**fits)[1] == (9, 0, 0)
    assert create(**fits, request=9)[1] == (9, 0, 0) and create(**fits, request=10)[1] == (10, 0, 0)
    assert create(**fits, f64=1, facts=0)[1] == (9, 0, 0)
    assert create(nb=4, nel=0, mx_elems=1)[1] == (9, 0, 0)
    for other in (dict(nb=5, nel=0, mx_elems=9), dict(nb=3, nel=0, mx_elems=16), dict(nb=3, nel=0, mx_elems=28), dict(nb=2, nel=0, mx_elems=64)):
        assert create(**other)[1] == (10, 0, 0)
        assert create(**other, request=10)[1] == (10, 0, 0)
        assert create(**other, request=9)[1] is REFUSED
    assert create(nb=4, nel=0, mx_elems=17)[1] is REFUSED  # 272 element nodes: more than 256
    assert create(nb=2, nel=0, mx_elems=65)[1] is REFUSED
    for request in list(range(1, 9)) + [11, 12, 13]:
        assert create(**fits, request=request)[1] is REFUSED
        assert create(nb=5, nel=0, mx_elems=9, request=request)[1] is REFUSED
    for p in (create(**fits)[0], create(nb=5, nel=0, mx_elems=9)[0]):
        for later in (dict(grids=1), dict(rk4=1), dict(grids=1, rk4=1)):
            assert set_option(p, **later)[1] == (p.kernel, 0, 0)


def test_time_grids():
    for shape, kernel in ((NB8, 7), (dict(**NB8, f64=1), 6), (dict(**NB5, nd=64), 12)):
        p, s = create(**shape)
        assert s == (kernel, 0, 0)
        assert set_option(p, grids=1)[1] == (1, 0, 0)
        p, s = create(**shape, request=kernel)
        assert s == (kernel, 0, 0)
        q, s = set_option(p, grids=1)
        assert s is REFUSED and q == p
    p, _ = create(**NB4, nd=8192)
    assert set_option(p, grids=1)[1] == (5, 1, 0)
    for form in (2, 3):
        q, _ = set_option(p, FORM, form=form)
        assert set_option(q, grids=1)[1] is REFUSED
        g, _ = set_option(p, grids=1)
        assert set_option(g, FORM, form=form)[1] is REFUSED
    for shape, request in ((NB4, 13), (NB5, 13), (BLOCK8, 11), (BLOCK8, 0), (NB4, 1), (NB4, 2), (NB4, 3), (NB4, 4), (dict(**NB4, f64=1), 8)):
        p, s = create(**shape, request=request)
        assert set_option(p, grids=1)[1] == s and s is not REFUSED


def test_rk4():
    p, _ = create(**NB4, f64=1)
    assert set_option(p, rk4=1)[1] == (2, 0, 0)  # auto 3 -> 2
    for shape in (NB8, dict(**NB8, f64=1), BLOCK8, dict(**NB5, nd=64)):
        p, s = create(**shape)
        assert s[0] in (6, 7, 11, 12)
        assert set_option(p, rk4=1)[1] == (1, 0, 0)
    for shape, request in ((NB4, 3), (NB4, 4), (NB8, 6), (NB8, 7), (BLOCK8, 11), (NB5, 12), (NB4, 13), (NB5, 13)):
        p, s = create(**shape, request=request)
        assert s[0] == request
        q, s = set_option(p, rk4=1)
        assert s is REFUSED and q == p
    p, _ = create(**NB4, nd=8192)
    assert set_option(p, rk4=1)[1] == (5, 1, 0)
    for form in (2, 3):
        q, _ = set_option(p, FORM, form=form)
        assert set_option(q, rk4=1)[1] is REFUSED
        r, _ = set_option(p, rk4=1)
        assert set_option(r, FORM, form=form)[1] is REFUSED
    for shape, request in ((NB4, 1), (NB4, 2), (NB4, 5), (dict(**NB4, f64=1), 8), (dict(nb=4, nel=0, mx_elems=16), 9), (dict(nb=4, nel=0, mx_elems=16), 10)):
        p, s = create(**shape, request=request)
        assert set_option(p, rk4=1)[1] == s and s[0] == request


def test_taking_rk4_back_leaves_the_moved_kernel():
    for shape, moved in ((dict(**NB4, f64=1), 2), (NB8, 1), (BLOCK8, 1), (dict(**NB5, nd=64), 1)):
        p, _ = create(**shape)
        p, s = set_option(p, rk4=1)
        assert s == (moved, 0, 0)
        p, s = set_option(p, rk4=0)
        assert s == (moved, 0, 0) and p.rk4 == 0
        assert resolve(p) == (moved, 0, 0)  # resolving again changes nothing
    # RK4 and time grids in either order end on the same kernel
    for shape in (NB8, BLOCK8, dict(**NB4, f64=1)):
        p, _ = create(**shape)
        a = set_option(set_option(p, rk4=1)[0], grids=1)[1]
        b = set_option(set_option(p, grids=1)[0], rk4=1)[1]
        assert a == b and a is not REFUSED


def test_chain_order_2_is_refused_with_grids_or_rk4():
    p, _ = create(**NB4)
    for later in (dict(grids=1), dict(rk4=1)):
        q, _ = set_option(p, **later)
        assert set_option(q, ORDER, order=2)[1] is REFUSED


def test_owner_rule():
    for shape, request, takes in ((BLOCK8, 0, True), (BLOCK8, 11, True), (NB5, 12, True), (dict(**NB5, nd=64), 0, True), (NB4, 13, True), (NB5, 13, True),
                                  (NB4, 0, False), (NB4, 1, False), (NB4, 2, False), (NB4, 3, False), (NB4, 4, False), (dict(**NB4, f64=1), 8, False),
                                  (NB8, 6, False), (NB8, 7, False), (NB5, 0, False), (dict(nb=4, nel=0, mx_elems=16), 9, False),
                                  (dict(nb=4, nel=0, mx_elems=16), 10, False)):
        p, s = create(**shape, request=request)
        assert s is not REFUSED
        assert (resolve(p, OWNER) == s) if takes else (resolve(p, OWNER) is REFUSED), (shape, request)
    p, _ = create(**NB4, nd=8192)
    assert resolve(set_option(p, FORM, form=2)[0], OWNER) is REFUSED  # kernel 5's rule is its form 3
    # an auto plan moved off kernel 12 keeps running; the rule can no longer be set
    p, _ = create(**NB5, nd=64)
    p, s = set_option(p, grids=1)
    assert s == (1, 0, 0) and resolve(p, OWNER) is REFUSED


def test_checks_plan_creation_runs():
    assert checks(Plan(**NB4)) == [S, U, I, DENSE, LANE]
    assert checks(Plan(**NB4, request=5)) == [S, U, I, DENSE, LANE]
    assert checks(Plan(**NB4, f64=1)) == [S]
    assert checks(Plan(**NB4, f64=1, request=8)) == [S, U, I, DENSE]
    for request in (2, 3, 4):
        assert checks(Plan(**NB4, request=request)) == [S]
    assert checks(Plan(**NB4, request=13)) == [S, U, I, LANE]
    assert checks(Plan(**NB8)) == [S, U, SEP8] and checks(Plan(**NB8, request=7)) == [S, U, SEP8]
    assert checks(Plan(**NB8, f64=1)) == [S] and checks(Plan(**NB8, request=6)) == [S]
    assert checks(Plan(**BLOCK8)) == [S, I, U, LANE] and checks(Plan(**BLOCK8, request=11)) == [S, I, U, LANE]
    assert checks(Plan(**BLOCK8, f64=1)) == []
    assert checks(Plan(**NB5, nd=64)) == [S, I, U, LANE] and checks(Plan(**NB5, nd=63)) == []
    assert checks(Plan(**NB5, request=12)) == [S, I, U, LANE] and checks(Plan(**NB5, request=13)) == [S, I, U, LANE]
    assert checks(Plan(**NB5, nd=64, f64=1)) == []
    for shape in SHAPES:
        assert checks(Plan(**shape, request=1)) == []
    assert checks(Plan(nb=6, nel=3)) == [] and checks(Plan(nb=4, nel=0, mx_elems=16)) == []
