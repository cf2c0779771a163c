"""DDH kernel 5's element-lane form assembles shared nodes without mask multiplications ("The write-masked
assembly"): one copy of a shared node forms the sum, the other takes it with a DPP move, and a lane without that neighbour is
not written where it used to add 0 * y.  Every written value is the same rounded sum as before, and x + 0 * y == x for
finite y up to the sign of a zero, so rhs, action and postprocess must equal those of the commit before under
np.array_equal (which takes -0.0 == 0.0; a byte comparison would not).  The dense fixtures of
tests/test_gpu_ddh_element_lane_packed.py never put an exact zero next to a masked lane; these inputs do: lambda is zero
except for one trace dof in the middle of an interior subdomain face and one where such a face meets the outer boundary (the
slot table has no slots on the outer boundary itself: its dofs have no neighbour to exchange with), so whole subdomains,
and most lanes of the others' first steps, hold exact zeros.  f is 0 for action and one wide Gaussian for rhs / postprocess.

  (i)  8 x 8 elements, n_basis 4, form 2: 4 subdomains, exactly one wavefront, through the entry points rhs, action, postprocess;
  (ii) 8 x 12 elements: 6 subdomains, so the second wavefront has two padding rows; launched whole and as the ranges (0, 1),
       (1, 6), each compared with the fixture, and the two with each other.
These are the smallest meshes that hold every (ex, ey) combination of the masks (any 4 x 4-element subdomain does) and a
padded wavefront.  The expected outputs were recorded once with the library of the commit before on an MI355X by
profiles/tools/record_element_lane_assembly_parent.py (which builds its inputs with this module's functions) into
tests/golden/element_lane_assembly/*.npz.
postprocess adds the shares of the 2 or 4 subdomains of a shared dof atomically in fp64; the order is the device's.  As in
test_gpu_ddh_element_lane_packed.py the sum of up to four fp32 values is exact, and so independent of the order, while
their exponents lie within 29 bits: the Gaussian is wide (exp(-4 r^2), at least 3e-6 of its peak everywhere) for that
reason.  The recording tool checks that two runs agree bitwise before it writes.
"""
import math
from pathlib import Path

import numpy as np
import pytest

import test_gpu_ddh_element_lane as E
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

FIXTURES = Path(__file__).resolve().parent / "golden" / "element_lane_assembly"
NAMES = ("rhs", "action", "postprocess")
MESHES = {"case_i": (8, 8), "case_ii": (8, 12)}
RANGES_II = ((0, 1), (1, 6))


def one_hot_traces(F, fem, nx, ny):
    """lambda: 1 on the real part of a trace dof inside an interior subdomain face, -0.75 on the imaginary part of one where
    an interior face meets the outer boundary, 0 elsewhere; chosen from the plan's own tables, the smallest slot of each kind"""
    info = F.info()
    nd, nl = info["n_domains"], info["n_lambda"]
    B = F.table("B").reshape(nd, 2, info["mx_fdof"])
    gI = F.table("gI").reshape(nd, info["mx_dof"])
    X = fem.physical_coordinates()
    inner, outer = [], []
    for s, d in zip(*np.nonzero(B[:, 0, :] >= 0)):
        x, y = X[:, gI[s, d]]
        on_boundary = max(abs(x), abs(y)) > 1 - 1e-12
        # subdomain faces lie on the lines x = -1 + 8 i / nx, y = -1 + 8 j / ny (4 elements per subdomain side)
        tx, ty = (x + 1) * nx / 8, (y + 1) * ny / 8
        on_x_line, on_y_line = abs(tx - round(tx)) < 1e-9, abs(ty - round(ty)) < 1e-9
        assert on_x_line or on_y_line, (s, d, x, y)
        if on_boundary:
            outer.append(int(B[s, 0, d]))
        elif on_x_line != on_y_line:  # not a cross point of the subdomain grid
            inner.append(int(B[s, 0, d]))
    assert inner and outer
    lam = np.zeros(F.size(), dtype=np.float32)
    assert lam.size == 2 * nl
    lam[min(inner)] = 1.0
    lam[nl + min(outer)] = -0.75
    return lam


def gaussian_source(fem):
    """one Gaussian, real part only: (f_re, f_im) at the dofs"""
    x, y = fem.physical_coordinates()
    return np.concatenate([np.exp(-4.0 * ((x + 0.3) ** 2 + (y - 0.2) ** 2)), np.zeros(fem.size())])


def plan(cd, name):
    nx, ny = MESHES[name]
    F, fem = E.make(cd, nx, 2, ny=ny)
    assert F.info()["kernel"] == 5 and F.sweep_form() == 2 and F.info()["n_domains"] == (nx // 4) * (ny // 4)
    return F, fem, gaussian_source(fem), one_hot_traces(F, fem, nx, ny)


def outputs_entry_points(torch, cuda, F, fem, fh, lam_h):
    """rhs (f, no lambda), action (lambda, f = 0: the form without x), postprocess (both)"""
    f, lam = to_dev(torch, fh, cuda), to_dev(torch, lam_h, cuda)
    b = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
    F.rhs(f, b)
    y = torch.zeros_like(b)
    F.action(lam, y)
    u = torch.zeros(2 * fem.size(), dtype=torch.float64, device=cuda)
    F.postprocess(lam, f, u)
    return b.cpu().numpy(), y.cpu().numpy(), u.cpu().numpy()


def outputs_ranges(torch, cuda, F, fem, fh, lam_h, ranges):
    """the same three as DDH forms them from local launches, one launch per range"""
    f, lam = to_dev(torch, fh, cuda), to_dev(torch, lam_h, cuda)
    b = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
    y = torch.zeros_like(b)
    u = torch.zeros(2 * fem.size(), dtype=torch.float64, device=cuda)
    for d0, d1 in ranges:
        F.local_traces(d0, d1, f, None, b)
        F.local_traces(d0, d1, None, lam, y)
        F.local_solution(d0, d1, lam, f, u, False)
    y.mul_(-1.0).add_(lam)
    return b.cpu().numpy(), y.cpu().numpy(), u.cpu().numpy()


def record(cd, torch, cuda, name):
    """what the fixture NAME holds: case (i) through the entry points, case (ii) as one whole launch"""
    p = plan(cd, name)
    if name == "case_i":
        return outputs_entry_points(torch, cuda, *p)
    return outputs_ranges(torch, cuda, *p, ((0, p[0].info()["n_domains"]),))


def expected(name):
    with np.load(FIXTURES / f"{name}.npz") as z:
        return tuple(z[n] for n in NAMES)


def check(out, ref, what):
    for nm, a, r in zip(NAMES, out, ref):
        assert a.dtype == r.dtype and a.shape == r.shape, (what, nm, a.dtype, r.dtype, a.shape, r.shape)
        assert np.abs(r).max() > 0, (what, nm, "the fixture is all zero")
        assert np.isfinite(a).all(), (what, nm)
        differ = int(np.count_nonzero(a != r))
        print(f"[{what}] {nm}: {a.size} values ({int(np.count_nonzero(r == 0))} exact zeros expected), {differ} differ, "
              f"max |difference| {np.abs(a.astype(np.float64) - r).max():.3e}")
        assert np.array_equal(a, r), (what, nm, differ)


def test_one_hot_traces_on_one_wavefront_equal_the_parent(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    check(record(cd, torch, cuda, "case_i"), expected("case_i"), "8x8, one-hot lambda")


def test_one_hot_traces_with_padding_rows_equal_the_parent(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    p = plan(cd, "case_ii")
    nd = p[0].info()["n_domains"]
    assert nd == 6 and RANGES_II[-1][1] == nd
    ref = expected("case_ii")
    whole = outputs_ranges(torch, cuda, *p, ((0, nd),))
    check(whole, ref, "8x12, one-hot lambda, one launch")
    ranged = outputs_ranges(torch, cuda, *p, RANGES_II)
    check(ranged, ref, "8x12, one-hot lambda, ranges")
    for nm, a, b in zip(NAMES, ranged, whole):
        assert np.array_equal(a, b), nm
