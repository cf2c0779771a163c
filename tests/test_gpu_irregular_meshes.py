"""The plan kernels of csrc/kernels/helmholtz_fused.hip on meshes whose topology the fixture meshes do not have
(tests/irregular_meshes.py; admitted and their layouts confirmed, without a GPU, in tests/test_irregular_meshes.py):

  * stars whose centre vertex is touched by five or six patches: the border kernels fetch a dof's first four slots together
    and add the rest in a tail loop that no other mesh of the suite enters;
  * valence 3, rings with two boundary loops, elements with boundary faces on opposite sides, proper subsets of the boundary;
  * 31 colours in one patch, and a mesh whose plan is refused (a 32nd colour): the null-plan paths of HelmholtzOperator,
    its gmres() and the single operators;
  * rectangles whose elements differ only in the orientation of their local axes: the uniform-metric decision.

Rules, as in tests/test_gpu_parity.py: the reference is the oracle (Stiffness, Mass with a random coefficient, helmholtz_apply)
on random x, a2, ax; relative l2 < 1e-12 against it; two forms of one apply agree to < 1e-13; a repetition is bitwise equal;
action_native between to_native / from_native is bitwise action.  At every dof with more than four slots, also
|y - ref| <= 1e-12 max|ref|: the norm cannot average a lost slot away."""
import functools

import numpy as np
import pytest

import irregular_meshes as im
import oracle
from test_patch_layout import build_layout, space_of

pytestmark = pytest.mark.gpu

OMEGA = 7.0


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


def to_dev(torch, a, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)  # (the cases are read-only)


def host(t):
    return t.cpu().numpy()


class Case:
    """one mesh (elements optionally turned), order and list of boundary faces: the product's mesh, the inputs and the oracle's
    results, computed once and never written to"""

    def __init__(self, name, nb, faces="all", shifts=None):
        import cuddhelmholtz_amd as cd

        xy, elems = im.by_name(name)
        if shifts is not None:
            elems = im.rotate_elements(elems, np.asarray(shifts))
        self.pm, om = cd.Mesh2D.from_vertices(xy, elems), oracle.Mesh(xy, elems)
        self.nb, self.d = nb, oracle.Discretization(om, nb)
        self.n = n = self.d.ndof
        boundary = self.pm.boundary_edges()
        assert np.array_equal(boundary, np.asarray(om.boundary_edges))
        if faces == "all":
            self.faces = boundary
        elif faces == "every other":
            self.faces = boundary[::2]
        else:  # the annulus's inner loop: the boundary edges between two vertices of the smaller radius
            radius = np.hypot(*xy[self.pm.edges()[boundary, 1:3]].transpose(2, 0, 1))
            self.faces = boundary[np.all(radius < 0.75, axis=1)]
            assert 0 < len(self.faces) < len(boundary)
        self.ofs = ofs = oracle.FaceSpaceO(self.d, list(self.faces))
        rng = np.random.default_rng(1000 * nb + len(elems))
        self.x, self.a2, self.ax = rng.standard_normal(2 * n), 0.5 + rng.random(n), 0.5 + rng.random(ofs.size)
        self.y0 = rng.standard_normal(n)  # what the accumulate form finds in y
        S, Mw = oracle.Stiffness(self.d), oracle.Mass(self.d, self.a2)
        self.refS, self.refMw, self.refM = S.apply(self.x[:n]), Mw.apply(self.x[:n]), oracle.Mass(self.d).apply(self.x[:n])
        self.refA = oracle.helmholtz_apply(self.d, S, Mw, oracle.FaceMass(ofs, self.ax), ofs, OMEGA, self.x)
        for a in (self.x, self.a2, self.ax, self.y0, self.refS, self.refMw, self.refM, self.refA):
            a.setflags(write=False)

    def spaces(self):
        import cuddhelmholtz_amd as cd

        fem = cd.H1Space(self.pm, cd.Basis(self.nb))
        return fem, cd.FaceSpace(fem, self.faces)

    def helmholtz(self, torch, dev):
        import cuddhelmholtz_amd as cd

        fem, fs = self.spaces()
        return cd.HelmholtzOperator(OMEGA, to_dev(torch, self.a2, dev), to_dev(torch, self.ax, dev), fem, fs)


@functools.lru_cache(maxsize=None)
def case(name, nb, faces="all", shifts=None):
    return Case(name, nb, faces, shifts)


@functools.lru_cache(maxsize=None)
def many_slot_dofs(name, nb, pe, fused):
    """(dofs with more than four slots, histogram of slots per border dof) of the layout a plan of this patch size builds"""
    ndof, I, xy, fI, face_elem = space_of(name, nb)
    err, L = build_layout(ndof, nb, I, xy, fI if fused else None, face_elem if fused else None, pe, fused, pe != 16)
    assert err == 0
    slots = np.diff(L["shared_off"])
    return L["shared_dof"][slots > 4], np.bincount(slots).tolist()


def set_knobs(monkeypatch, **knobs):
    for name in ("CUDDH_HELM_PE", "CUDDH_OP_PE", "CUDDH_HELM_LANE", "CUDDH_HELM_NB5_MFMA", "CUDDH_OPERATOR_PLAN", "CUDDH_PLAN_AFFINE", "CUDDH_HELM_PRE",
                 "CUDDH_PLAN_STREAMING", "CUDDH_HELM_MFMA_STAGE", "CUDDH_HELM_PAIR_MASS"):
        monkeypatch.delenv(name, raising=False)
    for name, value in knobs.items():
        monkeypatch.setenv("CUDDH_" + name, str(value))


def check_fused(torch, dev, c, A, dofs=(), what=""):
    """action against the oracle (norm, and pointwise at `dofs`), bitwise on repetition, bitwise through the native ordering;
    returns the result"""
    n = c.n
    x = to_dev(torch, c.x, dev)
    y = torch.full((2 * n,), 123.0, dtype=torch.float64, device=dev)
    A.action(x, y)
    yh = host(y)
    err = rel(yh, c.refA)
    at = np.concatenate([np.asarray(dofs, dtype=np.int64), n + np.asarray(dofs, dtype=np.int64)])
    worst = float(np.abs(yh[at] - c.refA[at]).max() / np.abs(c.refA).max()) if len(at) else 0.0
    print(f"{what}: {A.kernel()} vs oracle {err:.2e}" + (f", at the {len(dofs)} dof(s) with > 4 slots {worst:.2e} of max|ref|" if len(at) else ""))
    assert err < 1e-12 and worst <= 1e-12
    y2 = torch.full_like(y, -7.0)
    A.action(x, y2)
    assert torch.equal(y, y2)
    assert A.has_native()
    z, zy, yn = torch.full_like(y, 7.0), torch.full_like(y, -5.0), torch.zeros_like(y)
    A.to_native(x, z)
    back = torch.zeros_like(x)
    A.from_native(z, back)
    assert torch.equal(back, x)
    A.action_native(z, zy)
    A.from_native(zy, yn)
    assert torch.equal(yn, y)
    return yh


def check_single(torch, dev, c, op, ref, dofs=(), what=""):
    """overwrite form, then y <- y + c Op x over a non-zero y, against the oracle; a plan kernel bitwise on repetition; returns
    the overwrite result"""
    n = c.n
    x = to_dev(torch, c.x[:n], dev)
    y = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
    op.action(x, y)
    yh = host(y)
    coef = -0.75
    ya = to_dev(torch, c.y0, dev).clone()
    op.action(coef, x, ya)
    ref_acc = c.y0 + coef * ref
    errs = rel(yh, ref), rel(host(ya), ref_acc)
    dofs = np.asarray(dofs, dtype=np.int64)
    worst = max(float(np.abs(yh[dofs] - ref[dofs]).max() / np.abs(ref).max()), float(np.abs(host(ya)[dofs] - ref_acc[dofs]).max() / np.abs(ref_acc).max())) if len(dofs) else 0.0
    print(f"{what}: {op.kernel()} vs oracle {errs[0]:.2e} (overwrite) {errs[1]:.2e} (accumulate)" + (f", at the dof(s) with > 4 slots {worst:.2e} of max|ref|" if len(dofs) else ""))
    assert max(errs) < 1e-12 and worst <= 1e-12
    if op.kernel() != "generic":  # the plan kernels sum in a fixed order; the generic ones add with atomics
        y2 = torch.full_like(y, -3.0)
        op.action(x, y2)
        assert torch.equal(y, y2)
    return yh


# ------------------------------------------------------------------ many-slot border sums
def many_slot_cases():
    out = []
    for pe, group in im.MANY_SLOT_MESHES.items():
        for name, count in group:
            out += [(name, count, pe, nb) for nb in {16: (5, 6, 7, 8), 32: (2, 3, 4, 5), 64: (2, 3, 4)}[pe]]
    return out


@pytest.mark.parametrize("name,count,pe,nb", many_slot_cases())
def test_many_slot_border_sums_fused(cuda, monkeypatch, name, count, pe, nb):
    """helm_border_kernel and helm_border_native_kernel past their fourth slot, behind every fused kernel: helm_lane_kernel
    (n_basis 2-4, 64-element patches), helm_patch_kernel (n_basis 2-4 at 32 and 64 elements, n_basis 5 at 32: CUDDH_HELM_PE
    applies to n_basis <= 4) and helm_mfma_kernel (n_basis 5 on request and 6-8, 16-element batches)."""
    import torch

    c = case(name, nb)
    nqS, nqM = nb + 1, 2 + 3 * nb // 2
    if pe == 16:
        forms = {"mfma": (dict(HELM_NB5_MFMA=1), f"helm_mfma_kernel<{nb},{nqS},{nqM}")}
    elif pe == 32:
        forms = {"patch": (dict(HELM_PE=32, HELM_LANE=0), f"helm_patch_kernel<{nb},{nqS},{nqM},NT=0,UG=0,PEK=32")}
    else:
        forms = {"patch": (dict(HELM_PE=64, HELM_LANE=0), f"helm_patch_kernel<{nb},{nqS},{nqM},NT=0,UG=0,PEK=64"),
                 "lane": (dict(HELM_LANE=1), f"helm_lane_kernel<{nb},{nqS},{nqM},NT=0,UG=0> pe=64"),
                 "lane, streaming": (dict(HELM_LANE=1, PLAN_STREAMING=1), f"helm_lane_kernel<{nb},{nqS},{nqM},NT=1,UG=0> pe=64")}
    dofs, hist = many_slot_dofs(name, nb, pe, True)
    print(f"{name} pe {pe} n_basis {nb}: border dofs by number of slots {dict(enumerate(hist))}")
    assert len(hist) - 1 == count >= (6 if pe == 16 else 5) and len(dofs) >= 1
    got = {}
    for form, (knobs, kernel) in forms.items():
        set_knobs(monkeypatch, **knobs)
        A = c.helmholtz(torch, cuda)
        assert A.fused() and A.kernel().startswith(kernel) and A.kernel().endswith(f"pe={pe}" if pe != 16 else "affine=0"), A.kernel()
        got[form] = check_fused(torch, cuda, c, A, dofs, f"{name} n_basis {nb} {form}")
    for form, y in got.items():
        assert rel(y, got[next(iter(got))]) < 1e-13, form


def single_cases():
    out = []
    for pe, group in im.MANY_SLOT_MESHES.items():
        for name, count in group:
            out += [(name, count, pe, nb) for nb in {16: (6, 7, 8), 32: (2, 3, 5), 64: (2, 4, 5)}[pe]]
    return out


@pytest.mark.parametrize("name,count,pe,nb", single_cases())
def test_many_slot_border_sums_single_operators(cuda, monkeypatch, name, count, pe, nb):
    """op_border_kernel past its fourth slot, overwrite and accumulate form (y <- y + c Op x over a non-zero y), behind
    op_patch_kernel (64-element patches, and 32 with CUDDH_OP_PE=32) and op_mfma_kernel (n_basis 6-8): stiffness and weighted
    mass; and against the generic kernels (CUDDH_OPERATOR_PLAN=0) to rounding."""
    import torch

    import cuddhelmholtz_amd as cd

    c = case(name, nb)
    dofs, hist = many_slot_dofs(name, nb, pe, False)
    print(f"{name} pe {pe} n_basis {nb}: border dofs by number of slots {dict(enumerate(hist))}")
    assert len(hist) - 1 == count >= (6 if pe == 16 else 5) and len(dofs) >= 1
    nqS, nqM = nb + 1, 2 + 3 * nb // 2
    if pe == 16:
        kS, kM = f"op_mfma_kernel<{nb},{nqS},0> pe=16 affine=0", f"op_mfma_kernel<{nb},{nqM},1> pe=16 affine=0"
    else:
        kS, kM = f"op_patch_kernel<{nb},{nqS},0,NT=0,UG=0,PEK={pe}> pe={pe}", f"op_patch_kernel<{nb},{nqM},1,NT=0,UG=0,PEK={pe}> pe={pe}"
    got = {}
    for plan in ("1", "0"):
        set_knobs(monkeypatch, OP_PE=pe, OPERATOR_PLAN=plan)
        fem, _ = c.spaces()
        S, M = cd.StiffnessMatrix(fem), cd.MassMatrix(fem, to_dev(torch, c.a2, cuda))
        got[plan] = (check_single(torch, cuda, c, S, c.refS, dofs if plan == "1" else (), f"{name} n_basis {nb} stiffness"),
                     check_single(torch, cuda, c, M, c.refMw, dofs if plan == "1" else (), f"{name} n_basis {nb} weighted mass"))
        assert (S.kernel(), M.kernel()) == ((kS, kM) if plan == "1" else ("generic", "generic")), (S.kernel(), M.kernel())
    for a, b in zip(got["1"], got["0"]):
        assert rel(a, b) < 1e-13


# ------------------------------------------------------------------ valence 3, small rings, subsets of the boundary
@pytest.mark.parametrize("nb", [2, 4, 5, 7])
@pytest.mark.parametrize("name", im.SMALL_MESHES)
def test_small_meshes_and_face_subsets(cuda, monkeypatch, name, nb):
    """A vertex of valence 3, a ring of three elements (every element its own neighbour's neighbour), two boundary loops, a
    domain one element wide, a re-entrant corner; the fused apply with all boundary faces, every other one and, on the rings, the
    inner loop alone.  The default kernel of the order and, for n_basis <= 4, the lane form; the single operators."""
    import torch

    import cuddhelmholtz_amd as cd

    for faces in ("all", "every other") + (("inner loop",) if name.startswith("annulus") else ()):
        c = case(name, nb, faces)
        got = {}
        for form, knobs in (("default", {}),) + ((("lane", dict(HELM_LANE=1)), ("patch 64", dict(HELM_PE=64, HELM_LANE=0))) if nb <= 4 else ()):
            set_knobs(monkeypatch, **knobs)
            A = c.helmholtz(torch, cuda)
            assert A.fused()
            if form == "patch 64":
                assert A.kernel().startswith(f"helm_patch_kernel<{nb},") and A.kernel().endswith("pe=64"), A.kernel()
            got[form] = check_fused(torch, cuda, c, A, what=f"{name} n_basis {nb} faces: {faces} ({len(c.faces)}), {form}")
            y = torch.zeros(2 * c.n, dtype=torch.float64, device=cuda)
            A.action_unfused(to_dev(torch, c.x, cuda), y)
            assert rel(host(y), c.refA) < 1e-12
        for form, y in got.items():
            assert rel(y, got["default"]) < 1e-13, form
    set_knobs(monkeypatch)
    fem, _ = c.spaces()
    S, M = cd.StiffnessMatrix(fem), cd.MassMatrix(fem, to_dev(torch, c.a2, cuda))
    check_single(torch, cuda, c, S, c.refS, what=f"{name} n_basis {nb} stiffness")
    check_single(torch, cuda, c, M, c.refMw, what=f"{name} n_basis {nb} weighted mass")
    assert S.kernel().startswith("op_patch_kernel" if nb <= 5 else "op_mfma_kernel") and M.kernel().startswith("op_patch_kernel" if nb <= 5 else "op_mfma_kernel")


# ------------------------------------------------------------------ colour extremes
@pytest.mark.parametrize("nb", [2, 4, 6])
def test_thirty_one_colours(cuda, monkeypatch, nb):
    """star(31, 1): 31 elements at one vertex.  One element per lane (n_basis <= 5) they share a patch and take the 31 colours a
    plan can have (tests/test_irregular_meshes.py reads the count from the layout); the matrix cores (n_basis 6) see them in
    batches of 16."""
    import torch

    import cuddhelmholtz_amd as cd

    c = case("star(31,1)", nb)
    forms = (("default", {}),) + ((("lane", dict(HELM_LANE=1)), ("patch 64", dict(HELM_PE=64, HELM_LANE=0))) if nb <= 4 else ())
    got = {}
    for form, knobs in forms:
        set_knobs(monkeypatch, **knobs)
        A = c.helmholtz(torch, cuda)
        assert A.fused() and A.bytes_per_apply() > 0
        got[form] = check_fused(torch, cuda, c, A, what=f"star(31,1) n_basis {nb} {form}")
    for form, y in got.items():
        assert rel(y, got["default"]) < 1e-13, form
    set_knobs(monkeypatch)
    fem, _ = c.spaces()
    S, M = cd.StiffnessMatrix(fem), cd.MassMatrix(fem, to_dev(torch, c.a2, cuda))
    check_single(torch, cuda, c, S, c.refS, what=f"star(31,1) n_basis {nb} stiffness")
    check_single(torch, cuda, c, M, c.refMw, what=f"star(31,1) n_basis {nb} weighted mass")
    assert "generic" not in (S.kernel(), M.kernel())


@pytest.mark.parametrize("nb", [2, 4, 5])
def test_refused_plan_falls_back(cuda, monkeypatch, nb):
    """star(33, 1): the patch that holds the centre would need a 32nd colour, plan creation answers hipErrorNotSupported, and
    HelmholtzOperator (action, gmres) and the single operators run the kernels that need no plan."""
    import torch

    import cuddhelmholtz_amd as cd

    set_knobs(monkeypatch)
    c = case("star(33,1)", nb)
    n = c.n
    A = c.helmholtz(torch, cuda)
    assert not A.fused() and A.kernel() == "unfused" and not A.has_native()
    assert A.bytes_per_apply() == 0 and A.bytes_per_apply(actual=True) == 0 and A.bytes_native() == 0 and A.bytes_affine() == 0
    x = to_dev(torch, c.x, cuda)
    y, y2, y3 = (torch.full((2 * n,), v, dtype=torch.float64, device=cuda) for v in (5.0, -5.0, 9.0))
    A.action(x, y)
    A.action_unfused(x, y2)
    e1, e2 = rel(host(y), c.refA), rel(host(y2), c.refA)
    print(f"star(33,1) n_basis {nb}: action without a plan vs oracle {e1:.2e}, action_unfused {e2:.2e}")
    assert e1 < 1e-12 and e2 < 1e-12 and rel(host(y), host(y2)) < 1e-13
    with pytest.raises(RuntimeError):  # no plan, no native ordering: an error, not a crash
        A.to_native(x, y3)
    fem, _ = c.spaces()
    S, M = cd.StiffnessMatrix(fem), cd.MassMatrix(fem, to_dev(torch, c.a2, cuda))
    check_single(torch, cuda, c, S, c.refS, what=f"star(33,1) n_basis {nb} stiffness")
    check_single(torch, cuda, c, M, c.refMw, what=f"star(33,1) n_basis {nb} weighted mass")
    assert (S.kernel(), M.kernel()) == ("generic", "generic")
    # GMRES(10), three cycles: the member (which has no native ordering to iterate in) against the free function on the same system
    b = to_dev(torch, np.random.default_rng(nb).standard_normal(2 * n), cuda)
    x1, x2 = torch.zeros_like(b), torch.zeros_like(b)
    o1 = cd.gmres(2 * n, x1, A, b, 10, 3, 0.0)
    o2 = A.gmres(x2, b, 10, 3, 0.0)
    assert o1.num_matvec == o2.num_matvec > 0
    assert abs(o1.res_norm[-1] - o2.res_norm[-1]) <= 1e-10 * o1.res_norm[0]
    assert rel(host(x2), host(x1)) < 1e-9
    # and the same GMRES on the oracle's operator (as test_ddh_gmres_solve_fp64 compares solves)
    S, Mw, H = oracle.Stiffness(c.d), oracle.Mass(c.d, c.a2), oracle.FaceMass(c.ofs, c.ax)
    xo, info = oracle.gmres(lambda v: oracle.helmholtz_apply(c.d, S, Mw, H, c.ofs, OMEGA, np.ascontiguousarray(v)), host(b), m=10, maxit=3, tol=0.0)
    assert o2.num_matvec == info["num_matvec"] and len(o2.res_norm) == len(info["res_norm"])
    assert abs(o2.res_norm[-1] - info["res_norm"][-1]) <= 1e-10 * info["res_norm"][0]
    assert rel(host(x2), xo) < 1e-8


def test_matrix_core_plan_of_the_refused_star(cuda, monkeypatch):
    """the same star in batches of 16 elements has 16 colours at most: n_basis 6 gets its plan, three patches at the centre"""
    import torch

    set_knobs(monkeypatch)
    c = case("star(33,1)", 6)
    A = c.helmholtz(torch, cuda)
    assert A.fused() and A.kernel().startswith("helm_mfma_kernel<6,")
    check_fused(torch, cuda, c, A, what="star(33,1) n_basis 6")


# ------------------------------------------------------------------ the uniform-metric decision
def uniform_forms():
    n75, n66 = 35, 36
    rng = np.random.default_rng(3)
    mixed = tuple(int(s) for s in rng.integers(0, 4, n75))
    assert len({s % 2 for s in mixed}) == 2  # both orientations occur
    return [("rect(7,5)", None, True), ("rect(7,5)", (1,) * n75, True),  # every element turned: uniform again, G00 and G11 swapped
            ("rect(7,5)", (0,) * (n75 - 1) + (1,), False), ("rect(7,5)", mixed, False),
            ("rect(6,6)", tuple(int(s) for s in rng.integers(0, 4, n66)), True)]  # squares: a turn leaves G as it is


@pytest.mark.parametrize("nb", [2, 4, 6])
@pytest.mark.parametrize("form", range(5))
def test_uniform_metric_decision(cuda, monkeypatch, form, nb):
    """uniform_block() between its extremes: rectangles with hx != hy whose local axes are turned element by element.  A plan
    reads ONE metric block (bytes_affine() > 0) exactly when every element has the same one -- in particular not when only
    the last element differs -- and matches the oracle either way, as do the single operators (whose mass weights are uniform too)."""
    import torch

    import cuddhelmholtz_amd as cd

    name, shifts, uniform = uniform_forms()[form]
    c = case(name, nb, "all", shifts)
    got = {}
    for affine in ("1", "0"):
        set_knobs(monkeypatch, PLAN_AFFINE=affine)
        A = c.helmholtz(torch, cuda)
        assert A.fused() and (A.bytes_affine() > 0) == (uniform and affine == "1"), (A.kernel(), A.bytes_affine())
        what = f"{name} form {form} n_basis {nb} CUDDH_PLAN_AFFINE={affine}"
        yA = check_fused(torch, cuda, c, A, what=what)
        fem, _ = c.spaces()
        S, M = cd.StiffnessMatrix(fem), cd.MassMatrix(fem)
        got[affine] = (yA, check_single(torch, cuda, c, S, c.refS, what=what + " stiffness"), check_single(torch, cuda, c, M, c.refM, what=what + " mass"))
        # (a rectangle's mass weights w_q w_r detJ do not change under a turn: uniform in every form)
        flag = "affine=" if nb == 6 else "UG="
        assert f"{flag}{int(uniform and affine == '1')}" in S.kernel() and f"{flag}{int(affine == '1')}" in M.kernel(), (S.kernel(), M.kernel())
    for a, b in zip(got["1"], got["0"]):
        assert rel(a, b) < 1e-13
