"""DDH kernel 5's element-lane sweep form: lane = one element, one subdomain per 16-lane row, four subdomains
per wavefront, the separable sweep as in-lane FMAs, assembly by DPP row shifts.  The form is forced with
DDH.set_sweep_form(2) / cuddh_hip_ddh_plan_set_sweep_form.

  * parity: a = 1, rhs / action / postprocess at 8 x 8 and 16 x 16 elements (the cases of tests/test_gpu_ddh_mfma_layout.py
    and profiles/tools/kernel5_distances.py) against the fp64 oracle, gated at 2 x the distance the matrix form of the commit
    before had to the same oracle on the same inputs (PARENT5, profiles/r07/kernel5_distances.txt, "this tree"): another
    equally valid summation order of exact fp32 arithmetic can land on either side of the old one, a layout or table bug
    (wrong by O(1)) cannot hide in a factor 2.  Against the matrix form of the same plan the bound is the triangle
    inequality's: 2 x PARENT5 plus the matrix form's own distance;
  * reproducibility: four subdomains share a wavefront, so everything that changes which subdomains sit together, or in
    which row, must change nothing: one full launch, ranges whose lengths are no multiples of 4, a shuffled list cut at an
    odd place, a launch that holds issue priority and a repeated run give bitwise the same traces, with and without x; the
    y contributions of subdomains that share no dof are bitwise the same from one listed launch and from one launch each;
  * copies of shared nodes: a node that 2 or 4 elements of a subdomain share is held by as many (lane, register) pairs, and one
    of them publishes it.  The comparisons above keep that owner fixed and the fp64 gates are far too wide to see one fp32
    rounding, so form 3 turns the owner rule round (the copy with the largest element-node index publishes, not the smallest):
    traces and y contributions are bitwise those of form 2, i.e. the published result does not depend on the owning copy;
  * refusal and fallback: tables handed to cuddh_hip_ddh_plan_create directly (nothing is launched on them but the plan's
    checks): a metric that is not separable, and a separable one whose node weights differ between the two sides of a shared
    edge, stay on the matrix form under auto and refuse form 2 with hipErrorInvalidValue; a qualifying table takes it.  Form 2
    on an n_basis 8 plan, an fp64 plan and a plan on another kernel is refused;
  * auto: plans with at least AUTO_MIN_DOMAINS subdomains on rectangles take the element-lane form, smaller ones the matrix
    form, and info()["kernel"] stays 5 either way.
Every distance is printed (`pytest -s`).
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_ddh_mfma_layout as L
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu

# distance of the parent commit's kernel 5 (matrix form) to the fp64 oracle on L.case(nx): nx -> (rhs, action, postprocess)
PARENT5 = {8: (1.14e-06, 4.1e-07, 1.00e-06), 16: (7.6e-07, 4.9e-07, 1.09e-06)}
AUTO_MIN_DOMAINS = 8192  # ELEMENT_LANE_MIN_DOMAINS of csrc/src/ddh_resolve.cpp
HIP_ERROR_INVALID_VALUE = 1


def make(cd, nx, form, precision="f32", kernel=0, nb=4, ny=None):
    """DDH on nx x ny (default nx) elements (subdomains of 16 / nb elements per side), a = 1, L.case's frequency; form: forced, or None"""
    import math

    omega = 2 * math.pi * nx / 10
    ny = nx if ny is None else ny
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, ny, -1.0, 1.0), cd.Basis(nb))
    F = cd.DDH(omega, np.ones(fem.size()), fem, nx, ny, precision=precision, kernel=kernel)
    if form is not None:
        F.set_sweep_form(form)
    return F, fem


def outputs(torch, cuda, F, c):
    _, d, _, fh, _, lam_h, written = c
    f = to_dev(torch, fh, cuda)
    lam = to_dev(torch, lam_h.astype(np.float32), cuda)
    b = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
    F.rhs(f, b)
    y = torch.zeros_like(b)
    F.action(lam, y)
    u = torch.zeros(2 * d.ndof, dtype=torch.float64, device=cuda)
    F.postprocess(lam, f, u)
    return b.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)[written], u.cpu().numpy()


@pytest.mark.parametrize("nx", [8, 16])
def test_element_lane_vs_fp64_oracle_and_matrix_form(cuda, nx):
    import torch

    import cuddhelmholtz_amd as cd

    c = L.case(nx)
    ref = L.oracle_outputs(c)
    F, _ = make(cd, nx, 2)
    assert F.info()["kernel"] == 5 and F.sweep_form() == 2
    out2 = outputs(torch, cuda, F, c)
    F.set_sweep_form(1)
    assert F.info()["kernel"] == 5 and F.sweep_form() == 1
    out1 = outputs(torch, cuda, F, c)
    names = ("rhs", "action", "postprocess")
    e2 = tuple(rel(a, r) for a, r in zip(out2, ref))
    e1 = tuple(rel(a, r) for a, r in zip(out1, ref))
    e21 = tuple(float(np.linalg.norm(a - b) / np.linalg.norm(r)) for a, b, r in zip(out2, out1, ref))
    for i, nm in enumerate(names):
        print(f"[{nx}x{nx}, a=1] {nm}: element-lane form vs fp64 oracle {e2[i]:.4e} (parent's kernel 5 {PARENT5[nx][i]:.3e}, gate 2 x), "
              f"matrix form vs oracle {e1[i]:.4e}, element-lane vs matrix form {e21[i]:.4e}")
    for i, nm in enumerate(names):
        assert e2[i] < 2 * PARENT5[nx][i], (nm, e2[i], PARENT5[nx][i])
        assert e21[i] < 2 * PARENT5[nx][i] + e1[i], (nm, e21[i], e1[i])


def test_launch_partitions_are_bitwise_the_full_launch(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 32  # 8 x 8 subdomains
    c = L.case(nx)
    F, fem = make(cd, nx, 2)
    nd, ndx = F.info()["n_domains"], nx // 4
    assert nd == 64 and F.sweep_form() == 2
    f = to_dev(torch, c[3], cuda)
    lam = to_dev(torch, c[5].astype(np.float32), cuda)
    perm = np.random.default_rng(3).permutation(nd).astype(np.int32)
    cut = (nd // 3) | 1
    assert cut % 4 and (nd - cut) % 4
    for x, l in ((f, None), (None, lam), (f, lam)):  # sources only, traces only (the form without x), both
        plain = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
        F.local_traces(0, nd, x, l, plain)
        assert plain.abs().max().item() > 0
        again = torch.zeros_like(plain)
        F.local_traces(0, nd, x, l, again)
        assert torch.equal(again, plain)
        ranged = torch.zeros_like(plain)
        for d0, d1 in ((0, 13), (13, 14), (14, 27), (27, 29), (29, nd)):  # lengths 13, 1, 13, 2, nd - 29: every tail shape
            F.local_traces(d0, d1, x, l, ranged)
        assert torch.equal(ranged, plain)
        listed = torch.zeros_like(plain)
        for ids in (perm[:cut], perm[cut:]):
            F.local_traces_listed(to_dev(torch, ids, cuda), x, l, listed)
        assert torch.equal(listed, plain)
        F.set_wave_priority(True)
        held = torch.zeros_like(plain)
        F.local_traces(0, nd // 2 - 1, x, l, held)
        F.local_traces_listed(to_dev(torch, np.arange(nd // 2 - 1, nd, dtype=np.int32), cuda), x, l, held)
        F.set_wave_priority(False)
        assert torch.equal(held, plain)

    # y contributions: subdomains that share no dof (every other one in both directions), so that every entry of u gets one
    # add and the atomics' order cannot matter.  One shuffled listed launch against one launch per subdomain.
    info = F.info()
    gI = F.table("gI").reshape(nd, info["mx_dof"])
    apart = np.array([s for s in range(nd) if (s % ndx) % 2 == 0 and (s // ndx) % 2 == 0], dtype=np.int32)
    apart = np.random.default_rng(5).permutation(apart)[:-1].astype(np.int32)
    assert apart.size % 4 and apart.size >= 8
    touched = np.concatenate([gI[s] for s in apart])
    assert touched.min() >= 0 and np.unique(touched).size == touched.size  # disjoint dof sets
    n = fem.size()
    for x in (f, None):
        together = torch.zeros(2 * n, dtype=torch.float64, device=cuda)
        F.local_solution_listed(to_dev(torch, apart, cuda), lam, x, together, True)
        assert together.abs().max().item() > 0
        single = torch.zeros_like(together)
        for s in apart:
            F.local_solution(int(s), int(s) + 1, lam, x, single, False)
        assert torch.equal(single, together)
        ranged = torch.zeros_like(together)
        for s in np.sort(apart):
            F.local_solution_listed(to_dev(torch, np.array([s], dtype=np.int32), cuda), lam, x, ranged, False)
        assert torch.equal(ranged, together)


def test_published_result_does_not_depend_on_the_owning_copy(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 32  # 8 x 8 subdomains
    c = L.case(nx)
    F, fem = make(cd, nx, 2)
    nd, ndx = F.info()["n_domains"], nx // 4
    assert nd == 64
    f = to_dev(torch, c[3], cuda)
    lam = to_dev(torch, c[5].astype(np.float32), cuda)
    # as above: subdomains that share no dof, so that every entry of u gets one add; all 16 of them, 15 x 15 dofs each that
    # no other subdomain of the set touches (the 3 x 3 four-copy corners and the 24 two-copy edges' nodes among them)
    apart = np.array([s for s in range(nd) if (s % ndx) % 2 == 0 and (s // ndx) % 2 == 0], dtype=np.int32)
    n = fem.size()

    def published(form):
        F.set_sweep_form(form)
        assert F.sweep_form() == form and F.info()["kernel"] == 5
        out = []
        for x, l in ((f, None), (None, lam), (f, lam)):
            t = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
            F.local_traces(0, nd, x, l, t)
            assert t.abs().max().item() > 0
            out.append(t)
        for x in (f, None):
            u = torch.zeros(2 * n, dtype=torch.float64, device=cuda)
            F.local_solution_listed(to_dev(torch, apart, cuda), lam, x, u, True)
            assert u.abs().max().item() > 0
            out.append(u)
        return out

    first, last = published(2), published(3)
    for a, b in zip(first, last):
        assert torch.equal(a, b)
    F.set_sweep_form(0)
    assert F.sweep_form() == 1  # 64 subdomains: auto never takes form 3, and is below the threshold of form 2


def _plan_form(torch, cuda, G_el, is_f64=False, kernel=0):
    """one 4 x 4-element subdomain with the boundary dofs numbered first and element metric G_el (16 nodes x 3), handed to
    cuddh_hip_ddh_plan_create: (create's error, kernel, form under auto, error of set_sweep_form(2), form after it)"""
    from cuddhelmholtz_amd import _native as N

    side, nbnd = 13, 48
    X, Y = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    on_bnd = (X == 0) | (X == side - 1) | (Y == 0) | (Y == side - 1)
    numbering = np.empty((side, side), dtype=np.int32)
    numbering[on_bnd] = np.arange(nbnd, dtype=np.int32)
    numbering[~on_bnd] = np.arange(nbnd, side * side, dtype=np.int32)
    sI = np.empty(256, dtype=np.int32)
    for el in range(16):
        for l in range(4):
            for k in range(4):
                sI[k + 4 * (l + 4 * el)] = numbering[3 * (el % 4) + k, 3 * (el // 4) + l]
    real = np.float64 if is_f64 else np.float32
    Dm = np.random.default_rng(1).standard_normal(16)
    keep = [to_dev(torch, a, cuda) for a in (np.array([side * side], np.int32), np.array([nbnd], np.int32), sI, Dm.astype(real),
                                             np.tile(np.asarray(G_el, dtype=np.float64).reshape(48), 16).astype(real))]
    desc = N.DdhDesc(g_ndof=side * side, n_domains=1, n_lambda=nbnd, nb=4, nel1d=4, mx_dof=side * side, mx_fdof=nbnd, nt=1, omega=1.0,
                     dt=1.0, s_dof=keep[0].data_ptr(), s_fdof=keep[1].data_ptr(), sI=keep[2].data_ptr(), D=keep[3].data_ptr(),
                     G=keep[4].data_ptr())
    plan = C.c_void_p()
    err = N.lib.cuddh_hip_ddh_plan_create(C.byref(plan), C.byref(desc), int(is_f64), kernel)
    if err:
        return err, None, None, None, None
    picked = N.lib.cuddh_hip_ddh_plan_kernel(plan)
    auto = N.lib.cuddh_hip_ddh_plan_sweep_form(plan)
    err2 = N.lib.cuddh_hip_ddh_plan_set_sweep_form(plan, 2)
    after = N.lib.cuddh_hip_ddh_plan_sweep_form(plan)
    assert N.lib.cuddh_hip_ddh_plan_set_sweep_form(plan, 1) == 0 and N.lib.cuddh_hip_ddh_plan_set_sweep_form(plan, 0) == 0
    assert N.lib.cuddh_hip_ddh_plan_set_sweep_form(plan, 3) == err2  # the same form, the other copy publishing: refused alike
    assert N.lib.cuddh_hip_ddh_plan_set_sweep_form(plan, 0) == 0
    assert N.lib.cuddh_hip_ddh_plan_set_sweep_form(plan, 4) == HIP_ERROR_INVALID_VALUE
    assert N.lib.cuddh_hip_ddh_plan_set_sweep_form(plan, -1) == HIP_ERROR_INVALID_VALUE
    assert N.lib.cuddh_hip_ddh_plan_sweep_form(plan) == auto
    N.lib.cuddh_hip_ddh_plan_destroy(plan)
    torch.cuda.synchronize()
    return err, picked, auto, err2, after


def _separable_metric(alpha, beta, gamma, delta):
    G = np.zeros((4, 4, 3))  # [l][k][component], node k + 4 l
    for l in range(4):
        for k in range(4):
            G[l, k] = (alpha[k] * beta[l], 0.0, gamma[k] * delta[l])
    return G.reshape(16, 3)


def test_refusal_and_fallback_on_handmade_tables(cuda):
    import torch

    w = np.array([1.0, 5.0, 5.0, 1.0]) / 6.0  # symmetric 1-D weights, as a quadrature rule's
    # rectangles: gx = (hy / hx) w_k w_l, gz = (hx / hy) w_k w_l: qualifies; one subdomain is below the auto threshold
    good = _separable_metric(0.7 * w, w, w, 1.3 * w)
    assert _plan_form(torch, cuda, good) == (0, 5, 1, 0, 2)
    # a full random metric (gy != 0, no product form): kernel 5 is built, the element-lane form is not
    rng = np.random.default_rng(1)
    assert _plan_form(torch, cuda, rng.standard_normal((16, 3))) == (0, 5, 1, HIP_ERROR_INVALID_VALUE, 1)
    # diagonal but no product of 1-D factors
    bent = good.copy()
    bent[5, 0] *= 1.01
    assert _plan_form(torch, cuda, bent) == (0, 5, 1, HIP_ERROR_INVALID_VALUE, 1)
    # separable, but the weight differs between the two sides of a shared edge: gamma_3 != gamma_0, then beta_3 != beta_0
    skew = np.array([1.0, 5.0, 5.0, 1.1]) / 6.0
    assert _plan_form(torch, cuda, _separable_metric(0.7 * w, w, skew, 1.3 * w)) == (0, 5, 1, HIP_ERROR_INVALID_VALUE, 1)
    assert _plan_form(torch, cuda, _separable_metric(0.7 * w, skew, w, 1.3 * w)) == (0, 5, 1, HIP_ERROR_INVALID_VALUE, 1)
    # a weight that is not positive
    assert _plan_form(torch, cuda, _separable_metric(0.7 * w, w, np.array([1.0, -5.0, -5.0, 1.0]), 1.3 * w))[3] == HIP_ERROR_INVALID_VALUE
    # other kernels and fp64 on the qualifying table
    assert _plan_form(torch, cuda, good, kernel=3) == (0, 3, 0, HIP_ERROR_INVALID_VALUE, 0)
    assert _plan_form(torch, cuda, good, is_f64=True, kernel=8) == (0, 8, 0, HIP_ERROR_INVALID_VALUE, 0)
    assert _plan_form(torch, cuda, good, is_f64=True) == (0, 3, 0, HIP_ERROR_INVALID_VALUE, 0)


def test_form_2_is_refused_on_plans_that_are_not_kernel_5(cuda):
    import cuddhelmholtz_amd as cd

    for kwargs in ({"nb": 8}, {"precision": "f64"}, {"precision": "f64", "kernel": 8}, {"kernel": 3}):
        F, _ = make(cd, 8, None, **kwargs)
        kernel = F.info()["kernel"]
        assert kernel != 5 and F.sweep_form() == 0
        for form in (2, 3):
            with pytest.raises(RuntimeError):
                F.set_sweep_form(form)
        F.set_sweep_form(1)
        F.set_sweep_form(0)
        assert F.info()["kernel"] == kernel and F.sweep_form() == 0


def test_auto_takes_the_element_lane_form_from_the_threshold_on(cuda):
    import cuddhelmholtz_amd as cd

    # 64 x 64 subdomains, half the threshold, and 64 x 128 subdomains (rectangular elements), the threshold itself
    for (nx, ny), form in (((256, 256), 1), ((256, 512), 2)):
        F, _ = make(cd, nx, None, ny=ny)
        nd = F.info()["n_domains"]
        assert nd == (nx // 4) * (ny // 4) and (nd >= AUTO_MIN_DOMAINS) == (form == 2) and F.info()["kernel"] == 5
        assert F.sweep_form() == form
        F.set_sweep_form(3 - form)
        assert F.sweep_form() == 3 - form and F.info()["kernel"] == 5
        F.set_sweep_form(0)
        assert F.sweep_form() == form
