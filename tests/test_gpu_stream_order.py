"""Stream order: every entry point on a non-blocking side stream, against the same calls on the null stream.

The rest of the GPU suite runs on the null stream, where everything is ordered against everything else: a launch that goes to
nullptr instead of cuddh::stream(), a blocking hipMemcpy that reads an array a set-up kernel is still writing on stream(), a
hipMemset on the wrong stream all behave there.  Production does not run there ("Stream contract": bench.py and
dist.py run the boundary subdomains on a torch side stream, the multi-GPU host one stream per device, gmres() queues its operator
one step ahead of the host).  Here the library launches on a torch side stream, which is created non-blocking, so nothing on the
null stream waits for it.

Delayed inputs.  Every floating-point device input of a call under test (x, f, lam, b, z_in, the coefficients a, a2x, ax handed
to constructors, and the targets of accumulating calls) is a buffer that holds NaN, synchronised, when the call is issued; the
side stream is first given a busy kernel of DELAY_MS, then the copies of the real values into those buffers, then the library
call.  A stray null-stream launch or an unsynchronised host read sees NaN, zeros or the sentinel the outputs start as.  Integer
and index arrays (subdomain ids, labels, faces, halo ids) are never delayed: a stale index could address out of bounds, and
this module must only ever be able to produce wrong numbers.  Every tensor is allocated under the default stream before the
calls and lives until the final torch.cuda.synchronize(), so the caching allocator never hands a block from one stream to
another.  No two library calls run concurrently on two streams: the reduction workspace is shared by design.

The canary (the module fixture, before any test) proves that the set-up can see a defect at all: with the library pointed at
the NULL stream and the inputs delayed on the side stream, one StiffnessMatrix.action must NOT reproduce the reference.  If it
does, the side stream is not independent of the null stream (they share a hardware queue, say) and every test below would
pass vacuously; a stream from hipStreamCreateWithFlags(hipStreamNonBlocking) is tried once instead, and if the canary still
computes the right answer the module fails with that message.

Reference: the identical call sequence on the null stream in the same process (the rest of the suite holds those results to
the oracles).  Bitwise (torch.equal) wherever the suite asserts bitwise repeatability: plan kernels, the fused apply, DDH
traces and solution, WaveHoltz periods, GMRES with a handle operator, the BLAS-1 / Gram-Schmidt / box / halo kernels.
Relative l2 < 1e-13, the suite's gate "between two forms", where atomics leave the summation order free: the generic
element_ops.hip kernels (CUDDH_OPERATOR_PLAN=0, the face mass, the unfused Helmholtz apply), linear_functional,
face_linear_functional and FaceSpace.prolong.

Calls that only queue work (applies of operators whose plan exists, the native ordering, the partial DDH launches, a WaveHoltz
period, action and solution, the three reductions) are issued together behind one delay, and after the last of them the side
stream must still be busy (Run.late): a call that synchronised on the way would have let the calls behind it read inputs that
had arrived.  A call that may synchronise the stream (a constructor, the first apply of an operator that builds its plan, the
first FaceSpace.restrict, which uploads the projection, a functional, GMRES) has a delay of its own.  A fresh DDH builds its
plan in its first call (geometric factors, uploads, device checks, table builders, time grids), so that call is issued behind
the delay with f or lam late and no setter is called before it; the constructors of WaveHoltz and WaveHoltzBox take host data
and get a bare delay in front that is asserted to outlast the whole constructor as timed on the null stream, so that their
set-up kernels are late; the overwrite forms of nodal_values and the functionals, which read no vector, get a bare delay too.  DDH plans run at one element per wavelength: a short
period, the same kernels and branches.

The delay.  Measured on an MI355X with events on the null stream (test_report_the_longest_call prints the figures on every
run): the longest single library call behind a delay is the first rhs() of a WaveHoltz on the holed mesh, 9.73 ms (10.23 and
10.72 ms in two further runs); the first
call of a fresh label-built DDH, which creates the plan, takes 9.17 ms, its later calls 8.4 to 8.6 ms.  DELAY_MS = 60 is
more than five times the longest call and above the 20 ms floor; a case whose longest call on the null stream exceeds a quarter of the
delay says so in its output (not an assertion: one nodal_values, otherwise under 9 ms, measured 144 ms once on a shared machine).  The busy kernel is timed with events when the module starts, stretched to 1.1 DELAY_MS, and
its measured length is asserted to be at least DELAY_MS.  Canary on that machine: all 961 entries NaN with the library on the
null stream, on a plain torch.cuda.Stream().
"""
import ctypes as C
import functools
import math
import time

import numpy as np
import pytest

from conftest import load_unstructured_square

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DELAY_MS = 60.0
SENTINEL = -777.0
CONSTRUCTOR_DELAYS = 8  # a WaveHoltz constructor works on the host before its set-up kernels: a bare delay longer than the whole constructor
LOOSE = 1e-13  # the suite's gate between two forms of one operator; used where atomics order the sums
_S = {}  # the module's stream, delay and timings: set by the fixture
_TIMES = {}  # label -> ms of one library call on the null stream
_CONSTRUCTOR_MS = {}  # case -> wall ms of a WaveHoltz constructor on the null stream


# ================================================================== harness
def _events_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _calibrated_delay(torch, dev):
    """A callable that keeps the current stream busy for at least DELAY_MS, and the length it measured for it.  torch.cuda._sleep
    counts clock ticks whose rate differs between devices, so it is timed first; without it, a chain of in-place passes over a
    large tensor does the same."""
    if hasattr(torch.cuda, "_sleep"):
        probe = 2_000_000
        torch.cuda._sleep(probe)
        torch.cuda.synchronize()
        per_ms = probe / max(_events_ms(torch, lambda: torch.cuda._sleep(probe)), 1e-3)
        ticks = int(1.1 * DELAY_MS * per_ms)
        delay = lambda: torch.cuda._sleep(ticks)  # noqa: E731
        ms = _events_ms(torch, delay)
        if ms >= DELAY_MS:
            return delay, ms, f"torch.cuda._sleep({ticks})"
    big = torch.ones(1 << 26, dtype=torch.float32, device=dev)
    one = max(_events_ms(torch, lambda: big.mul_(1.0)), _events_ms(torch, lambda: big.mul_(1.0)), 1e-3)
    reps = int(math.ceil(1.2 * DELAY_MS / one))

    def delay():
        for _ in range(reps):
            big.mul_(1.0)

    return delay, _events_ms(torch, delay), f"{reps} in-place passes over 256 MiB"


def _external_stream(torch):
    """a stream from hipStreamCreateWithFlags(hipStreamNonBlocking), as torch sees it"""
    hip = C.CDLL("libamdhip64.so")
    handle = C.c_void_p()
    rc = hip.hipStreamCreateWithFlags(C.byref(handle), C.c_uint(1))  # hipStreamNonBlocking
    assert rc == 0 and handle.value, f"hipStreamCreateWithFlags failed: {rc}"
    return torch.cuda.ExternalStream(handle.value)


class Run:
    """One pass over a case: side None runs it on the null stream (the reference), a stream runs it there with every armed
    input delayed.  Buffers are declared before `with run:` (default stream); inside, the library launches on the run's stream;
    leaving synchronises the device and points the library back at torch's default stream."""

    def __init__(self, side, tag=""):
        import torch

        import cuddhelmholtz_amd as cd

        self.torch, self.cd, self.side, self.dev = torch, cd, side, torch.device("cuda:0")
        self.staged, self.buf, self.compared, self.values, self.loose = {}, {}, [], {}, set()
        self._ctx, self.tag, self.problems, self.times = None, tag, [], {}

    # ---- buffers (before `with`)
    def floats(self, dtype=None, **host):
        """delayed inputs: name -> host values; the device buffer holds NaN until arm() delivers them"""
        for name, a in host.items():
            t = self.torch.from_numpy(np.ascontiguousarray(a))
            if dtype is not None:
                t = t.to(dtype)
            self.staged[name] = t.to(self.dev)
            self.buf[name] = self.torch.full_like(self.staged[name], float("nan"))
        return [self.buf[n] for n in host] if len(host) > 1 else self.buf[next(iter(host))]

    def outs(self, dtype=None, **sizes):
        """outputs: name -> length; they start as the sentinel and are compared between the two passes"""
        dtype = dtype or self.torch.float64
        for name, n in sizes.items():
            self.buf[name] = self.torch.full((int(n),), SENTINEL, dtype=dtype, device=self.dev)
            self.compared.append(name)
        return [self.buf[n] for n in sizes] if len(sizes) > 1 else self.buf[next(iter(sizes))]

    def ints(self, a):
        """an index array: on the device and complete before anything runs, never delayed"""
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.dev)

    def compare(self, *names):
        """inputs a call updates in place are results too"""
        self.compared += names

    # ---- inside `with`
    def __enter__(self):
        self.torch.cuda.synchronize()
        if self.side is not None:
            self._ctx = self.torch.cuda.stream(self.side)
            self._ctx.__enter__()
        self.cd.use_torch_stream()
        return self

    def __exit__(self, *exc):
        try:
            self.torch.cuda.synchronize()
        finally:
            if self._ctx is not None:
                self._ctx.__exit__(*exc)
                self._ctx = None
            self.cd.use_torch_stream()  # torch's default stream again, whatever happened
        return False

    def arm(self, *names, times=1):
        """Deliver the real values of these inputs behind the delay: NaN everywhere and synchronised, then, on the run's stream, the
        busy kernel (`times` of them) and the copies.  On the null stream the copies alone.  Without names: a bare delay, which makes
        the set-up kernels of a constructor that takes host data late."""
        for n in names:
            self.buf[n].fill_(float("nan"))
        if self.side is not None:
            self.side.synchronize()
            for _ in range(times):
                _S["delay"]()
        for n in names:
            self.buf[n].copy_(self.staged[n], non_blocking=True)

    def call(self, label, fn, *args, **kw):
        """one library call behind armed inputs; on the null stream its length goes into _TIMES"""
        if self.side is not None:
            return fn(*args, **kw)
        out = []
        self.times[label] = _TIMES[f"{label} [{self.tag}]"] = _events_ms(self.torch, lambda: out.append(fn(*args, **kw)))
        return out[0]

    def late(self, what):
        """After the last call of a group issued behind one delay: the side stream must still be busy.  A call that synchronised the
        stream on the way would have let every call behind it read inputs that had arrived."""
        if self.side is not None and self.side.query():
            self.problems.append(f"{what}: the side stream was idle after the group, so a call in it synchronised and the calls behind it were not late")

    def results(self):
        return {n: self.buf[n] for n in self.compared}, dict(self.values), set(self.loose), list(self.problems), dict(self.times)


def both(case, *args, loose=(), **kw):
    """the case on the null stream, then on the side stream: every compared buffer bitwise equal (relative l2 < LOOSE for the
    names in `loose`), every recorded value equal"""
    import torch

    tag = " ".join(str(a) for a in args)
    ref, ref_values, ref_loose, _, times = case(Run(None, tag), *args, **kw)
    got, got_values, got_loose, wrong, _ = case(Run(_S["side"], tag), *args, **kw)
    assert ref.keys() == got.keys() and ref_values.keys() == got_values.keys() and ref_loose == got_loose
    loose = set(loose) | ref_loose  # (a case adds the results of an operator that reports the generic kernel)
    # The rule "the delay is four times the longest call" sizes DELAY_MS from the figures in the module docstring; it is printed, not
    # asserted: on a shared machine one call in a few hundred stalls on the host (a nodal_values that otherwise stays under 9 ms measured 144 ms once),
    # and such a stall must not fail the suite.  A stalled call is merely not late in that pass.
    slow = max(times, key=times.get) if times else None  # (the C ABI cases call the entry points themselves: launches only)
    if slow and 4 * times[slow] > _S["delay_ms"]:
        print(f"stream order: [{tag}] the delay of {_S['delay_ms']:.1f} ms is less than four times the {times[slow]:.2f} ms of {slow} on the null stream")
    for name, r in ref.items():
        g = got[name]
        if not bool(torch.isfinite(r).all()):
            wrong.append(f"{name}: the null-stream reference is not finite")
        elif bool((r == SENTINEL).all()):
            wrong.append(f"{name}: the null-stream reference was never written")
        elif name in loose:
            err = float(torch.linalg.norm((g - r).double()) / torch.linalg.norm(r.double()))
            if not err < LOOSE:
                wrong.append(f"{name}: side stream differs from the null stream by {err:.3e} relative l2, {int(torch.isnan(g).sum())} entries NaN")
        elif not torch.equal(g, r):
            err = float(torch.linalg.norm((g - r).double()) / torch.linalg.norm(r.double()))
            wrong.append(f"{name}: {int((g != r).sum())} of {r.numel()} entries differ from the null-stream run ({err:.3e} relative l2), "
                         f"{int(torch.isnan(g).sum())} are NaN")
    for name, v in ref_values.items():
        if got_values[name] != v:
            wrong.append(f"{name}: {got_values[name]!r} on the side stream, {v!r} on the null stream")
    assert not wrong, "\n".join(wrong)
    assert not loose - set(ref), f"loose names that no result has: {loose - set(ref)}"


def _canary(torch, cd, side):
    """True if delayed inputs are seen as NaN by work on the null stream: the condition under which this module can fail"""
    from cuddhelmholtz_amd import _native as N

    fem = cd.H1Space(cd.Mesh2D.uniform_rect(10, -1.0, 1.0, 10, -1.0, 1.0), cd.Basis(4))
    n = fem.size()
    xh = np.random.default_rng(1).standard_normal(n)
    ref_run = Run(None)
    x, y = ref_run.floats(x=xh), ref_run.outs(y=n)
    S = cd.StiffnessMatrix(fem)
    with ref_run:
        ref_run.arm("x")
        S.action(x, y)
    run = Run(side)
    x2, y2 = run.floats(x=xh), run.outs(y=n)
    with run:
        N.lib.cuddh_set_stream(None)  # the defect, on purpose: the library launches on the null stream
        run.arm("x")
        S.action(x2, y2)
    assert bool(torch.isfinite(y).all())
    return not torch.equal(y, y2), int(torch.isnan(y2).sum()), n


@pytest.fixture(scope="module", autouse=True)
def side_stream(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    try:
        _S["delay"], _S["delay_ms"], how = _calibrated_delay(torch, cuda)
        assert _S["delay_ms"] >= DELAY_MS >= 20.0, f"the delay runs {_S['delay_ms']:.1f} ms, not {DELAY_MS} ms"
        side = torch.cuda.Stream()
        seen, nans, n = _canary(torch, cd, side)
        _S["canary"] = f"torch.cuda.Stream(): {nans} of {n} entries NaN"
        if not seen:
            side = _external_stream(torch)
            seen, nans, n = _canary(torch, cd, side)
            _S["canary"] += f"; hipStreamNonBlocking stream: {nans} of {n} entries NaN"
        print(f"stream order: delay {_S['delay_ms']:.1f} ms ({how}); canary on the null stream: {_S['canary']}")
        assert seen, ("the canary computed the right answer from delayed inputs with the library on the null stream: the side stream "
                      f"is not independent of the null stream and this module would prove nothing ({_S['canary']})")
        _S["side"] = side
        yield side
        torch.cuda.synchronize()
    finally:
        cd.use_torch_stream()  # outside any stream context: the rest of the suite runs on torch's default stream


# ================================================================== operators
def _mesh(kind, nx=10):
    import cuddhelmholtz_amd as cd

    if kind == "structured":
        return cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0)
    return cd.Mesh2D.from_vertices(*load_unstructured_square())


def _spaces(kind, nx, nb):
    import cuddhelmholtz_amd as cd

    mesh = _mesh(kind, nx)
    fem = cd.H1Space(mesh, cd.Basis(nb))
    return fem, cd.FaceSpace(fem, mesh.boundary_edges())


def operators_case(r, kind, nx, nb, plan):
    cd = r.cd
    fem0, fs0 = _spaces(kind, nx, nb)
    n, nf = fem0.size(), fs0.size()
    rng = np.random.default_rng(7 * nb + nx)
    x, a, g, g2 = r.floats(x=rng.standard_normal(n), a=0.5 + rng.random(n), g=rng.standard_normal(n), g2=rng.standard_normal(n))
    xf, af = r.floats(xf=rng.standard_normal(nf), af=0.5 + rng.random(nf))
    accs = r.floats(**{f"acc{k}": rng.standard_normal(n) for k in "SMD"})
    faccs = r.floats(**{f"acc{k}": rng.standard_normal(nf) for k in "HE"})
    Facc, FFacc = r.floats(Facc=rng.standard_normal(n)), r.floats(FFacc=rng.standard_normal(nf))
    yS, yM, yD, nv, F1, F2 = r.outs(yS=n, yM=n, yD=n, nv=n, F1=n, F2=n)
    yH, yE, rF, FF = r.outs(yH=nf, yE=nf, rF=nf, FF=nf)
    r.compare("accS", "accM", "accD", "accH", "accE", "g", "g2", "Facc", "FFacc")
    with r:
        fem, fs = _spaces(kind, nx, nb)  # fresh: their device arrays are uploaded on the run's stream
        S = cd.StiffnessMatrix(fem)
        ops = {}
        for name, cls, space, coef in (("MassMatrix", cd.MassMatrix, fem, "a"), ("DiagInvMassMatrix", cd.DiagInvMassMatrix, fem, "a"),
                                       ("FaceMassMatrix", cd.FaceMassMatrix, fs, "af"), ("DiagInvFaceMassMatrix", cd.DiagInvFaceMassMatrix, fs, "af")):
            r.arm(coef)
            ops[name] = r.call(f"{name}(a)", cls, space, r.buf[coef])  # the constructor reads the delayed device coefficient
        M, D, H, E = ops.values()
        # the first apply of an operator with a plan builds it, and that synchronises: a delay each
        r.arm("x")
        r.call("StiffnessMatrix.action, first", S.action, x, yS)
        r.arm("x")
        r.call("MassMatrix.action, first", M.action, x, yM)
        r.arm("xf")
        r.call("FaceMassMatrix.action, first", H.action, xf, yH)
        r.arm("x")
        r.call("FaceSpace.restrict, first", fs.restrict, x, rF)  # uploads the projection on the way, which synchronises
        # what only queues work: one delay in front of all of it
        r.arm("x", "xf", "g", "g2", "accS", "accM", "accD", "accH", "accE")
        r.call("DiagInvMassMatrix.action", D.action, x, yD)
        r.call("DiagInvFaceMassMatrix.action", E.action, xf, yE)
        r.call("FaceSpace.restrict", fs.restrict, x, rF)
        r.call("FaceSpace.prolong", fs.prolong, xf, g)
        r.call("FaceSpace.orth", fs.orth, g2)
        for op, xin, acc, c in ((S, x, accs[0], 0.5), (M, x, accs[1], 0.25), (D, x, accs[2], 0.25), (H, xf, faccs[0], 0.25), (E, xf, faccs[1], 0.25)):
            r.call(f"{type(op).__name__}.action, accumulate", op.action, c, xin, acc)
        r.late("DiagInv applies, restrict, prolong, orth and the five accumulate applies")
        # the functionals synchronise when they are done: a delay in front of each that reads its target
        # the overwrite forms read no vector: a bare delay makes their own uploads, zero fills and kernels late
        r.arm()
        r.call("nodal_values", cd.nodal_values, fem, cd.MASS_POLY, nv)
        r.arm()
        r.call("linear_functional", cd.linear_functional, fem, cd.GAUSSIANS, F1, param=7.0)
        r.arm()
        r.call("linear_functional nq", cd.linear_functional, fem, cd.GAUSSIANS, F2, param=7.0, nq=nb + 3)
        r.arm("Facc")
        r.call("linear_functional, accumulate", cd.linear_functional, fem, cd.MASS_POLY, Facc, c=0.5, accumulate=True)
        r.arm()
        r.call("face_linear_functional", cd.face_linear_functional, fs, cd.MASS_POLY, FF)
        r.arm("FFacc")
        r.call("face_linear_functional, accumulate", cd.face_linear_functional, fs, cd.MASS_POLY, FFacc, c=0.5, nq=nb + 2, accumulate=True)
        if S.kernel() == "generic":  # no plan: element_ops.hip, atomics
            r.loose |= {"yS", "accS"}
        if M.kernel() == "generic":
            r.loose |= {"yM", "accM"}
    if plan == "0":
        assert S.kernel() == "generic" and {"yS", "accS", "yM", "accM"} <= r.loose
    return r.results()


# element_ops.hip, atomics: the face mass, prolong, the functionals; and the lumped masses the two DiagInv constructors sum
# (lumped_mass_kernel), so that two constructions of one DiagInv operator differ in the last bits of a few shared nodes
ATOMIC = ("yH", "accH", "g", "F1", "F2", "Facc", "FF", "FFacc", "yD", "accD", "yE", "accE")


@pytest.mark.parametrize("kind,nx,nb,plan", [("structured", 10, 4, "1"), ("unstructured", 0, 4, "1"), ("unstructured", 0, 4, "0"), ("structured", 5, 7, "1")])
def test_operators(monkeypatch, kind, nx, nb, plan):
    """StiffnessMatrix, MassMatrix and DiagInvMassMatrix with a delayed device coefficient, the face operators, FaceSpace, nodal
    values and the functionals: built and applied on the side stream, overwrite and accumulate form; plan kernels (n_basis 7: the
    matrix-core plans on the 5 x 5 mesh) bitwise, the generic kernels to 1e-13"""
    monkeypatch.setenv("CUDDH_OPERATOR_PLAN", plan)
    both(operators_case, kind, nx, nb, plan, loose=ATOMIC)


# ================================================================== HelmholtzOperator
def helmholtz_case(r, kind, nx, nb, expect):
    cd = r.cd
    fem0, fs0 = _spaces(kind, nx, nb)
    n, nf = fem0.size(), fs0.size()
    rng = np.random.default_rng(50 + nb)
    a2x, ax = r.floats(a2x=0.5 + rng.random(n), ax=0.5 + rng.random(nf))
    x, zin, b, xg = r.floats(x=rng.standard_normal(2 * n), zin=rng.standard_normal(2 * n), b=rng.standard_normal(2 * n), xg=np.zeros(2 * n))
    y, yu, z, zout, back = r.outs(y=2 * n, yu=2 * n, z=2 * n, zout=2 * n, back=2 * n)
    r.compare("xg")
    with r:
        fem, fs = _spaces(kind, nx, nb)
        r.arm("a2x", "ax")
        A = r.call("HelmholtzOperator(a2x, ax)", cd.HelmholtzOperator, 7.0, a2x, ax, fem, fs)
        assert A.fused() and A.has_native() and A.kernel().startswith(expect), A.kernel()
        r.arm("x")
        r.call("HelmholtzOperator.action", A.action, x, y)
        r.arm("x")
        r.call("HelmholtzOperator.action_unfused", A.action_unfused, x, yu)
        r.arm("x", "zin")  # the native ordering only queues work: one delay
        r.call("HelmholtzOperator.to_native", A.to_native, x, z)
        r.call("HelmholtzOperator.action_native", A.action_native, zin, zout)
        r.call("HelmholtzOperator.from_native", A.from_native, zin, back)
        r.late("to_native, action_native, from_native")
        r.arm("xg", "b")
        out = r.call("HelmholtzOperator.gmres", A.gmres, xg, b, 10, 3, 0.0)  # two cycles of GMRES(10), as test_fused_helmholtz_apply_native_ordering runs them
        r.values.update(num_matvec=out.num_matvec, res_norm=tuple(out.res_norm))
        assert out.num_matvec > 20 and len(out.res_norm) >= 3
    return r.results()


@pytest.mark.parametrize("affine", ["1", "0"])
@pytest.mark.parametrize("kind,nx,nb,variant", [("structured", 10, 4, "lane"), ("structured", 10, 4, "patch"), ("unstructured", 0, 4, "patch"),
                                                ("structured", 5, 7, "mfma")])
def test_helmholtz_operator(monkeypatch, kind, nx, nb, variant, affine):
    """a2x and ax delayed at construction (the plan repacks the metric on the null stream behind the setup's sync); action,
    action_unfused, the native ordering and A.gmres on the lane, patch and matrix-core forms, affine and general plans, selected
    as test_fused_helmholtz_apply_native_ordering selects them"""
    if variant == "lane":
        monkeypatch.setenv("CUDDH_HELM_LANE", "1")
    monkeypatch.setenv("CUDDH_PLAN_AFFINE", affine)
    lane = variant == "lane" and not (affine == "1" and kind == "structured")  # affine plans of n_basis 3, 4 run helm_patch_kernel
    expect = f"helm_lane_kernel<{nb}," if lane else f"helm_mfma_kernel<{nb}," if variant == "mfma" else f"helm_patch_kernel<{nb},"
    both(helmholtz_case, kind, nx, nb, expect, loose=("yu",))


# ================================================================== DDH
def _ddh_coefficient(fem, min_a):
    X = fem.physical_coordinates()
    return min_a + (1.0 - min_a) * 0.5 * (1.0 + np.cos(2.0 * X[0]) * np.cos(1.5 * X[1]))


BLOCK_PLANS = {
    # id: (n_basis, elements per side, min a, DDH keywords)
    "k1-f32": (4, 8, 1.0, dict(precision="f32", kernel=1)),
    "k2-f32": (4, 8, 1.0, dict(precision="f32", kernel=2)),
    "k5-f32": (4, 8, 1.0, dict(precision="f32", kernel=5)),
    "k8-f64": (4, 8, 1.0, dict(precision="f64", kernel=8)),
    "k11-block8": (4, 16, 1.0, dict(precision="f32", kernel=11, block=8)),  # 16 x 16: at 8 x 8 one 8 x 8 block is the whole domain, without traces
    "k12-nb5": (5, 8, 1.0, dict(precision="f32", kernel=12, block=4)),
    "k13-nb5": (5, 8, 1.0, dict(precision="f32", kernel=13, block=4)),
    "k13-coefficient": (4, 8, 0.5, dict(precision="f32", kernel=13, block=4, time_step="coefficient")),  # launch tables sorted by ratio
    "k2-rk4": (4, 8, 1.0, dict(precision="f32", kernel=2, integrator="rk4", coarsen=4)),
}
LABEL_PLANS = {"k9-labels": dict(precision="f64", kernel=9, time_ratios="coefficient"), "k10-labels": dict(precision="f32", kernel=10, time_ratios="coefficient")}


def _block_ddh(cd, name):
    nb, nx, min_a, kw = BLOCK_PLANS[name]
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(nb))
    h_a = np.ones(fem.size()) if min_a == 1.0 else _ddh_coefficient(fem, min_a)
    return cd.DDH(2 * math.pi * nx / 2, h_a, fem, nx, nx, **kw), fem  # one element per wavelength: a short period, accuracy is no concern here


def _label_ddh(cd, name):
    import ddh_general as dg

    mesh = _mesh("unstructured")
    fem = cd.H1Space(mesh, cd.Basis(4))
    xy, el = mesh.vertices(), mesh.elements()
    labels = dg.with_whole_star(dg.morton_labels(xy[el].mean(axis=1)), el, 98)  # the fixture of test_gpu_ddh_unstructured.py
    return cd.DDH.from_labels(8 * math.pi, _ddh_coefficient(fem, 0.6), fem, labels, **LABEL_PLANS[name]), fem


def _ddh(cd, name):
    """a fresh object: host tables only, the plan (geometric factors, uploads, checks, tables, time grids) is built by its first
    call.  (No knob is set here: every setter builds the plan first.)"""
    return (_block_ddh if name in BLOCK_PLANS else _label_ddh)(cd, name)[0]


def _plan_kw(name):
    return BLOCK_PLANS[name][3] if name in BLOCK_PLANS else LABEL_PLANS[name]


@functools.lru_cache(maxsize=None)
def _ddh_shape(name):
    """(traces, subdomains, dofs, kernel) of a plan, from an object of its own on the null stream"""
    import torch

    import cuddhelmholtz_amd as cd

    F = _ddh(cd, name)
    lam = torch.zeros(F.size(), dtype=F.trace_dtype, device="cuda")
    F.action(lam, torch.zeros_like(lam))  # the plan is resolved on first use
    torch.cuda.synchronize()
    info = F.info()
    return F.size(), info["n_domains"], F.fem.size(), info["kernel"]


def ddh_case(r, name):
    n, nd, ndof, kernel = _ddh_shape(name)
    assert n > 0 and nd >= 2 and kernel == _plan_kw(name)["kernel"], (n, nd, kernel)
    torch = r.torch
    rng = np.random.default_rng(nd + n)
    tdt = torch.float32 if _plan_kw(name)["precision"] == "f32" else torch.float64
    f = r.floats(f=rng.standard_normal(2 * ndof))
    lam = r.floats(dtype=tdt, lam=rng.standard_normal(n))
    r.floats(dtype=tdt, ranged=np.zeros(n), listed=np.zeros(n))
    b, y, y_first = r.outs(dtype=tdt, b=n, y=n, y_first=n)
    u = r.outs(u=2 * ndof)
    r.compare("ranged", "listed")
    perm = np.random.default_rng(nd).permutation(nd)
    ids = [r.ints(perm[:nd // 2]), r.ints(perm[nd // 2:])]  # complete before anything runs: never delayed
    with r:
        F = _ddh(r.cd, name)
        r.arm("f")
        r.call("DDH.rhs, first call of a fresh object", F.rhs, f, b)  # builds the plan: tables, checks, "raise on first use"
        r.arm("lam")
        r.call("DDH.action", F.action, lam, y)
        r.arm("lam", "f")
        r.call("DDH.postprocess", F.postprocess, lam, f, u)
        r.arm("f", "lam", "ranged", "listed")  # the four partial launches only queue work: one delay
        r.call("DDH.local_traces, first range", F.local_traces, 0, nd // 2, f, lam, r.buf["ranged"])
        r.call("DDH.local_traces, second range", F.local_traces, nd // 2, nd, f, lam, r.buf["ranged"])
        r.call("DDH.local_traces_listed, first list", F.local_traces_listed, ids[0], f, lam, r.buf["listed"])
        r.call("DDH.local_traces_listed, second list", F.local_traces_listed, ids[1], f, lam, r.buf["listed"])
        r.late("local_traces over two ranges, local_traces_listed over two lists")
        F2 = _ddh(r.cd, name)
        r.arm("lam")
        r.call("DDH.action, first call of a fresh object", F2.action, lam, y_first)
    return r.results()


@pytest.mark.parametrize("name", list(BLOCK_PLANS) + list(LABEL_PLANS))
def test_ddh(name):
    """rhs, action, postprocess, local_traces over two ranges and local_traces_listed (ids not delayed) with f and lam delayed,
    and the first call on a fresh object, for every local-solve kernel family, the per-subdomain time grids, RK4 and the
    label-built plans"""
    both(ddh_case, name)


# ================================================================== WaveHoltz
def _wave_mesh(holed):
    import cuddhelmholtz_amd as cd

    if not holed:
        return cd.Mesh2D.uniform_rect(8, -1.0, 1.0, 8, -1.0, 1.0)
    present = np.ones((8, 8), dtype=bool)
    present[2:5, 3:5] = False  # "hole-8x8" of test_gpu_waveholtz_cells.py
    return cd.Mesh2D.grid_cells(8, -1.0, 1.0, 8, -1.0, 1.0, present)


def _wave_march(r, make, n):
    rng = np.random.default_rng(n)
    f, zin, z = r.floats(f=rng.standard_normal(n), zin=rng.standard_normal(n), z=rng.standard_normal(n))
    b, zout, y, u = r.outs(b=n, zout=n, y=n, u=n)
    with r:
        r.arm(times=CONSTRUCTOR_DELAYS)  # a host coefficient, so nothing delayed goes in: a bare delay makes the set-up kernels late
        t0 = time.perf_counter()
        W = make()
        if r.side is None:
            _CONSTRUCTOR_MS[r.tag] = 1e3 * (time.perf_counter() - t0)  # host and device part together: more than the host part
        elif not CONSTRUCTOR_DELAYS * _S["delay_ms"] > _CONSTRUCTOR_MS[r.tag]:
            r.problems.append(f"the bare delay of {CONSTRUCTOR_DELAYS * _S['delay_ms']:.0f} ms does not outlast the constructor, which took "
                              f"{_CONSTRUCTOR_MS[r.tag]:.0f} ms on the null stream: its set-up kernels may not have been late")
        assert W.size() == n
        r.arm("f")
        r.call("WaveHoltz.rhs, first call", W.rhs, f, b)
        r.arm("zin", "f", "z")  # a period, an action and the solution only queue work: one delay
        r.call("WaveHoltz.period", W.period, zin, f, zout)
        r.call("WaveHoltz.action", W.action, zin, y)
        r.call("WaveHoltz.solution", W.solution, z, u)
        r.late("period, action, solution")
    return r.results()


def waveholtz_case(r, holed, precision, launch):
    cd = r.cd
    fem = cd.H1Space(_wave_mesh(holed), cd.Basis(4))
    X = fem.physical_coordinates()
    h_a = 1.0 + 0.2 * np.cos(X[0]) * np.sin(X[1])
    return _wave_march(r, lambda: cd.WaveHoltz(4 * math.pi, h_a, fem, stiffness="lobatto", sweep="lattice", precision=precision, launch=launch), 2 * fem.size())


@pytest.mark.parametrize("holed,precision,launch", [(False, "f64", "sweep"), (False, "f32", "sweep"), (True, "f64", "sweep"), (True, "f32", "sweep"),
                                                    (False, "f64", "pair"), (False, "f32", "pair")])
def test_waveholtz_lattice(holed, precision, launch):
    """cd.WaveHoltz(sweep="lattice") on the full and the holed 8 x 8 mesh, both precisions, and the paired march: rhs, a period from
    a delayed z_in under a delayed f, action, solution"""
    both(waveholtz_case, holed, precision, launch)


def waveholtz_box_case(r, precision):
    cd = r.cd
    L = 2 * 3 + 1
    k, j, i = np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij")
    h_a = 1.0 + 0.1 * np.cos(0.7 * i) * np.cos(0.5 * j + 0.3 * k)
    return _wave_march(r, lambda: cd.WaveHoltzBox(2 * math.pi, h_a, (2, 2, 2), ((0.0, 1.0), (0.0, 1.0), (0.0, 1.0)), n_basis=4, precision=precision), 2 * L ** 3)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_waveholtz_box(precision):
    both(waveholtz_box_case, precision)


# ================================================================== cd.gmres on operator handles
@functools.lru_cache(maxsize=None)
def _mass_and_preconditioner():
    """One pair for both passes: DiagInvMassMatrix sums its lumped mass with atomics, so a second construction differs in the last
    bits, and a bitwise comparison of two solves needs one preconditioner.  (Construction on the side stream: test_operators.)"""
    import torch

    import cuddhelmholtz_amd as cd

    fem = cd.H1Space(_mesh("structured", 10), cd.Basis(4))
    a = torch.from_numpy(0.5 + np.random.default_rng(4).random(fem.size())).cuda()
    M, P = cd.MassMatrix(fem, a), cd.DiagInvMassMatrix(fem, a)
    torch.cuda.synchronize()
    return M, P


def gmres_mass_case(r):
    cd = r.cd
    fem0 = cd.H1Space(_mesh("structured", 10), cd.Basis(4))
    n = fem0.size()  # 961
    rng = np.random.default_rng(3)
    b = r.floats(b=rng.standard_normal(n))
    runs = {"mgs": dict(orth="mgs"), "cgs2": dict(orth="cgs2"), "aug": dict(augment=2)}
    r.floats(**{f"x_{k}": 0.1 * rng.standard_normal(n) for k in runs})
    r.compare(*[f"x_{k}" for k in runs])
    M, P = _mass_and_preconditioner()
    with r:
        for k, kw in runs.items():
            r.arm("b", f"x_{k}")
            out = r.call(f"gmres {k}", cd.gmres, n, r.buf[f"x_{k}"], M, b, 5, 3, 1e-12, Precond=P, **kw)
            r.values[k] = (out.num_matvec, tuple(out.res_norm))
            assert out.num_matvec >= 5 and len(out.res_norm) >= 2
    return r.results()


def test_gmres_on_an_operator_handle():
    """cd.gmres with MassMatrix and DiagInvMassMatrix as Precond, n = 961, b and x0 delayed: mgs, cgs2 and augment=2; num_matvec,
    every entry of res_norm and x bitwise"""
    both(gmres_mass_case)


def gmres_ddh_case(r, name, arithmetic):
    n, nd, ndof, _ = _ddh_shape(name)
    tdt = r.torch.float32 if _plan_kw(name)["precision"] == "f32" else r.torch.float64
    rng = np.random.default_rng(n)
    b = r.floats(dtype=tdt, b=rng.standard_normal(n))
    x = r.floats(dtype=tdt, x=0.1 * rng.standard_normal(n))
    r.compare("x")
    with r:
        F = _ddh(r.cd, name)
        r.arm("b", "x")
        out = r.call(f"gmres on a DDH, {arithmetic}", r.cd.gmres, n, x, F, b, 3, 3, 0.0, arithmetic=arithmetic)  # two cycles of GMRES(3)
        r.values.update(num_matvec=out.num_matvec, res_norm=tuple(out.res_norm))
        assert out.num_matvec > 6 and len(out.res_norm) >= 3
    return r.results()


@pytest.mark.parametrize("name,arithmetic", [("k2-f32", "real"), ("k8-f64", "complex"), ("k2-f32", "complex")])
def test_gmres_on_a_ddh_handle(name, arithmetic):
    """fp32 Krylov vectors and arithmetic="complex" with a DDH queued one step ahead of the host"""
    both(gmres_ddh_case, name, arithmetic)


# ================================================================== created on one stream, used on another
def crossing_case(r, built_on_null):
    """built_on_null: the objects are built on the null stream and applied on the run's stream with delayed inputs; otherwise built
    on the run's stream (delayed coefficients) and applied on the null stream after the synchronisation"""
    cd, torch = r.cd, r.torch
    fem, fs = _spaces("structured", 10, 4)
    n, nf = fem.size(), fs.size()
    nl, nd, ndof, _ = _ddh_shape("k2-f32")
    rng = np.random.default_rng(17)
    a2x, ax, x = r.floats(a2x=0.5 + rng.random(n), ax=0.5 + rng.random(nf), x=rng.standard_normal(2 * n))
    lam = r.floats(dtype=torch.float32, lam=rng.standard_normal(nl))
    y = r.outs(y=2 * n)
    t = r.outs(dtype=torch.float32, t=nl)
    warm = r.floats(dtype=torch.float32, warm=rng.standard_normal(nl))
    warm_out = torch.zeros(nl, dtype=torch.float32, device=r.dev)

    def build():
        """both objects with all their device state: a DDH creates its plan, geometric factors, tables and uploads in its first
        call, so one action into a buffer that is not compared makes them here, on the building stream; on the side stream each
        of the two has a delay of its own in front, since the HelmholtzOperator's constructor synchronises"""
        r.arm("a2x", "ax")
        A = cd.HelmholtzOperator(7.0, a2x, ax, fem, fs)
        F = _ddh(cd, "k2-f32")
        r.arm("warm")
        F.action(warm, warm_out)
        assert F.info()["kernel"] == 2
        return A, F

    def apply(A, F):
        r.arm("x")
        A.action(x, y)
        r.arm("lam")
        F.action(lam, t)

    def on_the_null_stream(fn, *args):
        """outside `with r`, where the library is on torch's default stream: arm() then only copies"""
        side, r.side = r.side, None
        try:
            out = fn(*args)
            torch.cuda.synchronize()
        finally:
            r.side = side
        return out

    if built_on_null:
        A, F = on_the_null_stream(build)
        with r:
            apply(A, F)
    else:
        with r:
            A, F = build()
        on_the_null_stream(apply, A, F)
    return r.results()


@pytest.mark.parametrize("built_on_null", [True, False], ids=["null-then-side", "side-then-null"])
def test_objects_cross_streams_after_a_synchronisation(built_on_null):
    """one HelmholtzOperator and one fp32 DDH built on one stream and, after a synchronisation, applied on the other (the DDH
    creates its plan in a warm-up action on the building stream, so the apply finds a plan, geometric factors and tables made on the
    other stream)"""
    both(crossing_case, built_on_null)


# ================================================================== a slice of the direct C ABI
def _p(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset * t.element_size())


def blas1_case(r, dtype):
    import blas1_reference as br
    from test_gpu_blas1_kernels import Ctx

    n, M = 3 * 1024 * (2 if dtype == "f64" else 4) + 11, br.MAX_PARTIALS  # several tiles, a partial one and a scalar tail
    tdt = r.torch.float64 if dtype == "f64" else r.torch.float32
    rng = np.random.default_rng(n)
    x, y, w, v0, v1 = r.floats(dtype=tdt, x=rng.standard_normal(n), y=rng.standard_normal(n), w=rng.standard_normal(n), v0=rng.standard_normal(n) / math.sqrt(n),
                               v1=rng.standard_normal(n) / math.sqrt(n))
    ws = r.floats(ws=np.zeros(2 * M))
    part = r.floats(dtype=tdt, part=np.zeros(2 * M))
    res, h = r.outs(dtype=tdt, res=3, h=2)
    r.compare("w", "part")
    with r:
        ctx = Ctx(r.dev)  # its call() passes torch's current stream: the run's
        r.arm("x", "y", "ws")
        ctx.call(f"dot_{dtype}", n, _p(x), _p(y), _p(res, 0), _p(ws))
        ctx.call(f"sqdist_{dtype}", n, _p(x), _p(y), _p(res, 1), _p(ws))
        ctx.call(f"nrm2_{dtype}", n, _p(x), _p(res, 2), _p(ws))
        r.late("dot, sqdist, nrm2")
        # one fused Gram-Schmidt stage behind the stage that produces its partial sums (krylov.cpp::queue_step)
        r.arm("w", "v0", "v1", "part")
        ctx.call(f"mgs_stage_{dtype}", n, _p(w), None, _p(v0), _p(part), _p(part), _p(h, 0))
        ctx.call(f"mgs_stage_{dtype}", n, _p(w), _p(v0), _p(v1), _p(part), _p(part, M), _p(h, 1))
        r.late("two Gram-Schmidt stages")
    return r.results()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cabi_reductions_and_gram_schmidt_stage(dtype):
    """cuddh_hip_dot / sqdist / nrm2 with their workspace and one fused Gram-Schmidt stage, `st` the side stream"""
    both(blas1_case, dtype)


def krylov_update_case(r):
    from test_gpu_blas1_kernels import Ctx

    n, nv, nz = 2 * 1024 * 2 + 5, 3, 2
    rng = np.random.default_rng(n)
    x, V, Z, coef = r.floats(x=rng.standard_normal(n), V=rng.standard_normal(nv * n), Z=rng.standard_normal(nz * n), coef=rng.standard_normal(nv + nz))
    dx, pout = r.outs(dx=n, pout=Ctx(r.dev).lib.cuddh_hip_cgs_ws_bytes(0) // 8)
    r.compare("x")
    with r:
        r.arm("x", "V", "Z", "coef")
        Ctx(r.dev).call("krylov_update_f64", n, _p(x), _p(dx), _p(V), n, nv, _p(Z), n, nz, _p(coef), _p(pout))
    return r.results()


def test_cabi_krylov_update():
    both(krylov_update_case)


def wave_box_case(r):
    from test_gpu_wave_box_kernels import description, dims

    from cuddhelmholtz_amd import _native as N

    lat = (2, 2, 2, 3)
    Lx, Ly, Lz, stride = dims(*lat)
    rng = np.random.default_rng(3)
    A, w = rng.standard_normal((3, 3)), rng.random(3) + 0.5
    D = description(N, *lat, stride, A, w)
    pad = np.ones((Lz, Ly, stride))
    pad[:, :, Lx:] = 0.0
    names = ("ps", "p", "q", "invm", "Hi", "F", "G", "qs", "aq", "ap")
    r.floats(**{v: (rng.standard_normal((Lz, Ly, stride)) * pad).reshape(-1) for v in names})
    r.outs(ps_out=Lz * Ly * stride)
    r.compare("qs", "aq", "ap")
    with r:
        r.arm(*names)
        st = C.c_void_p(r.torch.cuda.current_stream().cuda_stream)
        ptr = lambda v: _p(r.buf[v])  # noqa: E731
        N.check(N.lib.cuddh_hip_wave_box_rk4_2_f64(C.byref(D), 0.37, 0.8, -0.6, ptr("ps"), ptr("p"), ptr("q"), ptr("invm"), ptr("Hi"), ptr("F"), ptr("G"),
                                                   ptr("ps_out"), ptr("qs"), ptr("aq"), ptr("ap"), st), "rk4_2")
    return r.results()


def test_cabi_wave_box_rk4_2():
    """cuddh_hip_wave_box_rk4_2_f64 on (2, 2, 2, 3), forced form, every lattice vector delayed"""
    both(wave_box_case)


def halo_case(r):
    from test_gpu_blas1_kernels import Ctx

    n, n_half = 1500, 3007
    rng = np.random.default_rng(n)
    ids = r.ints(rng.permutation(n_half)[:n])  # complete before anything runs: never delayed
    v, other = r.floats(v=rng.standard_normal(2 * n_half), other=rng.standard_normal(2 * n_half))
    packed = r.floats(packed=rng.standard_normal(2 * n))
    buf = r.outs(buf=2 * n)
    r.compare("v", "other")
    with r:
        ctx = Ctx(r.dev)
        r.arm("v")
        ctx.call("halo_pack_f64", n, n_half, _p(ids), _p(v), _p(buf), 1)  # pack and clear
        r.arm("packed", "other")
        ctx.call("halo_unpack_f64", n, n_half, _p(ids), _p(packed), _p(other), 1)  # add
    return r.results()


def test_cabi_halo_pack_unpack():
    both(halo_case)


# ================================================================== what the delay has to cover
def test_report_the_longest_call():
    """Prints the figures the module docstring records: the delay and the longest library calls on the null stream that the tests
    before it timed."""
    top = sorted(_TIMES.items(), key=lambda kv: -kv[1])[:8]
    print(f"stream order: delay {_S['delay_ms']:.1f} ms (DELAY_MS {DELAY_MS}); canary: {_S['canary']}; longest calls on the null stream: "
          + "; ".join(f"{k} {v:.2f} ms" for k, v in top))
