"""The step schedule of DDH kernel 5's scaled march with the velocity carried already multiplied by its chain head (head 2,
wh_march_pairs_carried) against the schedule that multiplies it out in every step (head 1, wh_march_pairs_scaled), both restated
in numpy on one subdomain (tests/ddh_head_march.py).  No GPU.

  * fp64: the two schedules are the same scheme, so they agree to rounding, 1e-12 relative (measured: 2.0e-16 to 8.7e-16);
  * fp32: they differ as two roundings of one scheme do.  profiles/r31 reports 3.0e-7 to 5.7e-7 between march 1 and march 2 on the
    device; the gate is twice the smaller figure, 6.0e-7 (measured here, u / v: 2.1e-7 / 3.6e-7 on squares,
    3.2e-7 / 4.2e-7 on hy = hx / 2, 1.1e-7 / 4.3e-7 with one WaveHoltz pass), and each schedule stays as close to the fp64 march as
    the other, within a factor 2.
Every figure is printed (`pytest -s`)."""
import numpy as np
import pytest

import ddh_head_march as H

CASES = {"square": dict(), "rect": dict(hy=0.125, nt=800), "one pass": dict(wh_iters=1)}


def _rel(a, b, ref):
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / np.linalg.norm(ref))


@pytest.fixture(scope="module", params=list(CASES))
def marched(request):
    c = H.case(**CASES[request.param])
    return request.param, {(dt, carried): H.march(c, dt, carried) for dt in (np.float64, np.float32) for carried in (False, True)}


def test_the_two_schedules_are_one_scheme_in_fp64(marched):
    name, m = marched
    for i, field in enumerate("uv"):
        ref = m[np.float64, False][i]
        d = _rel(m[np.float64, True][i], ref, ref)
        print(f"[{name}] {field}: carried vs multiplied in fp64 {d:.3e} (gate 1e-12)")
        assert np.linalg.norm(ref) > 1 and d < 1e-12, (field, d)


def test_the_two_schedules_differ_by_rounding_in_fp32(marched):
    name, m = marched
    for i, field in enumerate("uv"):
        ref = m[np.float64, False][i]
        d = _rel(m[np.float32, True][i], m[np.float32, False][i], ref)
        e1, e2 = _rel(m[np.float32, False][i], ref, ref), _rel(m[np.float32, True][i], ref, ref)
        print(f"[{name}] {field}: carried vs multiplied in fp32 {d:.3e} (gate 6.0e-7); vs the fp64 march: multiplied {e1:.3e}, carried {e2:.3e}")
        assert 0 < d < 2 * 3.0e-7, (field, d)
        assert e2 < 2 * e1, (field, e1, e2)

