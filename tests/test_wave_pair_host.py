"""The host side of launch="pair" of cd.WaveHoltz (two lattice sweeps per launch): no GPU.

Refusals: a bad launch name, or "pair" without sweep="lattice", is a ValueError naming `launch` before the space is touched; the C
API refuses launch codes other than 0 / 1 and 1 without the lattice form with "WaveHoltz error: launch:" before it allocates
anything (no device here).  The new kernel entry points and C-API names are declared (test_cabi_exports.py then holds the library to
them).

The paired schedule in numpy: tests/wave_pair_reference.py states each pair from its pointwise table (derived tile, two stencils,
two stage formulas) and marches nt steps with the solver's buffer swaps.  Its u, v equal, bit for bit, those of the per-sweep
restatements the one-sweep kernels are held to (ref_rk2_a / _b, ref_rk4_1 / _mid / _4 of test_gpu_wave_stage_kernels.py with the
stencil of test_gpu_wave_lattice_kernels.py), for nt = 3 and 4 (both parities of the swaps), forced and homogeneous, on (3, 2, 4) and
(2, 3, 5).  Inputs are integers and powers of two.
"""
import numpy as np
import pytest

import cuddhelmholtz_amd as cd
from cuddhelmholtz_amd import _native as N

import wave_pair_reference as wp
from test_gpu_wave_lattice_kernels import host_vectors, stencil, tables
from test_gpu_wave_stage_kernels import CS, DT, FILT, HALF_DT, SIXTH_DT, SN, ref_rk2_a, ref_rk2_b, ref_rk4_1, ref_rk4_4, ref_rk4_mid

KERNEL_ENTRY_POINTS = [f"cuddh_hip_wave_pair_{name}" for name in ("rk2_f64", "rk4_12_f64", "rk4_34_f64", "tile_x", "tile_y")] + \
                      [f"cuddh_hip_wave_pair32_{name}" for name in ("rk2", "rk4_12", "rk4_34", "tile_x", "tile_y")]


class NoSpace:  # anything that touches the space fails the test with another exception
    def __getattr__(self, name):
        raise AssertionError(f"the space was used ({name}) before the arguments were checked")


@pytest.mark.parametrize("kwargs", [dict(launch="pairs", stiffness="lobatto", sweep="lattice"), dict(launch=1, stiffness="lobatto", sweep="lattice"),
                                    dict(launch="pair"), dict(launch="pair", sweep="operator"), dict(launch="pair", stiffness="lobatto", sweep="operator")],
                         ids=["pairs", "1", "pair-default-sweep", "pair-operator", "pair-operator-lobatto"])
def test_bad_launch_raises_before_the_space_is_touched(kwargs):
    with pytest.raises(ValueError, match="launch"):
        cd.WaveHoltz(1.0, np.ones(4), NoSpace(), **kwargs)
    assert cd.WaveHoltz.LAUNCHES == ("sweep", "pair")


def test_native_refusals_of_the_option_itself():
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(2, -1.0, 1.0, 2, -1.0, 1.0), cd.Basis(2))
    a = np.ones(fem.size())
    # (stiffness, sweep, precision, launch)
    for codes in ((1, 0, 0, 1), (0, 0, 0, 1), (1, 1, 0, 2), (1, 1, 0, -1), (1, 1, 1, 2), (1, 0, 0, 2)):
        stiffness, sweep, precision, launch = codes
        h = N.lib.cuddh_waveholtz_create_launch(1.0, a.ctypes.data, fem._h, 0, 1, 1, stiffness, None, -1, sweep, precision, launch)
        assert not h and N.last_error().startswith("WaveHoltz error: launch:"), (codes, N.last_error())
    assert N.lib.cuddh_waveholtz_launch(None) == -1
    # launch = 0 is cuddh_waveholtz_create_precision: its refusals keep their names
    h = N.lib.cuddh_waveholtz_create_launch(1.0, a.ctypes.data, fem._h, 0, 1, 1, 1, None, -1, 0, 1, 0)
    assert not h and N.last_error().startswith("WaveHoltz error: precision:"), N.last_error()
    h = N.lib.cuddh_waveholtz_create_launch(1.0, a.ctypes.data, fem._h, 0, 1, 1, 1, None, -1, 2, 0, 0)
    assert not h and N.last_error().startswith("WaveHoltz error: sweep:"), N.last_error()


def test_new_symbols_are_declared():
    declared = set(N.declared_symbols())
    missing = [s for s in (*KERNEL_ENTRY_POINTS, "cuddh_waveholtz_create_launch", "cuddh_waveholtz_launch") if s not in declared]
    assert not missing, missing
    assert len(KERNEL_ENTRY_POINTS) == 10


def per_sweep_march(nx, ny, nb, stride, A, w, x, nt, rk4, forced):
    """nt steps of the per-sweep schedule of csrc/src/waveholtz.cpp on the existing restatements; returns (u, v)"""
    b = {name: v.copy() for name, v in x.items()}
    K = lambda v: stencil(nx, ny, nb, stride, A, w, v)  # noqa: E731
    for _ in range(nt):
        if not rk4:
            y = ref_rk2_a({**b, "w": K(b["p"])}, forced)
            b["qs"], b["ps"] = y["qs"], y["ps"]
            y = ref_rk2_b({**b, "w": K(b["ps"])}, forced)
        else:
            y = ref_rk4_1({**b, "w": K(b["p"])}, forced)
            b.update(y)
            y = ref_rk4_mid(HALF_DT)({**b, "w": K(b["ps"])}, forced)
            b.update(y)
            y = ref_rk4_mid(DT)({**b, "w": K(b["ps"])}, forced)
            b.update(y)
            y = ref_rk4_4({**b, "w": K(b["ps"])}, forced)
        b.update(y)
    return b["u"], b["v"]


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "homogeneous"])
@pytest.mark.parametrize("rk4", [False, True], ids=["rk2", "rk4"])
@pytest.mark.parametrize("nt", [3, 4])
@pytest.mark.parametrize("nx,ny,nb", [(3, 2, 4), (2, 3, 5)])
def test_paired_schedule_gives_the_per_sweep_bits(nx, ny, nb, nt, rk4, forced):
    Lx = nx * (nb - 1) + 1
    stride = Lx + Lx % 2
    A, w = tables(nb, seed=nb)
    x = host_vectors(nx, ny, nb, stride, seed=7 * nx + ny)
    scalars = dict(half_dt=HALF_DT, dt=DT, sixth_dt=SIXTH_DT, c=CS, s=SN, filt=FILT)
    u, v = wp.march_pairs(wp.stiffness(nx, ny, nb, stride, A, w), x, nt, rk4, scalars, forced)
    want_u, want_v = per_sweep_march(nx, ny, nb, stride, A, w, x, nt, rk4, forced)
    assert np.all(np.isfinite(want_u)) and float(np.abs(want_u).max()) > 0 and not np.array_equal(want_u, x["u"])
    assert np.array_equal(u.view(np.uint64), want_u.view(np.uint64))
    assert np.array_equal(v.view(np.uint64), want_v.view(np.uint64))
    if not forced:  # the load matters
        fu, _ = per_sweep_march(nx, ny, nb, stride, A, w, x, nt, rk4, True)
        assert not np.array_equal(fu, want_u)
