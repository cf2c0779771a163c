"""DDH local-solve kernels 1 to 13 on rectangles (hx != hy), parallelograms (g01 != 0, one metric) and skewed quadrilaterals
(every element its own metric) against ddh_general.OracleDDH, on the cases of tests/ddh_metric_cases.py (proven on the CPU
in tests/test_ddh_metric_cases.py: valid elements, angles, the two oracle restatements, floors, and that g01 -> -g01 moves the
reference by more than 4e4 fp32 gates).

  (a) parity: every kernel at the n_basis and block it is built for (KERNELS[] in ddh_resolve.cpp), in both precisions where
      it has both, on every family that it accepts: rhs, action (on the written slots) and postprocess into pre-filled
      buffers, against the fp64 oracle.  fp64: relative l2 <= 1e-10, the project's fp64 DDH gate.  fp32: relative l2 and max
      norm <= 4 x the fp32 oracle's own distance to the fp64 oracle on the same case (the floor rule of
      tests/test_gpu_ddh_block_size.py; the kernel's summation order is as legitimate as the fp32 oracle's, and a metric
      fault costs g01 / sqrt(g00 g11) ~ 1e-1, four orders above the gate);
  (b) local_traces over [0, nd), over [0, 3) + [3, nd) and local_traces_listed in a permuted order cut after five are bitwise
      equal on the new meshes, among them kernel 6 (two subdomains per wavefront) and kernel 5's element-lane form (four);
  (c) what a plan refuses on these meshes (kernels that need a diagonal, separable metric on `shear`, those that need one
      metric for all elements on `skew`) and what auto takes.  `shear` has exact coordinates and passes the bitwise
      uniformity check: fp32 auto at n_basis 4 stays on kernel 5, in its matrix form.

Every distance, floor and ratio is printed (`pytest -s`).  Measured on one MI355X:
fp64, relative l2 to the fp64 oracle, largest of rhs / action / postprocess per kernel (gate 1e-10):
  8x12 n_basis 4 block 4 square: 1: 5.2e-16, 2: 4.8e-16, 3: 4.8e-16, 4: 4.8e-16, 8: 7.3e-16, 9: 5.0e-16, 10: 5.2e-16
  8x12 n_basis 4 block 4 rect  : 1: 5.6e-16, 2: 5.8e-16, 3: 5.8e-16, 4: 5.8e-16, 8: 1.2e-15, 9: 5.7e-16, 10: 5.6e-16
  8x12 n_basis 4 block 4 shear : 1: 6.3e-16, 2: 5.5e-16, 3: 5.5e-16, 4: 5.5e-16, 8: 4.3e-15, 9: 5.8e-16, 10: 6.3e-16
  8x12 n_basis 4 block 4 skew  : 1: 5.2e-16, 2: 5.4e-16, 3: 5.4e-16, 4: 5.4e-16, 9: 5.9e-16, 10: 5.2e-16
  4x6 n_basis 8 block 2 square: 1: 8.1e-16, 6: 8.7e-16, 10: 8.1e-16
  4x6 n_basis 8 block 2 rect  : 1: 1.1e-15, 6: 1.2e-15, 10: 1.1e-15
  4x6 n_basis 8 block 2 shear : 1: 1.1e-15, 6: 1.2e-15, 10: 1.1e-15
  4x6 n_basis 8 block 2 skew  : 1: 1.0e-15, 6: 9.9e-16, 10: 1.0e-15
  8x12 n_basis 5 block 4 square: 1: 6.4e-16
  8x12 n_basis 5 block 4 rect  : 1: 8.1e-16
  8x12 n_basis 5 block 4 shear : 1: 8.1e-16
  8x12 n_basis 5 block 4 skew  : 1: 8.3e-16
  16x8 n_basis 4 block 8 rect  : 1: 1.0e-15
  16x8 n_basis 4 block 8 shear : 1: 8.1e-16

fp32: per output `distance (ratio)` in relative l2, then in max norm; floor = fp32 oracle vs fp64 oracle; gate: ratio <= 4.
  8x12 n_basis 4 block 4 square: floors l2 4.41e-07 / 2.85e-07 / 4.56e-07; max 5.67e-07 / 4.28e-07 / 9.16e-07
    kernel     rhs                               action                            postprocess
    1          4.15e-07 (0.94) 5.67e-07 (1.00) 2.67e-07 (0.94) 3.21e-07 (0.75) 4.61e-07 (1.01) 8.07e-07 (0.88)
    2          4.36e-07 (0.99) 5.69e-07 (1.00) 2.68e-07 (0.94) 3.21e-07 (0.75) 4.60e-07 (1.01) 8.23e-07 (0.90)
    3          4.63e-07 (1.05) 5.69e-07 (1.00) 2.68e-07 (0.94) 3.21e-07 (0.75) 4.61e-07 (1.01) 8.23e-07 (0.90)
    4          4.14e-07 (0.94) 6.27e-07 (1.11) 2.77e-07 (0.97) 3.46e-07 (0.81) 4.61e-07 (1.01) 1.01e-06 (1.10)
    5 form 1   9.29e-07 (2.11) 7.67e-07 (1.35) 3.60e-07 (1.26) 4.28e-07 (1.00) 8.57e-07 (1.88) 1.10e-06 (1.20)
    5 form 2   4.96e-07 (1.12) 7.28e-07 (1.28) 2.78e-07 (0.98) 3.46e-07 (0.81) 5.04e-07 (1.11) 1.05e-06 (1.15)
    9          4.52e-07 (1.03) 5.69e-07 (1.00) 2.79e-07 (0.98) 3.21e-07 (0.75) 4.58e-07 (1.01) 1.01e-06 (1.10)
    10         4.15e-07 (0.94) 5.67e-07 (1.00) 2.67e-07 (0.94) 3.21e-07 (0.75) 4.61e-07 (1.01) 8.07e-07 (0.88)
    13         4.96e-07 (1.12) 7.28e-07 (1.28) 2.78e-07 (0.98) 3.46e-07 (0.81) 5.04e-07 (1.11) 1.05e-06 (1.15)
  8x12 n_basis 4 block 4 rect: floors l2 5.24e-07 / 3.81e-07 / 5.46e-07; max 9.90e-07 / 6.15e-07 / 1.08e-06
    kernel     rhs                               action                            postprocess
    1          5.66e-07 (1.08) 9.25e-07 (0.93) 3.96e-07 (1.04) 6.68e-07 (1.09) 5.62e-07 (1.03) 1.15e-06 (1.06)
    2          5.40e-07 (1.03) 1.06e-06 (1.07) 3.95e-07 (1.04) 7.40e-07 (1.20) 5.37e-07 (0.98) 1.04e-06 (0.97)
    3          5.58e-07 (1.06) 1.18e-06 (1.20) 3.81e-07 (1.00) 6.15e-07 (1.00) 5.51e-07 (1.01) 1.06e-06 (0.99)
    4          5.60e-07 (1.07) 1.06e-06 (1.07) 3.83e-07 (1.00) 7.40e-07 (1.20) 5.47e-07 (1.00) 1.08e-06 (1.00)
    5 form 1   6.79e-07 (1.30) 1.18e-06 (1.20) 4.00e-07 (1.05) 5.53e-07 (0.90) 5.96e-07 (1.09) 1.08e-06 (1.00)
    5 form 2   6.19e-07 (1.18) 9.90e-07 (1.00) 4.00e-07 (1.05) 8.02e-07 (1.30) 5.97e-07 (1.09) 1.06e-06 (0.99)
    9          5.59e-07 (1.07) 1.06e-06 (1.07) 4.04e-07 (1.06) 6.77e-07 (1.10) 5.42e-07 (0.99) 1.15e-06 (1.06)
    10         5.66e-07 (1.08) 9.25e-07 (0.93) 3.96e-07 (1.04) 6.68e-07 (1.09) 5.62e-07 (1.03) 1.15e-06 (1.06)
    13         6.19e-07 (1.18) 9.90e-07 (1.00) 4.00e-07 (1.05) 8.02e-07 (1.30) 5.97e-07 (1.09) 1.06e-06 (0.99)
  8x12 n_basis 4 block 4 shear: floors l2 5.01e-07 / 3.10e-07 / 5.46e-07; max 7.83e-07 / 4.94e-07 / 9.67e-07
    kernel     rhs                               action                            postprocess
    1          5.33e-07 (1.06) 8.54e-07 (1.09) 2.96e-07 (0.95) 4.00e-07 (0.81) 5.46e-07 (1.00) 9.32e-07 (0.96)
    2          5.46e-07 (1.09) 7.90e-07 (1.01) 3.13e-07 (1.01) 4.73e-07 (0.96) 5.39e-07 (0.99) 9.49e-07 (0.98)
    3          5.17e-07 (1.03) 8.54e-07 (1.09) 2.94e-07 (0.95) 4.00e-07 (0.81) 5.36e-07 (0.98) 8.82e-07 (0.91)
    4          5.41e-07 (1.08) 7.89e-07 (1.01) 2.99e-07 (0.96) 4.61e-07 (0.93) 5.47e-07 (1.00) 8.82e-07 (0.91)
    5 form 1   1.20e-06 (2.39) 1.52e-06 (1.94) 4.09e-07 (1.32) 6.61e-07 (1.34) 9.69e-07 (1.78) 1.15e-06 (1.19)
    9          5.00e-07 (1.00) 7.43e-07 (0.95) 3.07e-07 (0.99) 5.04e-07 (1.02) 5.59e-07 (1.02) 8.82e-07 (0.91)
    10         5.33e-07 (1.06) 8.54e-07 (1.09) 2.96e-07 (0.95) 4.00e-07 (0.81) 5.46e-07 (1.00) 9.32e-07 (0.96)
  8x12 n_basis 4 block 4 skew: floors l2 5.43e-07 / 3.50e-07 / 5.67e-07; max 7.49e-07 / 6.91e-07 / 1.53e-06
    kernel     rhs                               action                            postprocess
    1          5.03e-07 (0.93) 7.05e-07 (0.94) 3.48e-07 (0.99) 6.91e-07 (1.00) 5.81e-07 (1.03) 1.44e-06 (0.94)
    2          5.45e-07 (1.00) 8.12e-07 (1.08) 3.58e-07 (1.02) 6.91e-07 (1.00) 5.61e-07 (0.99) 1.27e-06 (0.83)
    3          4.64e-07 (0.85) 6.51e-07 (0.87) 3.56e-07 (1.02) 6.91e-07 (1.00) 5.56e-07 (0.98) 1.44e-06 (0.94)
    4          4.99e-07 (0.92) 7.05e-07 (0.94) 3.60e-07 (1.03) 6.30e-07 (0.91) 5.77e-07 (1.02) 1.44e-06 (0.94)
    9          4.86e-07 (0.89) 6.50e-07 (0.87) 3.58e-07 (1.02) 6.91e-07 (1.00) 5.76e-07 (1.02) 1.61e-06 (1.06)
    10         5.03e-07 (0.93) 7.05e-07 (0.94) 3.48e-07 (0.99) 6.91e-07 (1.00) 5.81e-07 (1.03) 1.44e-06 (0.94)
  4x6 n_basis 8 block 2 square: floors l2 7.43e-07 / 4.23e-07 / 7.84e-07; max 1.39e-06 / 6.89e-07 / 1.64e-06
    kernel     rhs                               action                            postprocess
    1          7.04e-07 (0.95) 1.22e-06 (0.88) 4.14e-07 (0.98) 6.89e-07 (1.00) 7.50e-07 (0.96) 1.42e-06 (0.87)
    6          7.56e-07 (1.02) 1.28e-06 (0.93) 4.09e-07 (0.97) 6.89e-07 (1.00) 7.59e-07 (0.97) 1.55e-06 (0.94)
    7          1.98e-06 (2.66) 2.50e-06 (1.80) 6.52e-07 (1.54) 1.00e-06 (1.46) 1.61e-06 (2.05) 2.46e-06 (1.50)
    10         7.04e-07 (0.95) 1.22e-06 (0.88) 4.14e-07 (0.98) 6.89e-07 (1.00) 7.50e-07 (0.96) 1.42e-06 (0.87)
  4x6 n_basis 8 block 2 rect: floors l2 9.03e-07 / 5.52e-07 / 1.10e-06; max 1.52e-06 / 8.25e-07 / 1.90e-06
    kernel     rhs                               action                            postprocess
    1          8.81e-07 (0.98) 1.75e-06 (1.15) 5.48e-07 (0.99) 8.87e-07 (1.07) 1.12e-06 (1.02) 1.82e-06 (0.95)
    6          9.44e-07 (1.05) 1.56e-06 (1.03) 5.47e-07 (0.99) 7.99e-07 (0.97) 1.11e-06 (1.01) 1.78e-06 (0.93)
    7          3.23e-06 (3.58) 2.92e-06 (1.91) 9.37e-07 (1.70) 1.01e-06 (1.22) 2.50e-06 (2.28) 2.58e-06 (1.36)
    10         8.81e-07 (0.98) 1.75e-06 (1.15) 5.48e-07 (0.99) 8.87e-07 (1.07) 1.12e-06 (1.02) 1.82e-06 (0.95)
  4x6 n_basis 8 block 2 shear: floors l2 9.33e-07 / 5.21e-07 / 1.14e-06; max 1.29e-06 / 8.27e-07 / 2.72e-06
    kernel     rhs                               action                            postprocess
    1          9.71e-07 (1.04) 1.53e-06 (1.19) 4.98e-07 (0.96) 7.96e-07 (0.96) 1.07e-06 (0.94) 2.04e-06 (0.75)
    6          9.84e-07 (1.05) 1.51e-06 (1.17) 5.04e-07 (0.97) 7.96e-07 (0.96) 1.09e-06 (0.95) 1.99e-06 (0.73)
    10         9.71e-07 (1.04) 1.53e-06 (1.19) 4.98e-07 (0.96) 7.96e-07 (0.96) 1.07e-06 (0.94) 2.04e-06 (0.75)
  4x6 n_basis 8 block 2 skew: floors l2 9.93e-07 / 5.64e-07 / 1.09e-06; max 1.66e-06 / 9.66e-07 / 3.22e-06
    kernel     rhs                               action                            postprocess
    1          9.56e-07 (0.96) 1.30e-06 (0.78) 5.66e-07 (1.00) 9.97e-07 (1.03) 1.10e-06 (1.01) 3.00e-06 (0.93)
    6          9.50e-07 (0.96) 1.24e-06 (0.75) 5.73e-07 (1.01) 1.11e-06 (1.14) 1.12e-06 (1.02) 3.32e-06 (1.03)
    10         9.56e-07 (0.96) 1.30e-06 (0.78) 5.66e-07 (1.00) 9.97e-07 (1.03) 1.10e-06 (1.01) 3.00e-06 (0.93)
  8x12 n_basis 5 block 4 square: floors l2 4.50e-07 / 3.40e-07 / 5.12e-07; max 5.57e-07 / 5.87e-07 / 7.93e-07
    kernel     rhs                               action                            postprocess
    1          4.22e-07 (0.94) 6.74e-07 (1.21) 3.35e-07 (0.99) 5.87e-07 (1.00) 5.31e-07 (1.04) 1.06e-06 (1.34)
    12         7.42e-07 (1.65) 7.01e-07 (1.26) 3.79e-07 (1.11) 5.61e-07 (0.96) 7.83e-07 (1.53) 7.89e-07 (1.00)
    13         7.42e-07 (1.65) 7.01e-07 (1.26) 3.79e-07 (1.11) 5.61e-07 (0.96) 7.83e-07 (1.53) 7.89e-07 (1.00)
  8x12 n_basis 5 block 4 rect: floors l2 6.54e-07 / 3.34e-07 / 7.19e-07; max 1.25e-06 / 4.72e-07 / 1.72e-06
    kernel     rhs                               action                            postprocess
    1          6.63e-07 (1.01) 1.19e-06 (0.95) 3.39e-07 (1.01) 4.66e-07 (0.99) 7.02e-07 (0.98) 1.57e-06 (0.91)
    12         7.05e-07 (1.08) 1.32e-06 (1.05) 3.64e-07 (1.09) 4.43e-07 (0.94) 7.29e-07 (1.01) 1.64e-06 (0.95)
    13         7.05e-07 (1.08) 1.32e-06 (1.05) 3.64e-07 (1.09) 4.43e-07 (0.94) 7.29e-07 (1.01) 1.64e-06 (0.95)
  8x12 n_basis 5 block 4 shear: floors l2 6.06e-07 / 4.03e-07 / 6.94e-07; max 1.02e-06 / 7.88e-07 / 1.77e-06
    kernel     rhs                               action                            postprocess
    1          6.16e-07 (1.02) 1.09e-06 (1.08) 3.97e-07 (0.99) 6.61e-07 (0.84) 6.85e-07 (0.99) 1.77e-06 (1.00)
  8x12 n_basis 5 block 4 skew: floors l2 6.06e-07 / 3.48e-07 / 6.82e-07; max 6.75e-07 / 5.49e-07 / 1.26e-06
    kernel     rhs                               action                            postprocess
    1          6.65e-07 (1.10) 9.99e-07 (1.48) 3.43e-07 (0.98) 4.56e-07 (0.83) 6.98e-07 (1.02) 1.32e-06 (1.05)
  16x8 n_basis 4 block 8 rect: floors l2 4.35e-07 / 1.80e-07 / 6.69e-07; max 4.46e-07 / 4.72e-07 / 9.74e-07
    kernel     rhs                               action                            postprocess
    1          4.70e-07 (1.08) 3.70e-07 (0.83) 1.94e-07 (1.08) 4.72e-07 (1.00) 6.69e-07 (1.00) 1.07e-06 (1.10)
    11         7.27e-07 (1.67) 5.98e-07 (1.34) 1.65e-07 (0.92) 3.45e-07 (0.73) 7.51e-07 (1.12) 9.36e-07 (0.96)
  16x8 n_basis 4 block 8 shear: floors l2 8.35e-07 / 1.10e-07 / 6.63e-07; max 8.39e-07 / 1.33e-07 / 1.29e-06
    kernel     rhs                               action                            postprocess
    1          8.33e-07 (1.00) 7.42e-07 (0.89) 1.17e-07 (1.07) 1.33e-07 (1.00) 6.68e-07 (1.01) 1.28e-06 (0.99)

No cell misses a gate and no fault was found.  The largest fp32 ratio is 3.58 (kernel 7, rhs, rect; 2.66 on square), then 2.39
(kernel 5's matrix form, rhs, shear; 2.11 on square, the project's recorded 2.2; 1.30 on rect).  Both apply an element matrix
that was formed in double and rounded to float once (kernel 7: Ax, Ay of separable_factors; kernel 5: build_dense_element_matrix),
where the oracle and the sum-factorised kernels 1 to 4, 6, 9 and 10 (ratios 0.85 to 1.2) round after every one-dimensional
product: another rounding of the same operator.  That it is the same operator is what the fp64 column says of the one builder
that has an fp64 twin: kernel 8 runs build_dense_element_matrix<double> and sits at 4.3e-15 on shear.  A metric fault would cost
1e-1 in every output; the largest fp32 distance in the table is 3.3e-6.  This reading of the ratios is from the code, not from an
experiment.  Kernels 12 and 13 and kernel 5's element-lane form give the same bits where they share a sweep (13 = form 2 at
n_basis 4, 13 = 12 at n_basis 5), as do kernels 1 and 10.
"""
import numpy as np
import pytest

import ddh_metric_cases as mc
from ddh_metric_cases import FLOOR_FACTOR, FP64_GATE, NAMES
from test_gpu_parity import to_dev

pytestmark = pytest.mark.gpu

# kernel (or (5, sweep form)) per (n_basis, block) and precision: where KERNELS[] of ddh_resolve.cpp builds it.  9 and 10 are the
# label-built plans' (at most 256 element nodes per subdomain, 9 at n_basis 4 only).
BUILT = {
    (4, 4): {"f64": (1, 2, 3, 4, 8, 9, 10), "f32": (1, 2, 3, 4, (5, 1), (5, 2), 9, 10, 13)},
    (8, 2): {"f64": (1, 6, 10), "f32": (1, 6, 7, 10)},
    (5, 4): {"f64": (1,), "f32": (1, 12, 13)},
    (4, 8): {"f64": (1,), "f32": (1, 11)},
}
NEEDS_ONE_METRIC = {5, 7, 8, 11, 12, 13}  # refused on skew
NEEDS_DIAGONAL_METRIC = {7, 11, 12, 13}  # and kernel 5's element-lane form: refused on shear and skew
CELLS = [pytest.param(f, nb, block, id=f"{f}-nb{nb}-block{block}") for nb, block in mc.SHAPES for f in mc.cells(nb, block)]


def number(kernel):
    return kernel[0] if isinstance(kernel, tuple) else kernel


def accepted(kernel, family):
    k, form = (kernel if isinstance(kernel, tuple) else (kernel, 0))
    if family == "skew" and k in NEEDS_ONE_METRIC:
        return False
    return family in ("square", "rect") or not (k in NEEDS_DIAGONAL_METRIC or form >= 2)


def plan(cd, c, precision, kernel=0, xy=None, shape=None):
    """a DDH plan on the case's mesh (or on `xy`, numbered the same): DDH.from_labels for kernels 9 and 10"""
    k, form = (kernel if isinstance(kernel, tuple) else (kernel, 0))
    mesh = cd.Mesh2D.from_vertices(np.array(c.xy if xy is None else xy), np.array(c.elems))
    fem = cd.H1Space(mesh, cd.Basis(c.nb))
    if k in (9, 10):
        F = cd.DDH.from_labels(c.omega, np.array(c.h_a), fem, c.labels, precision=precision, kernel=k)
    else:
        F = cd.DDH(c.omega, np.array(c.h_a), fem, c.nx, c.ny, precision=precision, kernel=k, block=c.block)
    F._keep = (mesh, fem)
    if form:
        F.set_sweep_form(form)
    return F


def entry_points(torch, cuda, F, c):
    f = to_dev(torch, np.array(c.fh), cuda)
    lam = to_dev(torch, c.lam.astype(np.float64 if F.f64 else np.float32), cuda)
    b = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
    F.rhs(f, b)
    y = torch.full((F.size(),), 5.0, dtype=F.trace_dtype, device=cuda)
    F.action(lam, y)
    u = torch.full((2 * c.d.ndof,), 9.0, dtype=torch.float64, device=cuda)
    F.postprocess(lam, f, u)
    return b.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64)[c.written], u.cpu().numpy()


# ------------------------------------------------------------------ (a) parity
@pytest.mark.parametrize("family,nb,block", CELLS)
def test_every_kernel_vs_oracle(cuda, family, nb, block):
    import torch

    import cuddhelmholtz_amd as cd

    c = mc.case(family, nb, block)
    missed, ran = [], 0
    for precision in ("f64", "f32"):
        for kernel in BUILT[(nb, block)][precision]:
            if not accepted(kernel, family):
                continue
            F = plan(cd, c, precision, kernel)
            info = F.info()
            tag = f"[{c.name}, {precision}] kernel {number(kernel)}" + (f" form {kernel[1]}" if isinstance(kernel, tuple) else "")
            assert info["kernel"] == number(kernel), tag
            assert (info["nt"], info["n_domains"], info["nel1d"]) == (c.O64.t.nt, c.n_domains, 0 if number(kernel) in (9, 10) else block), tag
            assert F.size() == c.O64.size, tag
            if isinstance(kernel, tuple):
                assert F.sweep_form() == kernel[1], tag
            ran += 1
            for nm, got, ref, (fl2, fmax) in zip(NAMES, entry_points(torch, cuda, F, c), c.ref, c.floor):
                e2, emax = mc.rel(got, ref), mc.rel_max(got, ref)
                if precision == "f64":
                    print(f"{tag} {nm}: vs fp64 oracle {e2:.3e} (gate {FP64_GATE:.0e})")
                    ok = e2 <= FP64_GATE
                else:
                    print(f"{tag} {nm}: vs fp64 oracle l2 {e2:.3e}, floor {fl2:.3e}, ratio {e2 / fl2:.2f}; max {emax:.3e}, floor {fmax:.3e}, "
                          f"ratio {emax / fmax:.2f} (gate {FLOOR_FACTOR:.0f})")
                    ok = e2 <= FLOOR_FACTOR * fl2 and emax <= FLOOR_FACTOR * fmax
                if not ok:
                    missed.append((tag, nm, e2, emax))
    assert ran > 0
    assert not missed, missed


@pytest.mark.parametrize("nb,block,precision,kernel", [(4, 4, "f32", (5, 1)), (4, 4, "f32", 3), (4, 4, "f64", 8), (4, 4, "f32", 9), (8, 2, "f32", 6)],
                         ids=["nb4-f32-kernel5", "nb4-f32-kernel3", "nb4-f64-kernel8", "nb4-f32-kernel9", "nb8-f32-kernel6"])
def test_the_sign_of_g01_is_told_apart_on_the_device(cuda, nb, block, precision, kernel):
    """the shear mesh sheared the other way (g01 -> -g01, everything else bit for bit, same input vectors by index): the kernel
    follows that mesh's own reference within the gate, and lies more than 100 fp32 gates from the shear case's reference.  So
    the parity gates above do separate the two signs for what the device computes, not only for the oracle."""
    import torch

    import cuddhelmholtz_amd as cd

    s, o = mc.case("shear", nb, block), mc.opposite_shear(nb, block)
    F = plan(cd, o, precision, kernel)
    assert F.info()["kernel"] == number(kernel)
    for nm, got, own, other, (fl2, _), (sfl2, _) in zip(NAMES, entry_points(torch, cuda, F, o), o.ref, s.ref, o.floor, s.floor):
        e_own, e_other = mc.rel(got, own), mc.rel(got, other)
        gate = FP64_GATE if precision == "f64" else FLOOR_FACTOR * fl2
        print(f"[{o.name}, sheared the other way, {precision}] kernel {number(kernel)} {nm}: vs its own reference {e_own:.3e} (gate {gate:.2e}), "
              f"vs the shear case's {e_other:.3e} = {e_other / (FLOOR_FACTOR * sfl2):.0f} fp32 gates")
        assert e_own <= gate, (nm, e_own, gate)
        assert e_other >= 100 * FLOOR_FACTOR * sfl2, (nm, e_other)


# ------------------------------------------------------------------ (b) launch partitions
PARTITIONS = [("square", 8, 2, "f32", 7), ("square", 4, 4, "f64", 8),
              ("rect", 4, 4, "f32", (5, 2)), ("rect", 8, 2, "f32", 6), ("rect", 5, 4, "f32", 12), ("rect", 4, 4, "f64", 8),
              ("shear", 4, 4, "f32", (5, 1)), ("shear", 8, 2, "f64", 6), ("shear", 4, 4, "f64", 3),
              ("skew", 8, 2, "f32", 6), ("skew", 4, 4, "f32", 9), ("skew", 4, 4, "f64", 2)]


@pytest.mark.parametrize("family,nb,block,precision,kernel", PARTITIONS,
                         ids=[f"{f}-nb{nb}-block{bl}-{p}-kernel{number(k)}" for f, nb, bl, p, k in PARTITIONS])
def test_launch_partitions_are_bitwise_the_full_launch(cuda, family, nb, block, precision, kernel):
    import torch

    import cuddhelmholtz_amd as cd

    c = mc.case(family, nb, block)
    F = plan(cd, c, precision, kernel)
    nd = F.info()["n_domains"]
    assert F.info()["kernel"] == number(kernel) and nd == 6
    if isinstance(kernel, tuple):
        assert F.sweep_form() == kernel[1]
    f = to_dev(torch, np.array(c.fh), cuda)
    lam = to_dev(torch, c.lam.astype(np.float64 if F.f64 else np.float32), cuda)
    perm = np.random.default_rng(3).permutation(nd).astype(np.int32)
    for x, l in ((f, None), (None, lam), (f, lam)):
        full = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
        F.local_traces(0, nd, x, l, full)
        assert full.abs().max().item() > 0
        ranged = torch.zeros_like(full)
        F.local_traces(0, 3, x, l, ranged)
        F.local_traces(3, nd, x, l, ranged)
        assert torch.equal(ranged, full)
        listed = torch.zeros_like(full)
        for ids in (perm[:5], perm[5:]):
            F.local_traces_listed(to_dev(torch, ids, cuda), x, l, listed)
        assert torch.equal(listed, full)


# ------------------------------------------------------------------ (c) refusals and auto
def test_refusals_on_sheared_and_skewed_meshes(cuda):
    import cuddhelmholtz_amd as cd

    # (n_basis, block, precision, kernel): the plan is made on first use, and refuses there
    on_shear = ((8, 2, "f32", 7), (4, 8, "f32", 11), (5, 4, "f32", 12), (4, 4, "f32", 13), (5, 4, "f32", 13))
    on_skew = on_shear + ((4, 4, "f32", 5), (4, 4, "f64", 8))
    for family, requests in (("shear", on_shear), ("skew", on_skew)):
        for nb, block, precision, kernel in requests:
            # 16 x 8 at block 8 has no skew case: the shear case's inputs on skewed vertices (nothing is computed)
            c = mc.case(family if (nb, block) != (4, 8) else "shear", nb, block)
            F = plan(cd, c, precision, kernel, xy=mc.vertices(family, c.nx, c.ny)[0])
            with pytest.raises(RuntimeError):
                F.info()
    # the same requests are taken on the rectangles with the same numbering: it is the metric that is refused
    for nb, block, precision, kernel in on_skew:
        assert plan(cd, mc.case("rect", nb, block), precision, kernel).info()["kernel"] == kernel
    # kernel 5 on shear: one metric, so the plan exists, in the matrix form; the element-lane form needs g01 == 0
    F = plan(cd, mc.case("shear", 4, 4), "f32", 5)
    assert F.info()["kernel"] == 5 and F.sweep_form() == 1
    for form in (2, 3):
        with pytest.raises(RuntimeError):
            F.set_sweep_form(form)
    assert F.sweep_form() == 1
    F.set_sweep_form(1)
    G = plan(cd, mc.case("rect", 4, 4), "f32", 5)
    G.set_sweep_form(2)
    assert G.sweep_form() == 2


def test_auto_selection_on_the_new_meshes(cuda):
    import cuddhelmholtz_amd as cd

    # family -> (n_basis, block, precision) -> kernel
    want = {
        "shear": {(4, 4, "f32"): 5, (4, 4, "f64"): 3, (8, 2, "f32"): 6, (8, 2, "f64"): 6, (4, 8, "f32"): 1, (4, 8, "f64"): 1, (5, 4, "f32"): 1,
                  (5, 4, "f64"): 1},
        "skew": {(4, 4, "f32"): 3, (4, 4, "f64"): 3, (8, 2, "f32"): 6, (8, 2, "f64"): 6, (5, 4, "f32"): 1},
        # today's choices: 6 subdomains are fewer than kernel 12 needs under auto (64) and than the element-lane form does (8192)
        "rect": {(4, 4, "f32"): 5, (4, 4, "f64"): 3, (8, 2, "f32"): 7, (8, 2, "f64"): 6, (4, 8, "f32"): 11, (4, 8, "f64"): 1, (5, 4, "f32"): 1,
                 (5, 4, "f64"): 1},
    }
    for family, cells in want.items():
        for (nb, block, precision), kernel in cells.items():
            F = plan(cd, mc.case(family, nb, block), precision)
            got = F.info()["kernel"]
            print(f"[{family}, n_basis {nb}, block {block}, {precision}] auto takes kernel {got}, sweep form {F.sweep_form()}")
            assert got == kernel, (family, nb, block, precision, got)
            assert F.sweep_form() == (1 if kernel == 5 else 0)
