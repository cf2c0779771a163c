"""The inputs and the numpy restatement of the fp32 box-sweep kernel tests (TEST INFRASTRUCTURE), shared by
tests/test_wave_box_f32_host.py (which asserts on the CPU that every value is exact in float32) and
tests/test_gpu_wave_box_f32_kernels.py (which holds csrc/kernels/wave_box_f32.hip to them bit for bit).

`line`, `tables`, STAGES and the stage references are those of test_gpu_wave_lattice_kernels.py / test_gpu_wave_stage_kernels.py; the
stencil is the one of include/cuddh_hip.h (cuddh_wave_box) written with an explicit stride, rows of a multiple of four floats.
A holds integers in [-4, 4] and is not symmetric, the weights are 1 or 2, cx, cy, cz = 2, 1/2, 4, vectors hold integers in
[-8, 8], invm is 1/2, 1 or 2, Hi is 0, 1 or 2 and every coefficient is a power of two.

Lattices (nx, ny, nz, n_basis), the smallest at which a path of the kernel changes: (1,1,1,2); (3..6,1,1,2), whose Lx = 4, 5, 6, 7
give the paddings stride - Lx = 0, 3, 2, 1; (3,1,1,4), (1,3,1,4), (1,1,3,4) and (1,1,1,5): one element in a direction, where the
clamped z loads of the compile-time forms leave the node's range at both ends; (2,2,2,3), (2,1,2,5), (1,2,2,6), (2,1,1,8); tile - 1,
tile and tile + 1 nodes in each direction at n_basis 2 (at least 2 nodes, the smallest line there is), the tile read from
cuddh_hip_wave_box32_tile_x / _y / _z; one lattice of n_basis 4 with more than eight workgroups and no multiple of eight ((43,6,2,4):
2 x 2 x 7 = 28 at 128 x 16 x 1); with a tile of more than one plane, the two z-walk lattices of test_gpu_wave_box_kernels.py.
"""
import functools

import numpy as np

from test_gpu_wave_lattice_kernels import STAGES, VECTORS, line, tables

CX, CY, CZ = 2.0, 0.5, 4.0
FIXED = [(1, 1, 1, 2), (3, 1, 1, 2), (4, 1, 1, 2), (5, 1, 1, 2), (6, 1, 1, 2), (3, 1, 1, 4), (1, 3, 1, 4), (1, 1, 3, 4), (1, 1, 1, 5),
         (2, 2, 2, 3), (2, 1, 2, 5), (1, 2, 2, 6), (2, 1, 1, 8)]


def tile():
    from cuddhelmholtz_amd import _native as N

    return N.lib.cuddh_hip_wave_box32_tile_x(), N.lib.cuddh_hip_wave_box32_tile_y(), N.lib.cuddh_hip_wave_box32_tile_z()


def dims(nx, ny, nz, nb):
    """Lx, Ly, Lz and the stride: Lx rounded up to a multiple of four"""
    H = nb - 1
    Lx = nx * H + 1
    return Lx, ny * H + 1, nz * H + 1, (Lx + 3) // 4 * 4


def workgroups(lat):
    TX, TY, TZ = tile()
    Lx, Ly, Lz, stride = dims(*lat)
    return -(-stride // TX) * -(-Ly // TY) * -(-Lz // TZ)


@functools.lru_cache(maxsize=None)
def lattices():
    TX, TY, TZ = tile()
    out = list(FIXED)
    for axis, T in enumerate((TX, TY, TZ)):
        for L in sorted({max(2, T - 1), max(2, T), T + 1}):  # nodes; n_basis 2 has L = n + 1
            n = [1, 1, 1]
            n[axis] = L - 1
            out.append((*n, 2))
    # n_basis 4 (L = 3 n + 1): two tiles in x, two in y, then planes until the count is above eight and no multiple of it
    many = [TX // 3 + 1, TY // 3 + 1, 1, 4]
    while workgroups(tuple(many)) <= 8 or workgroups(tuple(many)) % 8 == 0:
        many[2] += 1
    out.append(tuple(many))
    if TZ > 1:  # a z run that ends inside a walk, and two walks (n_basis 3: an element layer is two planes)
        out += [(1, 1, max(1, (TZ + TZ // 2) // 2), 3), (1, 1, TZ + 1, 3)]
    return tuple(dict.fromkeys(out))


def stencil(nx, ny, nz, nb, stride, A, w, p):
    """K p on the padded lattice vector p (stride * Ly * Lz, float64) as include/cuddh_hip.h states it; zero in the padding columns"""
    H = nb - 1
    Lx, Ly, Lz = nx * H + 1, ny * H + 1, nz * H + 1
    assert stride >= Lx and p.shape == (stride * Ly * Lz,)
    P = p.reshape(Lz, Ly, stride)
    sx, sy, sz = (np.zeros((Lz, Ly, stride)) for _ in range(3))
    lx, ly, lz = line(nx, nb, A, w), line(ny, nb, A, w), line(nz, nb, A, w)
    for I, (terms, _) in enumerate(lx):
        for d, c in terms:
            assert 0 <= I + d < Lx
            sx[:, :, I] += c * P[:, :, I + d]
    for J, (terms, _) in enumerate(ly):
        for d, c in terms:
            assert 0 <= J + d < Ly
            sy[:, J, :Lx] += c * P[:, J + d, :Lx]
    for K, (terms, _) in enumerate(lz):
        for d, c in terms:
            assert 0 <= K + d < Lz
            sz[K, :, :Lx] += c * P[K + d, :, :Lx]
    Wx = np.zeros(stride)
    Wx[:Lx] = [wt for _, wt in lx]
    Wy, Wz = np.array([wt for _, wt in ly]), np.array([wt for _, wt in lz])
    ax = CX * (Wy[None, :, None] * Wz[:, None, None])
    ay = CY * (Wx[None, None, :] * Wz[:, None, None])
    az = CZ * (Wx[None, None, :] * Wy[None, :, None])
    Kp = ax * sx + (ay * sy + az * sz)
    Kp[:, :, Lx:] = 0
    return Kp.reshape(-1)


def host_vectors(nx, ny, nz, nb, stride, seed):
    H = nb - 1
    Lx, Ly, Lz = nx * H + 1, ny * H + 1, nz * H + 1
    rng = np.random.default_rng(seed)
    x = {name: rng.integers(-8, 9, (Lz, Ly, stride)).astype(np.float64) for name in VECTORS}
    x["invm"] = 2.0 ** rng.integers(-1, 2, (Lz, Ly, stride))
    x["Hi"] = rng.integers(0, 3, (Lz, Ly, stride)).astype(np.float64)
    for v in x.values():
        v[:, :, Lx:] = 0.0  # the padding: zero state, zero load, invm = 0
    return {name: v.reshape(-1) for name, v in x.items()}


def exact32(x, what):
    """x (float64) as float32, after asserting that nothing is lost"""
    y = np.ascontiguousarray(x, dtype=np.float64).astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x), f"{what} is not exact in float32"
    return y


@functools.lru_cache(maxsize=None)
def case(lat, stencil_input):
    """(A, w, vectors with the stencil of `stencil_input` as "w"), computed once and never changed"""
    nx, ny, nz, nb = lat
    stride = dims(*lat)[3]
    A, w = tables(nb, seed=nb)
    x = host_vectors(*lat, stride, seed=100000 * nx + 1000 * ny + 10 * nz + nb)
    x["w"] = stencil(*lat, stride, A, w, x[stencil_input])
    for v in x.values():
        v.setflags(write=False)
    return A, w, x


@functools.lru_cache(maxsize=None)
def expected(lat, name, forced):
    """the float64 restatement of stage `name` on `lat`: {output: vector}"""
    _, stencil_input, _, _, ref = STAGES[name]
    return ref(case(lat, stencil_input)[2], forced)
