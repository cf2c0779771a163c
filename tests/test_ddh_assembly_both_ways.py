"""The neighbour sums of the element-lane sweep (csrc/kernels/ddh_element_lane.hpp), restated in numpy on the lane map of
ddh_element_lane_kernel<4, ..>: lane = ex + 4 ey of a 16-lane row, four rows (subdomains) per 64-lane wavefront, z[k, l] the element's
node (k, l).  No GPU.

  * one copy forms it (assembly 1, element_assemble_xi_row_asm / element_assemble_eta_row_asm): the k == 3 column adds the k == 0
    column of lane + 1 and lane + 1 takes that sum; then the l == 3 row adds the l == 0 row of lane + 4 and lane + 4 takes it; a
    lane without the neighbour is left as it is (in xi: adds 0 times what the shift delivers);
  * both ways (assembly 2): every copy fetches the other copy's partial sum, xi first and eta on the xi results.  xi: lane -+ 1
    within the quad of four lanes that is one eta-row (a lane without the neighbour fetches itself), and the lanes with the
    neighbour add it (the others are not written).  eta: lane -+ 4 modulo 32 (a lane without the neighbour fetches from the other
    row of its 32-lane half, or from the other end of its own), and every lane adds 0 or 1 times it.

The two are the same bits on every node of 2 and 4 copies and on every other node, since a + b and b + a are one float and
fma(1, y, x) is x + y rounded once; what the foreign rows hold never reaches a result as long as it is finite."""
import numpy as np
import pytest

F = np.float32


def one_copy(z):
    """z: (64, 4, 4) float32 [lane, k, l] -> the assembled values, formed by one copy and moved to the other"""
    z = z.copy()
    lane = np.arange(64)
    ex, ey = lane & 3, (lane >> 2) & 3
    # xi: hi += mHi * (lo of lane + 1, 0 past the end of the 16-lane row); lo = that sum of lane - 1 unless ex == 0
    lo_next = np.zeros((64, 4), dtype=F)
    in_row = (lane & 15) < 15
    lo_next[in_row] = z[lane[in_row] + 1, 0, :]
    m_hi = (ex < 3).astype(F)[:, None]
    z[:, 3, :] = (z[:, 3, :] + (lo_next * m_hi).astype(F)).astype(F)
    take = ex > 0
    z[take, 0, :] = z[lane[take] - 1, 3, :]
    # eta: up += dn of lane + 4 where that lane is in the row; dn = that sum of lane - 4 where that lane is in the row
    add = ey < 3
    z[add, :, 3] = (z[add, :, 3] + z[lane[add] + 4, :, 0]).astype(F)
    take = ey > 0
    z[take, :, 0] = z[lane[take] - 4, :, 3]
    return z


def both_ways(z):
    """the same sums with every copy fetching the other's partial sum (the lane maps of FETCH_* in ddh_element_lane.hpp)"""
    z = z.copy()
    lane = np.arange(64)
    ex, ey = lane & 3, (lane >> 2) & 3
    m_d, m_u = (ey > 0).astype(F)[:, None], (ey < 3).astype(F)[:, None]
    quad = lane & ~3
    from_left, from_right = z[quad + np.maximum(ex - 1, 0), 3, :], z[quad + np.minimum(ex + 1, 3), 0, :]  # both from the values before the additions
    z[:, 0, :] = np.where((ex > 0)[:, None], (z[:, 0, :] + from_left).astype(F), z[:, 0, :])  # xi: a lane without the neighbour is not written
    z[:, 3, :] = np.where((ex < 3)[:, None], (z[:, 3, :] + from_right).astype(F), z[:, 3, :])
    half = lane & 32
    from_below, from_above = z[half + (lane - 4) % 32, :, 3], z[half + (lane + 4) % 32, :, 0]  # the xi results
    z[:, :, 0] = (z[:, :, 0] + (m_d * from_below).astype(F)).astype(F)
    z[:, :, 3] = (z[:, :, 3] + (m_u * from_above).astype(F)).astype(F)
    return z


def copies():
    """(64, 4, 4) int: how many (lane, node) pairs of the same row hold the node"""
    lane = np.arange(64)
    ex, ey = (lane & 3)[:, None, None], ((lane >> 2) & 3)[:, None, None]
    k, l = np.arange(4)[None, :, None], np.arange(4)[None, None, :]
    two_x = ((k == 0) & (ex > 0)) | ((k == 3) & (ex < 3))
    two_y = ((l == 0) & (ey > 0)) | ((l == 3) & (ey < 3))
    return (1 + two_x) * (1 + two_y)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_both_ways_is_bitwise_the_one_copy_sum(seed):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((64, 4, 4)) * 10.0 ** rng.integers(-3, 4, (64, 4, 4))).astype(F)  # magnitudes that make the sums round
    a, b = one_copy(z), both_ways(z)
    m = copies()
    assert sorted(np.unique(m)) == [1, 2, 4] and (m == 4).sum() == 64 * 4 * 9 // 16  # 9 interior corners per row, 4 copies each
    for count in (1, 2, 4):
        assert np.array_equal(bits(a[m == count]), bits(b[m == count])), count
    assert (a[m > 1] != z[m > 1]).mean() > 0.9  # the shared nodes were summed (a small addend may round away)
    assert np.array_equal(bits(a[m == 1]), bits(z[m == 1]))  # and no other node was touched
    # the copies of a node hold one value: (k == 3) of lane meets (k == 0) of lane + 1, (l == 3) of lane meets (l == 0) of lane + 4
    lane = np.arange(64)
    right, above = lane[(lane & 3) < 3], lane[((lane >> 2) & 3) < 3]
    assert np.array_equal(bits(b[right, 3, :]), bits(b[right + 1, 0, :]))
    assert np.array_equal(bits(b[above, :, 3]), bits(b[above + 4, :, 0]))


def test_the_lane_maps_are_those_the_hardware_showed():
    """ds_swizzle_b32 on lane numbers, read on an MI355X (profiles/r33): rotate by 4 within 32 lanes, quad permutations"""
    lane = np.arange(64)
    assert list(((lane & 32) + (lane + 4) % 32)[:8]) == [4, 5, 6, 7, 8, 9, 10, 11] and list(((lane & 32) + (lane + 4) % 32)[28:36]) == [0, 1, 2, 3, 36, 37, 38, 39]
    assert list(((lane & 32) + (lane - 4) % 32)[:8]) == [28, 29, 30, 31, 0, 1, 2, 3]
    assert list(((lane & ~3) + np.minimum((lane & 3) + 1, 3))[:8]) == [1, 2, 3, 3, 5, 6, 7, 7]
    assert list(((lane & ~3) + np.maximum((lane & 3) - 1, 0))[:8]) == [0, 0, 1, 2, 4, 4, 5, 6]


def test_what_a_fetch_out_of_the_row_returns_never_reaches_a_result():
    rng = np.random.default_rng(5)
    z = rng.standard_normal((64, 4, 4)).astype(F)
    plain = both_ways(z)
    for row in range(4):
        other = z.copy()
        foreign = np.ones(64, dtype=bool)
        foreign[16 * row:16 * row + 16] = False
        # arbitrary finite values in the three other rows, from the smallest floats to the largest whose four-copy sums stay finite
        # (a row that overflows is a subdomain that has diverged: 0 times its infinity is the one thing that would get through)
        other[foreign] = rng.choice(np.array([5e37, -5e37, 1e-45, -1e-45, 1.0, -7.5e20], dtype=F), (48, 4, 4))
        got = both_ways(other)
        assert np.isfinite(got).all()
        assert np.array_equal(bits(got[~foreign]), bits(plain[~foreign])), row
        assert np.array_equal(bits(got[~foreign]), bits(one_copy(other)[~foreign])), row


def test_a_row_that_repeats_another_as_the_padding_rows_do():
    """a launch whose length is no multiple of 4 recomputes the wavefront's first subdomain in the missing rows"""
    rng = np.random.default_rng(9)
    z = rng.standard_normal((64, 4, 4)).astype(F)
    z[32:48] = z[:16]
    z[48:] = z[:16]
    a, b = one_copy(z), both_ways(z)
    assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(b[32:48]), bits(b[:16])) and np.array_equal(bits(b[48:]), bits(b[:16]))
