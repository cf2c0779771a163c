// The lattice of a box of nx x ny x nz congruent brick elements, for the box sweeps of the three-dimensional whole-domain
// WaveHoltz solver (waveholtz_box.hpp, csrc/kernels/wave_box.hip).  Plain host code: nothing here touches the device.
//
// The box is described by the caller, not detected: there is no 3-D mesh class.  With H = n_basis - 1 the lattice has
// Lx x Ly x Lz Gauss-Lobatto nodes, L = n H + 1; node (I, J, K) is collocation point (I % H, J % H, K % H) of element
// (I / H, J / H, K / H) (the last node of a line belongs to the last element) and has the public index I + Lx (J + Ly K).
#ifndef CUDDH_AMD_WAVE_BOX_HPP
#define CUDDH_AMD_WAVE_BOX_HPP

#include <vector>

#include "cuddh_hip.h"

namespace cuddh
{
    struct WaveBox
    {
        enum Face : unsigned
        {
            x0 = 1,
            x1 = 2,
            y0 = 4,
            y1 = 8,
            z0 = 16,
            z1 = 32,
            all_faces = 63
        };

        cuddh_wave_box desc = {}; // what the kernels take: counts, stride (Lx rounded up to the row multiple), cx, cy, cz and the 1-D tables
        int Lx = 0, Ly = 0, Lz = 0;
        double hx = 0.0, hy = 0.0, hz = 0.0;
        // in public (unpadded lattice) order, Lx Ly Lz each: the lumped mass, the lumped mass of the absorbing faces,
        // 1 / (a^2 m) and h a
        std::vector<double> m, h, invm, Hi;
        // padded slot I + stride (J + Ly K) -> public index (-1: padding), and back
        std::vector<int> dof_of_slot, slot_of_dof;

        int nodes() const { return Lx * Ly * Lz; }
        int slots() const { return desc.stride * Ly * Lz; }
    };

    /// What build_wave_box refuses, checked without allocating anything: a count < 1, an empty or inverted interval (or one that is
    /// not finite), n_basis outside [2, 8], a face mask outside 6 bits, stride Ly Lz beyond an int, a coefficient that is not finite
    /// and positive.  box = {ax, bx, ay, by, az, bz}; h_a: Lx Ly Lz values in public order, or null for a == 1.  Refusals go through
    /// cuddh_error with a message that starts "WaveHoltz error: box:".  Returns min a.
    /// row_multiple: rows hold a multiple of this many elements, 2 (the fp64 sweeps: wave_box.hip) or 4 (the fp32 sweeps:
    /// wave_box_f32.hip); anything else is refused, and stride is Lx rounded up to it.
    double check_wave_box(int nx, int ny, int nz, const double *box, int n_basis, const double *h_a, unsigned face_mask, int row_multiple = 2);

    /// the whole description (check_wave_box first)
    WaveBox build_wave_box(int nx, int ny, int nz, const double *box, int n_basis, const double *h_a, unsigned face_mask, int row_multiple = 2);
} // namespace cuddh

#endif
