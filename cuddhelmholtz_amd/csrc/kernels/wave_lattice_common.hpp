// What the two lattice-sweep files share (wave_lattice.hip: fp64; wave_lattice_f32.hip: fp32): the kernel's view of a
// cuddh_wave_lattice and the stencil's row ids and offset ranges.  The rows and tables are stated at the head of wave_lattice.hip.
#ifndef CUDDH_AMD_WAVE_LATTICE_COMMON_HPP
#define CUDDH_AMD_WAVE_LATTICE_COMMON_HPP

#include "common.hpp"

namespace cuddh_k
{
    namespace wave
    {
        constexpr int NB_MAX = 8, N_XCD = 8;

        template <typename R>
        struct LatticeT
        {
            int Lx, Ly, stride, nb;
            R cx, cy;
            R T[(NB_MAX + 1) * 2 * NB_MAX]; // row r at r * 2 nb, offset d at d + H
            R Wt[NB_MAX + 1];
        };

        __device__ inline int row_id(int i, int L, int nb) { return i == 0 ? nb - 1 : (i == L - 1 ? nb : i % (nb - 1)); }
        __device__ inline int first_offset(int r, int nb) { return (r == 0 || r == nb) ? -(nb - 1) : (r == nb - 1 ? 0 : -r); }
        __device__ inline int last_offset(int r, int nb) { return (r == 0 || r == nb - 1) ? nb - 1 : (r == nb ? 0 : nb - 1 - r); }

        // The kernel's view of the caller's description, or false.  Rows hold a multiple of `stride_multiple` elements.  Every
        // table entry is formed in double (T[0][0] = A[H][H] + A[0][0] and Wt[0] = w[H] + w[0] are sums) and then rounded to R
        // once: for R = double that is the entry itself.
        template <typename R>
        bool describe(const cuddh_wave_lattice *D, int stride_multiple, LatticeT<R> &L)
        {
            if (!D || D->nx < 1 || D->ny < 1 || D->n_basis < 2 || D->n_basis > NB_MAX)
                return false;
            const int nb = D->n_basis, H = nb - 1;
            const long long Lx = static_cast<long long>(D->nx) * H + 1, Ly = static_cast<long long>(D->ny) * H + 1;
            if (D->stride < Lx || D->stride % stride_multiple != 0 || D->stride * Ly > 0x7fffffffLL)
                return false;
            L = {};
            L.Lx = static_cast<int>(Lx);
            L.Ly = static_cast<int>(Ly);
            L.stride = D->stride;
            L.nb = nb;
            L.cx = static_cast<R>(D->cx);
            L.cy = static_cast<R>(D->cy);
            const double *A = D->A, *w = D->w;
            const int WP = 2 * nb;
            auto T = [&](int r, int d) -> R & { return L.T[r * WP + d + H]; };
            for (int d = -H; d <= H; ++d)
            {
                T(0, d) = static_cast<R>(d < 0 ? A[H * nb + H + d] : (d == 0 ? A[H * nb + H] + A[0] : A[d]));
                if (d >= 0)
                    T(H, d) = static_cast<R>(A[d]);
                if (d <= 0)
                    T(H + 1, d) = static_cast<R>(A[H * nb + H + d]);
            }
            for (int k = 1; k < H; ++k)
                for (int d = -k; d <= H - k; ++d)
                    T(k, d) = static_cast<R>(A[k * nb + k + d]);
            L.Wt[0] = static_cast<R>(w[H] + w[0]);
            for (int k = 1; k < H; ++k)
                L.Wt[k] = static_cast<R>(w[k]);
            L.Wt[H] = static_cast<R>(w[0]);
            L.Wt[H + 1] = static_cast<R>(w[H]);
            return true;
        }
    } // namespace wave
} // namespace cuddh_k

#endif
