// What the lattice-sweep files share (wave_lattice.hip and the files modelled on it, fp64 and fp32): the kernel's view of a
// cuddh_wave_lattice or a cuddh_wave_box and the stencil's row ids and offset ranges.  The rows and tables are stated at the head
// of wave_lattice.hip.  What the files' launchers share is in wave_sweep_launch.hpp.
#ifndef CUDDH_AMD_WAVE_LATTICE_COMMON_HPP
#define CUDDH_AMD_WAVE_LATTICE_COMMON_HPP

#include "common.hpp"
#include "wave_stages.hpp"

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

        // The lattice vectors of one period come in through these two, rounded to R once (for R = double: as they are); padding
        // slots carry dof -1.
        constexpr int LOAD_BLOCK = 256;
        template <typename R>
        __global__ void __launch_bounds__(LOAD_BLOCK) load_kernel(int n, const int *__restrict__ dof, const double *__restrict__ x, R *__restrict__ y)
        {
            for (int i = blockIdx.x * LOAD_BLOCK + threadIdx.x; i < n; i += gridDim.x * LOAD_BLOCK)
            {
                const int g = dof[i];
                y[i] = g >= 0 ? static_cast<R>(x[g]) : R(0);
            }
        }
        template <typename R>
        __global__ void __launch_bounds__(LOAD_BLOCK) begin_kernel(int n, R filt0, const int *__restrict__ dof, const double *__restrict__ zu,
                                                                   const double *__restrict__ zv, R *__restrict__ p, R *__restrict__ q,
                                                                   R *__restrict__ u, R *__restrict__ v)
        {
            for (int i = blockIdx.x * LOAD_BLOCK + threadIdx.x; i < n; i += gridDim.x * LOAD_BLOCK)
            {
                const int g = dof[i];
                const R xe[2] = {g >= 0 ? static_cast<R>(zu[g]) : R(0), g >= 0 ? static_cast<R>(zv[g]) : R(0)};
                R ye[4];
                BeginT<R>::template apply<false>(xe, ye, &filt0);
                p[i] = ye[0];
                q[i] = ye[1];
                u[i] = ye[2];
                v[i] = ye[3];
            }
        }

        // The box sweeps' view of a cuddh_wave_box (wave_box.hip, wave_box_f32.hip): Lz planes of one lattice.
        template <typename R>
        struct BoxT
        {
            LatticeT<R> L; // one plane: Lx, Ly, stride, nb, cx, cy and the tables
            int Lz;
            R cz;
        };

        // the kernel's view of the caller's description, or false
        template <typename R>
        bool describe_box(const cuddh_wave_box *D, int stride_multiple, BoxT<R> &B)
        {
            if (!D || D->nz < 1)
                return false;
            cuddh_wave_lattice P = {};
            P.nx = D->nx;
            P.ny = D->ny;
            P.n_basis = D->n_basis;
            P.stride = D->stride;
            P.cx = D->cx;
            P.cy = D->cy;
            for (int i = 0; i < 64; ++i)
                P.A[i] = D->A[i];
            for (int i = 0; i < 8; ++i)
                P.w[i] = D->w[i];
            if (!describe(&P, stride_multiple, B.L))
                return false;
            const long long Lz = static_cast<long long>(D->nz) * (D->n_basis - 1) + 1;
            if (static_cast<long long>(B.L.stride) * B.L.Ly * Lz > 0x7fffffffLL)
                return false;
            B.Lz = static_cast<int>(Lz);
            B.cz = static_cast<R>(D->cz);
            return true;
        }
    } // namespace wave
} // namespace cuddh_k

#endif
