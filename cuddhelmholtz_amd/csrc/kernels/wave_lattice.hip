// Lattice sweeps of the whole-domain WaveHoltz march (csrc/src/waveholtz.cpp): on a uniform rectangle mesh the
// collocated (Gauss-Lobatto) stiffness is a Kronecker sum on the global lattice of Lx x Ly Gauss-Lobatto nodes,
//   K = cx diag(Wy) (x) Ax  +  cy Ay (x) diag(Wx),      cx = hy / hx,  cy = hx / hy,      node (I, J) at I + stride J,
// Ax, Ay the 1-D element matrix A (n_basis x n_basis, row-major) assembled along a row of nx / ny elements that overlap in one
// node, Wx, Wy the weights w assembled the same way.  A node therefore computes its own (K p)(I, J) from at most 2 (n_basis - 1)
// neighbours to each side, and ONE launch does a whole Runge-Kutta sweep: the stencil, then the stage of wave_stages.hpp with
// x[0] computed instead of loaded.  No element phase, no assembly, no atomics.
//
// The stencil.  H = n_basis - 1, k = I mod H.  A node gets a row id r and a range of offsets d:
//   r = 0         element boundary (k = 0, 0 < I < Lx - 1):  d in [-H, H],      T[0][d] = A[H][H + d] (d < 0), A[H][H] + A[0][0] (d = 0), A[0][d] (d > 0)
//   r = k         element interior (0 < k < H):               d in [-k, H - k],  T[k][d] = A[k][k + d]
//   r = H         I = 0 (only the element to the right):      d in [0, H],       T[H][d] = A[0][d]
//   r = H + 1     I = Lx - 1 (only the element to the left):  d in [-H, 0],      T[H + 1][d] = A[H][H + d]
// and the weight Wt[r] = w[H] + w[0], w[k], w[0], w[H].  With rx = r(I), ry = r(J):
//   sx = sum_d T[rx][d] p(I + d, J),   sy = sum_d T[ry][d] p(I, J + d),   each from zero, d ascending over the node's range, by fma;
//   (K p)(I, J) = fma(cx Wt[ry], sx, (cy Wt[rx]) sy).
// The order depends on nothing but (I, J): results are bitwise reproducible.  Offsets outside a node's range are not read.
//
// Layout.  Rows have `stride` >= Lx doubles, stride even, so that every row starts on a 16-byte boundary; the columns from Lx on
// are padding that must hold zero state, zero load and invm = 0 (the march keeps them zero).  The stencil never reads them: a tile
// takes p(I, J) for 0 <= I < Lx, 0 <= J < Ly only, and zero elsewhere.
//
// Decomposition.  A workgroup of four wavefronts owns a tile of TX x TY nodes.  It stages the stencil input of the tile and its
// halo of H rows and columns in LDS (8-byte loads, cached: the halo is some other tile's interior), then every wavefront takes
// rows of the tile, a lane two neighbouring columns, so that the pointwise streams are waveholtz.hip's: one 16-byte load and
// one 16-byte store per stream, two rows in flight, non-temporal from 64 MB per vector.  In rk2_a and rk4_1 the stencil input
// is also the stage's p: it is taken from the tile, not read again.  Workgroup ids are renumbered so that each XCD (ids are dealt
// round robin over eight) gets a contiguous run of tiles, whose halos then meet in that XCD's L2.
// n_basis 4 and 5 are compile-time; every other n_basis in [2, 8] shares an instantiation with loops of run-time length over
// LDS (no register arrays, hence no scratch).
// The host side below is the family's launcher only (description, extra argument, grid, compile-time n_basis list); the stage
// arguments and their refusals, the dispatch and the six wirings of the entry points are wave_sweep_launch.hpp's.
#include "wave_lattice_common.hpp"
#include "wave_sweep_launch.hpp"

#include "cuddh_hip.h"

using namespace cuddh_k;
using namespace cuddh_k::wave;

namespace
{
    constexpr int BLOCK = 256, WAVES = BLOCK / WAVE;
#ifndef CUDDH_WAVE_LATTICE_TY
#define CUDDH_WAVE_LATTICE_TY 16 // (a define, for A/B builds with profiles/tools/build_variant.py: 8 and 32 were measured)
#endif
    constexpr int TX = 128, TY = CUDDH_WAVE_LATTICE_TY; // nodes per tile; TX = 2 columns per lane
    constexpr int ROWS_PER_WAVE = TY / WAVES, UNROLL = 2;
    static_assert(TX == 2 * WAVE && ROWS_PER_WAVE % UNROLL == 0, "a lane owns two columns; rows go in pairs");

    using Lattice = LatticeT<double>; // (wave_lattice_common.hpp, with the stencil's row ids and offset ranges)

    // PSLOT > 0: input PSLOT of the stage is the stencil input itself
    template <typename Stage, int PSLOT, bool FORCED, bool NT, int NBT>
    __global__ void __launch_bounds__(BLOCK) lattice_kernel(Lattice L, StageArgs a)
    {
        constexpr int NIN = Stage::NIN + (FORCED ? 2 : 0), NOUT = Stage::NOUT;
        static_assert(NIN <= MAX_IN && NOUT <= MAX_OUT, "StageArgs holds every stage");
        constexpr int HM = (NBT ? NBT : NB_MAX) - 1, HP = (HM + 1) & ~1; // halo; the tile's first column sits at LDS column HP (even)
        constexpr int LW = TX + 2 * HP;
        __shared__ __attribute__((aligned(16))) double tile[(TY + 2 * HM) * LW];
        __shared__ __attribute__((aligned(16))) double sT[(NB_MAX + 1) * 2 * NB_MAX];
        __shared__ double sWt[NB_MAX + 1];

        const int nb = NBT ? NBT : L.nb, H = nb - 1, WP = 2 * nb;
        const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;

        // this workgroup's tile: XCD x gets the x-th contiguous run of tiles
        const int ntx = (L.stride + TX - 1) / TX, n_tiles = gridDim.x;
        const int xcd = blockIdx.x % N_XCD, slot = blockIdx.x / N_XCD;
        const int t = xcd * (n_tiles / N_XCD) + min(xcd, n_tiles % N_XCD) + slot;
        const int tx0 = (t % ntx) * TX, ty0 = (t / ntx) * TY;

        for (int i = tid; i < (nb + 1) * WP; i += BLOCK)
            sT[i] = L.T[i];
        if (tid <= nb)
            sWt[tid] = L.Wt[tid];
        const double *__restrict__ pin = a.in[0];
        for (int i = tid; i < (TY + 2 * H) * LW; i += BLOCK)
        {
            const int jl = i / LW, il = i - jl * LW;
            const int I = tx0 - HP + il, J = ty0 - H + jl;
            tile[i] = (I >= 0 && I < L.Lx && J >= 0 && J < L.Ly) ? pin[J * L.stride + I] : 0.0;
        }
        __syncthreads();

        // what a lane's two columns need in every row
        const int I0 = tx0 + 2 * lane;
        int rx[2], lox[2], hix[2];
        double wx[2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
        {
            const bool valid = I0 + c < L.Lx;
            rx[c] = valid ? row_id(I0 + c, L.Lx, nb) : 0;
            lox[c] = valid ? first_offset(rx[c], nb) : 1;
            hix[c] = valid ? last_offset(rx[c], nb) : 0;
            wx[c] = valid ? L.cy * sWt[rx[c]] : 0.0;
        }
        const int ctr = HP + 2 * lane; // LDS column of I0

        for (int m0 = 0; m0 < ROWS_PER_WAVE; m0 += UNROLL)
        {
            V2 x[UNROLL][NIN];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                // clamped, not guarded (blas1.hip, map_kernel)
                const int J = min(ty0 + wv + WAVES * (m0 + u), L.Ly - 1), I = min(I0, L.stride - 2);
                const int i = (J * L.stride + I) / 2;
#pragma unroll
                for (int s = 1; s < NIN; ++s)
                    if (s != PSLOT)
                        x[u][s] = stream_load<NT>(reinterpret_cast<const V2 *>(a.in[s]) + i);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                const int jt = wv + WAVES * (m0 + u), J = ty0 + jt;
                if (J < L.Ly && I0 < L.stride)
                {
                    const int ry = row_id(J, L.Ly, nb), loy = first_offset(ry, nb), hiy = last_offset(ry, nb);
                    const double wy = L.cx * sWt[ry];
                    const double *row = tile + (jt + H) * LW + ctr;
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                    {
                        double sx = 0.0, sy = 0.0;
#pragma unroll
                        for (int d = -HM; d <= HM; ++d)
                            if (d >= lox[c] && d <= hix[c])
                                sx = fmadd(sT[rx[c] * WP + d + H], row[c + d], sx);
#pragma unroll
                        for (int d = -HM; d <= HM; ++d)
                            if (d >= loy && d <= hiy)
                                sy = fmadd(sT[ry * WP + d + H], row[c + d * LW], sy);
                        x[u][0][c] = fmadd(wy, sx, wx[c] * sy);
                        if constexpr (PSLOT > 0)
                            x[u][PSLOT][c] = row[c];
                    }
                    V2 y[NOUT];
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                    {
                        double xe[NIN], ye[NOUT];
#pragma unroll
                        for (int s = 0; s < NIN; ++s)
                            xe[s] = x[u][s][c];
                        Stage::template apply<FORCED>(xe, ye, a.coef);
#pragma unroll
                        for (int s = 0; s < NOUT; ++s)
                            y[s][c] = ye[s];
                    }
                    const int i = (J * L.stride + I0) / 2;
#pragma unroll
                    for (int s = 0; s < NOUT; ++s)
                        stream_store<NT>(reinterpret_cast<V2 *>(a.out[s]) + i, y[s]);
                }
            }
        }
    }

    // the family's launcher (wave_sweep_launch.hpp): one sweep on the entry points' leading arguments
    struct launch_lattice
    {
        const cuddh_wave_lattice *D;
        void *stream;

        template <typename Stage, int PSLOT>
        int sweep(const double *const (&in)[Stage::NIN], const double *F, const double *G, double *const (&out)[Stage::NOUT],
                  const double (&coef)[MAX_COEF]) const
        {
            Lattice L;
            StageArgs a;
            if (!describe(D, 2, L) || !stage_args<Stage>(in, F, G, out, coef, a))
                return invalid_value;
            const int grid = ((L.stride + TX - 1) / TX) * ((L.Ly + TY - 1) / TY);
            dispatch_sweep(L.nb, NBasis<4, 5>{}, F != nullptr, static_cast<long long>(L.stride) * L.Ly * sizeof(double),
                           [&](auto forced_c, auto nt_c, auto nbt)
                           { hipLaunchKernelGGL((lattice_kernel<Stage, PSLOT, decltype(forced_c)::value, decltype(nt_c)::value, decltype(nbt)::value>),
                                                dim3(grid), dim3(BLOCK), 0, as_stream(stream), L, a); });
            return launch_status();
        }
    };
} // namespace

extern "C"
{
    int cuddh_hip_wave_lattice_tile_x(void) { return TX; }
    int cuddh_hip_wave_lattice_tile_y(void) { return TY; }

    int cuddh_hip_wave_lattice_gather_f64(int n, const int *dof_of_slot, const double *x, double *y, void *stream)
    {
        if (n <= 0)
            return 0;
        hipLaunchKernelGGL(load_kernel<double>, dim3(stream_grid(n, LOAD_BLOCK)), dim3(LOAD_BLOCK), 0, as_stream(stream), n, dof_of_slot, x, y);
        return launch_status();
    }

    int cuddh_hip_wave_lattice_begin_f64(int n, double filt0, const int *dof_of_slot, const double *zu, const double *zv, double *p, double *q,
                                         double *u, double *v, void *stream)
    {
        if (n <= 0)
            return 0;
        hipLaunchKernelGGL(begin_kernel<double>, dim3(stream_grid(n, LOAD_BLOCK)), dim3(LOAD_BLOCK), 0, as_stream(stream), n, filt0, dof_of_slot, zu, zv, p, q, u, v);
        return launch_status();
    }

    int cuddh_hip_wave_lattice_rk2_a_f64(const cuddh_wave_lattice *lattice, double half_dt, double c, double s, const double *p, const double *q,
                                         const double *invm, const double *Hi, const double *F, const double *G, double *qh, double *ph,
                                         void *stream)
    {
        return rk2_a(launch_lattice{lattice, stream}, half_dt, c, s, p, q, invm, Hi, F, G, qh, ph);
    }

    int cuddh_hip_wave_lattice_rk2_b_f64(const cuddh_wave_lattice *lattice, double dt, double c, double s, double filt, const double *ph,
                                         const double *qh, const double *invm, const double *Hi, const double *F, const double *G, double *p,
                                         double *q, double *u, double *v, void *stream)
    {
        return rk2_b(launch_lattice{lattice, stream}, dt, c, s, filt, ph, qh, invm, Hi, F, G, p, q, u, v);
    }

    int cuddh_hip_wave_lattice_rk4_1_f64(const cuddh_wave_lattice *lattice, double half_dt, double c, double s, const double *p, const double *q,
                                         const double *invm, const double *Hi, const double *F, const double *G, double *ps, double *qs,
                                         double *aq, double *ap, void *stream)
    {
        return rk4_1(launch_lattice{lattice, stream}, half_dt, c, s, p, q, invm, Hi, F, G, ps, qs, aq, ap);
    }

    int cuddh_hip_wave_lattice_rk4_2_f64(const cuddh_wave_lattice *lattice, double half_dt, double c, double s, const double *ps_in,
                                         const double *p, const double *q, const double *invm, const double *Hi, const double *F,
                                         const double *G, double *ps_out, double *qs, double *aq, double *ap, void *stream)
    {
        return rk4_2(launch_lattice{lattice, stream}, half_dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
    }

    int cuddh_hip_wave_lattice_rk4_3_f64(const cuddh_wave_lattice *lattice, double dt, double c, double s, const double *ps_in, const double *p,
                                         const double *q, const double *invm, const double *Hi, const double *F, const double *G,
                                         double *ps_out, double *qs, double *aq, double *ap, void *stream)
    {
        return rk4_3(launch_lattice{lattice, stream}, dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
    }

    int cuddh_hip_wave_lattice_rk4_4_f64(const cuddh_wave_lattice *lattice, double sixth_dt, double c, double s, double filt, const double *ps,
                                         const double *qs, const double *aq, const double *ap, const double *invm, const double *Hi,
                                         const double *F, const double *G, double *p, double *q, double *u, double *v, void *stream)
    {
        return rk4_4(launch_lattice{lattice, stream}, sixth_dt, c, s, filt, ps, qs, aq, ap, invm, Hi, F, G, p, q, u, v);
    }
}
