// Paired lattice sweeps of the whole-domain WaveHoltz march (csrc/src/waveholtz.cpp, launch = per_pair): two
// consecutive sweeps of wave_lattice.hip in ONE launch.  The second sweep's stencil input is pointwise in vectors that exist
// before the first sweep (wave_pair_stages.hpp), so the halo stays H = n_basis - 1, nothing is recomputed and no grid barrier is
// needed: a workgroup stages TWO tiles with halo in LDS, tile 1 stored and tile 2 = fma(-h, q', p') formed while staging (zero
// outside 0 <= I < Lx, 0 <= J < Ly, like tile 1), takes the stencil of wave_lattice.hip from each (the same rows, offset ranges
// and order of fused multiply-adds) and runs the two stages back to back with the first one's outputs in registers.
//   rk2      tiles p and ph = fma(-dt/2, q, p);       Rk2A then Rk2B;        writes p_out q_out u v
//   rk4_12   tiles p and ps1 = fma(-dt/2, q, p);      Rk4First then Rk4Mid;  writes ps2 qs aq ap
//   rk4_34   tiles ps2 and ps3 = fma(-dt, qs, p);     Rk4Mid then Rk4Last;   writes p_out q u v
// A vector read with a halo is still needed by a neighbouring workgroup: it is never an output of the same launch.
//
// The frame is wave_lattice.hip's: rows of `stride` doubles (even), four wavefronts on a tile of TX x TY nodes, a lane two
// neighbouring columns, 16-byte pointwise streams (clamped, not guarded), two rows in flight, non-temporal from 64 MB per vector
// (the streams that were just staged are read through the cache), workgroup ids renumbered so that an XCD gets a contiguous
// run of tiles.  n_basis 4 and 5 are compile-time on tiles of 128 x 16; every other n_basis in [2, 8] shares an instantiation
// with loops over LDS only and a halo of 7, on tiles of 128 x 8 so that its two tiles stay below 64 KB of LDS.
// The launcher's arguments and refusals are pair_args (wave_pair_stages.hpp); its dispatch of n_basis, forced and streaming to an
// instantiation is dispatch_sweep (wave_sweep_launch.hpp).
#include "cuddh_hip.h"

#include "wave_pair_stages.hpp"

using namespace cuddh_k;
using namespace cuddh_k::wave;

namespace
{
    constexpr int BLOCK = 256, WAVES = BLOCK / WAVE;
    constexpr int TX = 128, TY = 16, TY_RUN_TIME = 8; // nodes per tile; TX = 2 columns per lane
    constexpr int UNROLL = 2;
    static_assert(TX == 2 * WAVE && (TY / WAVES) % UNROLL == 0 && (TY_RUN_TIME / WAVES) % UNROLL == 0, "a lane owns two columns; rows go in pairs");

    using Lattice = LatticeT<double>;
    using PairArgs = PairArgsT<double>;

    constexpr int tile_y(int nbt) { return nbt ? TY : TY_RUN_TIME; }

    template <typename Kind, bool FORCED, bool NT, int NBT>
    __global__ void __launch_bounds__(BLOCK) pair_kernel(Lattice L, PairArgs a)
    {
        constexpr int NIN = Kind::NIN + (FORCED ? 2 : 0), NOUT = Kind::NOUT;
        constexpr int TYK = tile_y(NBT), ROWS_PER_WAVE = TYK / WAVES;
        constexpr int HM = (NBT ? NBT : NB_MAX) - 1, HP = (HM + 1) & ~1; // halo; the tile's first column sits at LDS column HP (even)
        constexpr int LW = TX + 2 * HP, TILE = (TYK + 2 * HM) * LW;
        static_assert(2 * TILE * sizeof(double) + 2048 <= 65536, "the two tiles and the tables stay within 64 KB");
        __shared__ __attribute__((aligned(16))) double tile[2 * TILE];
        __shared__ __attribute__((aligned(16))) double sT[(NB_MAX + 1) * 2 * NB_MAX];
        __shared__ double sWt[NB_MAX + 1];

        const int nb = NBT ? NBT : L.nb, H = nb - 1, WP = 2 * nb;
        const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;

        // this workgroup's tile: XCD x gets the x-th contiguous run of tiles
        const int ntx = (L.stride + TX - 1) / TX, n_tiles = gridDim.x;
        const int xcd = blockIdx.x % N_XCD, slot = blockIdx.x / N_XCD;
        const int t = xcd * (n_tiles / N_XCD) + min(xcd, n_tiles % N_XCD) + slot;
        const int tx0 = (t % ntx) * TX, ty0 = (t / ntx) * TYK;

        for (int i = tid; i < (nb + 1) * WP; i += BLOCK)
            sT[i] = L.T[i];
        if (tid <= nb)
            sWt[tid] = L.Wt[tid];
        const double *__restrict__ h0 = a.halo[0], *__restrict__ h1 = a.halo[1], *__restrict__ h2 = a.halo[2];
        const double mh = -a.coef[0];
        for (int i = tid; i < (TYK + 2 * H) * LW; i += BLOCK)
        {
            const int jl = i / LW, il = i - jl * LW;
            const int I = tx0 - HP + il, J = ty0 - H + jl;
            double t1 = 0.0, t2 = 0.0;
            if (I >= 0 && I < L.Lx && J >= 0 && J < L.Ly)
            {
                const int g = J * L.stride + I;
                t1 = h0[g];
                t2 = fmadd(mh, h2[g], Kind::P_IS_TILE ? t1 : h1[g]);
            }
            tile[i] = t1;
            tile[TILE + i] = t2;
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
                for (int s = 0; s < NIN; ++s)
                    x[u][s] = Kind::halo_stream(s) ? stream_load<false>(reinterpret_cast<const V2 *>(a.in[s]) + i)
                                                   : stream_load<NT>(reinterpret_cast<const V2 *>(a.in[s]) + i);
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
                    V2 y[NOUT];
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                    {
                        double w[2];
#pragma unroll
                        for (int k = 0; k < 2; ++k)
                        {
                            const double *r = row + k * TILE;
                            double sx = 0.0, sy = 0.0;
#pragma unroll
                            for (int d = -HM; d <= HM; ++d)
                                if (d >= lox[c] && d <= hix[c])
                                    sx = fmadd(sT[rx[c] * WP + d + H], r[c + d], sx);
#pragma unroll
                            for (int d = -HM; d <= HM; ++d)
                                if (d >= loy && d <= hiy)
                                    sy = fmadd(sT[ry * WP + d + H], r[c + d * LW], sy);
                            w[k] = fmadd(wy, sx, wx[c] * sy);
                        }
                        double se[NIN], ye[NOUT];
#pragma unroll
                        for (int s = 0; s < NIN; ++s)
                            se[s] = x[u][s][c];
                        Kind::template apply<FORCED>(w[0], w[1], row[c], se, ye, a.coef);
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

    template <typename Kind, int NCOEF>
    int launch_pair(const cuddh_wave_lattice *D, const double *const (&halo)[PAIR_HALO], const double *const (&in)[Kind::NIN], const double *F,
                    const double *G, double *const (&out)[Kind::NOUT], const double (&coef)[NCOEF], void *stream)
    {
        Lattice L;
        PairArgs a;
        if (!pair_args<double, Kind>(D, 2, halo, in, F, G, out, coef, L, a))
            return invalid_value;
        dispatch_sweep(L.nb, NBasis<4, 5>{}, F != nullptr, static_cast<long long>(L.stride) * L.Ly * sizeof(double),
                       [&](auto forced_c, auto nt_c, auto nbt)
                       {
                           constexpr int ty = tile_y(decltype(nbt)::value);
                           const int grid = ((L.stride + TX - 1) / TX) * ((L.Ly + ty - 1) / ty);
                           hipLaunchKernelGGL((pair_kernel<Kind, decltype(forced_c)::value, decltype(nt_c)::value, decltype(nbt)::value>), dim3(grid),
                                              dim3(BLOCK), 0, as_stream(stream), L, a);
                       });
        return launch_status();
    }
} // namespace

extern "C"
{
    int cuddh_hip_wave_pair_tile_x(void) { return TX; }
    int cuddh_hip_wave_pair_tile_y(void) { return TY; }
    int cuddh_hip_wave_pair_tile_y_run_time(void) { return TY_RUN_TIME; }

    int cuddh_hip_wave_pair_rk2_f64(const cuddh_wave_lattice *lattice, double half_dt, double dt, double c0, double s0, double c1, double s1,
                                    double filt, const double *p, const double *q, const double *invm, const double *Hi, const double *F,
                                    const double *G, double *p_out, double *q_out, double *u, double *v, void *stream)
    {
        return launch_pair<PairRk2T<double>>(lattice, {p, p, q}, {q, u, v, invm, Hi}, F, G, {p_out, q_out, u, v},
                                             {half_dt, dt, c0, s0, c1, s1, filt}, stream);
    }

    int cuddh_hip_wave_pair_rk4_12_f64(const cuddh_wave_lattice *lattice, double half_dt, double c0, double s0, double c1, double s1,
                                       const double *p, const double *q, const double *invm, const double *Hi, const double *F, const double *G,
                                       double *ps2, double *qs, double *aq, double *ap, void *stream)
    {
        return launch_pair<PairRk4_12T<double>>(lattice, {p, p, q}, {q, invm, Hi}, F, G, {ps2, qs, aq, ap}, {half_dt, c0, s0, c1, s1}, stream);
    }

    int cuddh_hip_wave_pair_rk4_34_f64(const cuddh_wave_lattice *lattice, double dt, double sixth_dt, double c1, double s1, double c2, double s2,
                                       double filt, const double *ps2, const double *p, const double *qs, const double *aq, const double *ap,
                                       const double *invm, const double *Hi, const double *F, const double *G, double *p_out, double *q,
                                       double *u, double *v, void *stream)
    {
        return launch_pair<PairRk4_34T<double>>(lattice, {ps2, p, qs}, {p, q, qs, aq, ap, u, v, invm, Hi}, F, G, {p_out, q, u, v},
                                                {dt, sixth_dt, c1, s1, c2, s2, filt}, stream);
    }
}
