// The paired lattice sweeps of wave_pair.hip with state, stencil and stages stored and computed in fp32: two
// consecutive sweeps of wave_lattice_f32.hip in one launch, bit for bit what those two launches give.  The description is the
// fp64 one; the host rounds every table entry, cx, cy and every scalar of the call to float once, the scalars the march forms
// today (dt / 2, dt / 6) each as its own argument.
//
// The frame is wave_lattice_f32.hip's: rows of `stride` floats (a multiple of 4), a tile of TX x TY = 128 x 16 nodes in every
// instantiation, both tiles staged as aligned 16-byte pieces (tile 2 = fmaf(-h, q', p') piece by piece, masked like tile 1), a
// lane four neighbouring columns, 32 lanes a row, a wavefront two rows per pass and two passes, all of a lane's stream requests
// (clamped, not guarded) issued before its first store, non-temporal from 64 MB per vector (the streams that were just staged
// are read through the cache).  The x-window of a lane's four columns is read as aligned 16-byte pieces, the y-window as one
// 16-byte piece per offset, from each tile in turn.
// The launcher's arguments and refusals are pair_args (wave_pair_stages.hpp); its dispatch of n_basis, forced and streaming to an
// instantiation is dispatch_sweep (wave_sweep_launch.hpp).
#include "cuddh_hip.h"

#include "wave_pair_stages.hpp"

using namespace cuddh_k;
using namespace cuddh_k::wave;

namespace
{
    constexpr int BLOCK = 256, WAVES = BLOCK / WAVE;
    constexpr int COLS = 4;                                       // columns per lane: one 16-byte access per stream
    constexpr int TX = 128, TY = 16;                              // nodes per tile
    constexpr int ROW_LANES = TX / COLS, ROWS = WAVE / ROW_LANES; // lanes per row; rows per wavefront pass
    constexpr int PASSES = TY / (WAVES * ROWS);
    static_assert(ROW_LANES * ROWS == WAVE && PASSES * WAVES * ROWS == TY, "a wavefront pass covers whole rows; the passes cover the tile");

    using V4 = float __attribute__((ext_vector_type(4)));
    using Lattice32 = LatticeT<float>;
    using PairArgs32 = PairArgsT<float>;

    template <typename Kind, bool FORCED, bool NT, int NBT>
    __global__ void __launch_bounds__(BLOCK) pair32_kernel(Lattice32 L, PairArgs32 a)
    {
        constexpr int NIN = Kind::NIN + (FORCED ? 2 : 0), NOUT = Kind::NOUT;
        constexpr int HM = (NBT ? NBT : NB_MAX) - 1, HP = (HM + COLS - 1) & ~(COLS - 1); // halo; the tile's first column sits at LDS column HP
        constexpr int LW = TX + 2 * HP, LG = LW / COLS, TILE = (TY + 2 * HM) * LW;
        static_assert(2 * TILE * sizeof(float) + 1024 <= 65536, "the two tiles and the tables stay within 64 KB");
        __shared__ __attribute__((aligned(16))) float tile[2 * TILE];
        __shared__ __attribute__((aligned(16))) float sT[(NB_MAX + 1) * 2 * NB_MAX];
        __shared__ float sWt[NB_MAX + 1];

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
        const float *__restrict__ h0 = a.halo[0], *__restrict__ h1 = a.halo[1], *__restrict__ h2 = a.halo[2];
        const float mh = -a.coef[0];
        for (int g = tid; g < (TY + 2 * H) * LG; g += BLOCK)
        {
            // tx0, HP and stride are multiples of four: a piece lies in its row or outside it
            const int jl = g / LG, il = COLS * (g - jl * LG);
            const int I = tx0 - HP + il, J = ty0 - H + jl;
            V4 t1 = {0.0f, 0.0f, 0.0f, 0.0f}, t2 = {0.0f, 0.0f, 0.0f, 0.0f};
            if (I >= 0 && I < L.stride && J >= 0 && J < L.Ly)
            {
                const int e = J * L.stride + I;
                t1 = *reinterpret_cast<const V4 *>(h0 + e);
                const V4 q = *reinterpret_cast<const V4 *>(h2 + e);
                V4 p = t1;
                if constexpr (!Kind::P_IS_TILE)
                    p = *reinterpret_cast<const V4 *>(h1 + e);
#pragma unroll
                for (int c = 0; c < COLS; ++c)
                {
                    t2[c] = I + c < L.Lx ? fmadd(mh, q[c], p[c]) : 0.0f;
                    t1[c] = I + c < L.Lx ? t1[c] : 0.0f;
                }
            }
            *reinterpret_cast<V4 *>(tile + jl * LW + il) = t1;
            *reinterpret_cast<V4 *>(tile + TILE + jl * LW + il) = t2;
        }
        __syncthreads();

        // what a lane's four columns need in every row
        const int lx = lane & (ROW_LANES - 1), half = lane / ROW_LANES;
        const int I0 = tx0 + COLS * lx;
        int rx[COLS], lox[COLS], hix[COLS];
        float wx[COLS];
#pragma unroll
        for (int c = 0; c < COLS; ++c)
        {
            const bool valid = I0 + c < L.Lx;
            rx[c] = valid ? row_id(I0 + c, L.Lx, nb) : 0;
            lox[c] = valid ? first_offset(rx[c], nb) : 1;
            hix[c] = valid ? last_offset(rx[c], nb) : 0;
            wx[c] = valid ? L.cy * sWt[rx[c]] : 0.0f;
        }
        const int ctr = HP + COLS * lx; // LDS column of I0

        V4 x[PASSES][NIN];
#pragma unroll
        for (int u = 0; u < PASSES; ++u)
        {
            // clamped, not guarded (blas1.hip, map_kernel)
            const int J = min(ty0 + ROWS * (wv + WAVES * u) + half, L.Ly - 1), I = min(I0, L.stride - COLS);
            const int i = (J * L.stride + I) / COLS;
#pragma unroll
            for (int s = 0; s < NIN; ++s)
                x[u][s] = Kind::halo_stream(s) ? stream_load<false>(reinterpret_cast<const V4 *>(a.in[s]) + i)
                                               : stream_load<NT>(reinterpret_cast<const V4 *>(a.in[s]) + i);
        }
#pragma unroll
        for (int u = 0; u < PASSES; ++u)
        {
            const int jt = ROWS * (wv + WAVES * u) + half, J = ty0 + jt;
            if (J < L.Ly && I0 < L.stride)
            {
                const int ry = row_id(J, L.Ly, nb), loy = first_offset(ry, nb), hiy = last_offset(ry, nb);
                const float wy = L.cx * sWt[ry];
                float w[2][COLS];
#pragma unroll
                for (int k = 0; k < 2; ++k)
                {
                    const float *row = tile + k * TILE + (jt + H) * LW + ctr;
                    float sx[COLS] = {0.0f, 0.0f, 0.0f, 0.0f}, sy[COLS] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if constexpr (NBT != 0)
                    {
                        float win[COLS + 2 * HP]; // columns I0 - HP .. I0 + COLS + HP - 1
#pragma unroll
                        for (int j = 0; j < COLS + 2 * HP; j += COLS)
                        {
                            const V4 piece = *reinterpret_cast<const V4 *>(row - HP + j);
#pragma unroll
                            for (int c = 0; c < COLS; ++c)
                                win[j + c] = piece[c];
                        }
#pragma unroll
                        for (int c = 0; c < COLS; ++c)
                        {
#pragma unroll
                            for (int d = -HM; d <= HM; ++d)
                                if (d >= lox[c] && d <= hix[c])
                                    sx[c] = fmadd(sT[rx[c] * WP + d + H], win[HP + c + d], sx[c]);
                        }
#pragma unroll
                        for (int d = -HM; d <= HM; ++d)
                        {
                            const V4 piece = *reinterpret_cast<const V4 *>(row + d * LW); // (a halo row of the tile when out of range)
                            const float coef = sT[ry * WP + d + H];
                            if (d >= loy && d <= hiy)
                            {
#pragma unroll
                                for (int c = 0; c < COLS; ++c)
                                    sy[c] = fmadd(coef, piece[c], sy[c]);
                            }
                        }
                    }
                    else
                    {
#pragma unroll
                        for (int c = 0; c < COLS; ++c)
                            for (int d = lox[c]; d <= hix[c]; ++d)
                                sx[c] = fmadd(sT[rx[c] * WP + d + H], row[c + d], sx[c]);
                        for (int d = loy; d <= hiy; ++d)
                        {
                            const V4 piece = *reinterpret_cast<const V4 *>(row + d * LW);
                            const float coef = sT[ry * WP + d + H];
#pragma unroll
                            for (int c = 0; c < COLS; ++c)
                                sy[c] = fmadd(coef, piece[c], sy[c]);
                        }
                    }
#pragma unroll
                    for (int c = 0; c < COLS; ++c)
                        w[k][c] = fmadd(wy, sx[c], wx[c] * sy[c]);
                }
                const V4 centre = *reinterpret_cast<const V4 *>(tile + (jt + H) * LW + ctr);
                V4 y[NOUT];
#pragma unroll
                for (int c = 0; c < COLS; ++c)
                {
                    float se[NIN], ye[NOUT];
#pragma unroll
                    for (int s = 0; s < NIN; ++s)
                        se[s] = x[u][s][c];
                    Kind::template apply<FORCED>(w[0][c], w[1][c], centre[c], se, ye, a.coef);
#pragma unroll
                    for (int s = 0; s < NOUT; ++s)
                        y[s][c] = ye[s];
                }
                const int i = (J * L.stride + I0) / COLS;
#pragma unroll
                for (int s = 0; s < NOUT; ++s)
                    stream_store<NT>(reinterpret_cast<V4 *>(a.out[s]) + i, y[s]);
            }
        }
    }

    template <typename Kind, int NCOEF>
    int launch_pair32(const cuddh_wave_lattice *D, const float *const (&halo)[PAIR_HALO], const float *const (&in)[Kind::NIN], const float *F,
                      const float *G, float *const (&out)[Kind::NOUT], const double (&coef)[NCOEF], void *stream)
    {
        Lattice32 L;
        PairArgs32 a;
        if (!pair_args<float, Kind>(D, COLS, halo, in, F, G, out, coef, L, a))
            return invalid_value;
        const int grid = ((L.stride + TX - 1) / TX) * ((L.Ly + TY - 1) / TY);
        dispatch_sweep(L.nb, NBasis<4, 5>{}, F != nullptr, static_cast<long long>(L.stride) * L.Ly * sizeof(float),
                       [&](auto forced_c, auto nt_c, auto nbt)
                       { hipLaunchKernelGGL((pair32_kernel<Kind, decltype(forced_c)::value, decltype(nt_c)::value, decltype(nbt)::value>), dim3(grid),
                                            dim3(BLOCK), 0, as_stream(stream), L, a); });
        return launch_status();
    }
} // namespace

extern "C"
{
    int cuddh_hip_wave_pair32_tile_x(void) { return TX; }
    int cuddh_hip_wave_pair32_tile_y(void) { return TY; }

    int cuddh_hip_wave_pair32_rk2(const cuddh_wave_lattice *lattice, double half_dt, double dt, double c0, double s0, double c1, double s1,
                                  double filt, const float *p, const float *q, const float *invm, const float *Hi, const float *F, const float *G,
                                  float *p_out, float *q_out, float *u, float *v, void *stream)
    {
        return launch_pair32<PairRk2T<float>>(lattice, {p, p, q}, {q, u, v, invm, Hi}, F, G, {p_out, q_out, u, v},
                                              {half_dt, dt, c0, s0, c1, s1, filt}, stream);
    }

    int cuddh_hip_wave_pair32_rk4_12(const cuddh_wave_lattice *lattice, double half_dt, double c0, double s0, double c1, double s1, const float *p,
                                     const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps2, float *qs,
                                     float *aq, float *ap, void *stream)
    {
        return launch_pair32<PairRk4_12T<float>>(lattice, {p, p, q}, {q, invm, Hi}, F, G, {ps2, qs, aq, ap}, {half_dt, c0, s0, c1, s1}, stream);
    }

    int cuddh_hip_wave_pair32_rk4_34(const cuddh_wave_lattice *lattice, double dt, double sixth_dt, double c1, double s1, double c2, double s2,
                                     double filt, const float *ps2, const float *p, const float *qs, const float *aq, const float *ap,
                                     const float *invm, const float *Hi, const float *F, const float *G, float *p_out, float *q, float *u,
                                     float *v, void *stream)
    {
        return launch_pair32<PairRk4_34T<float>>(lattice, {ps2, p, qs}, {p, q, qs, aq, ap, u, v, invm, Hi}, F, G, {p_out, q, u, v},
                                                 {dt, sixth_dt, c1, s1, c2, s2, filt}, stream);
    }
}
