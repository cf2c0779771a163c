// The box sweeps of wave_box.hip with state, stencil and stages stored and computed in fp32: the same Kronecker-sum
// stencil on the lattice of Lx x Ly x Lz Gauss-Lobatto nodes, the same rows and offset ranges (wave_lattice_common.hpp), the same
// stage formulas (wave_stages.hpp at R = float), every product-sum a fused multiply-add (__builtin_fmaf) in wave_box.hip's order:
//   sx = sum_d T[rx][d] p(I + d, J, K),   sy = sum_d T[ry][d] p(I, J + d, K),   sz = sum_d T[rz][d] p(I, J, K + d),
//        each from zero, d ascending over the node's range;
//   ax = cx * (Wt[ry] * Wt[rz]),   ay = cy * (Wt[rx] * Wt[rz]),   az = cz * (Wt[rx] * Wt[ry]),   each product rounded, the inner first;
//   (K p)(I, J, K) = fma(ax, sx, fma(ay, sy, az * sz)).
// The description is the fp64 one (cuddh_wave_box): the host builds T and Wt in double (wave::describe) and rounds each entry,
// cx, cy, cz and every scalar of the call to float once.  Results depend on (I, J, K) only: bitwise reproducible.
//
// Layout.  Node (I, J, K) at I + stride (J + Ly K); rows have `stride` >= Lx floats, stride a multiple of 4, so that every row and
// every plane starts on a 16-byte boundary; the up to three columns from Lx on are padding that must hold zero state, zero load and
// invm = 0 (the march keeps them zero).  The stencil never uses them: a padding column's sums are taken as zero.
//
// Decomposition.  A workgroup of four wavefronts owns a tile of TX x TY = 128 x 16 nodes of ONE z plane.  The plane's part of the
// stencil is wave_lattice_f32.hip's: the tile and its x-y halo staged in LDS as floats by 16-byte pieces, a lane four neighbouring
// columns, 32 lanes a row, a wavefront two rows per pass and two passes, one 16-byte load and one 16-byte store per stream and
// row.  The z term is wave_box.hip's: the up to 2 H neighbours of the other planes are cached 16-byte loads, one per plane and
// lane (the centre comes from the tile), and the tiles are numbered with z fastest inside each XCD's contiguous run, so that the
// workgroups resident on an XCD at one time are neighbouring planes of few x-y tiles and meet each other's planes in that XCD's
// L2.  n_basis 4 and 5 are compile-time: all z loads of both passes are issued, clamped, together with the streams, before the
// first is used.  Every other n_basis in [2, 8] shares an instantiation whose loops have run-time bounds over LDS and whose z
// loop has a run-time length (no register arrays, hence no scratch).  Streams are non-temporal from 64 MB per vector.
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
    constexpr int COLS = 4;                                       // columns per lane: one 16-byte access per stream
    constexpr int TX = 128, TY = 16, TZ = 1;                      // nodes per tile
    constexpr int ROW_LANES = TX / COLS, ROWS = WAVE / ROW_LANES; // lanes per row; rows per wavefront pass
    constexpr int PASSES = TY / (WAVES * ROWS);
    static_assert(ROW_LANES * ROWS == WAVE && PASSES * WAVES * ROWS == TY, "a wavefront pass covers whole rows; the passes cover the tile");

    using V4 = float __attribute__((ext_vector_type(4)));

    using Box32 = BoxT<float>; // (wave_lattice_common.hpp)

    using StageArgs32 = StageArgsT<float>;

    // PSLOT > 0: input PSLOT of the stage is the stencil input itself
    template <typename Stage, int PSLOT, bool FORCED, bool NT, int NBT>
    __global__ void __launch_bounds__(BLOCK) box32_kernel(Box32 B, StageArgs32 a)
    {
        constexpr int NIN = Stage::NIN + (FORCED ? 2 : 0), NOUT = Stage::NOUT;
        static_assert(NIN <= MAX_IN && NOUT <= MAX_OUT, "StageArgs32 holds every stage");
        constexpr int HM = (NBT ? NBT : NB_MAX) - 1, HP = (HM + COLS - 1) & ~(COLS - 1); // halo; the tile's first column sits at LDS column HP
        constexpr int LW = TX + 2 * HP, LG = LW / COLS;
        constexpr int NZ = NBT ? 2 * HM : 1; // z neighbours held in registers (compile-time form)
        __shared__ __attribute__((aligned(16))) float tile[(TY + 2 * HM) * LW];
        __shared__ __attribute__((aligned(16))) float sT[(NB_MAX + 1) * 2 * NB_MAX];
        __shared__ float sWt[NB_MAX + 1];

        const LatticeT<float> &L = B.L;
        const int nb = NBT ? NBT : L.nb, H = nb - 1, WP = 2 * nb;
        const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;

        // this workgroup's tile: XCD x gets the x-th contiguous run of tiles, z fastest
        const int ntx = (L.stride + TX - 1) / TX, n_tiles = gridDim.x;
        const int xcd = blockIdx.x % N_XCD, slot = blockIdx.x / N_XCD;
        const int t = xcd * (n_tiles / N_XCD) + min(xcd, n_tiles % N_XCD) + slot;
        const int Kz = t % B.Lz, txy = t / B.Lz;
        const int tx0 = (txy % ntx) * TX, ty0 = (txy / ntx) * TY;
        const int plane = L.stride * L.Ly; // (stride Ly Lz fits in an int); a multiple of four

        for (int i = tid; i < (nb + 1) * WP; i += BLOCK)
            sT[i] = L.T[i];
        if (tid <= nb)
            sWt[tid] = L.Wt[tid];
        const float *__restrict__ pin = a.in[0];
        const float *__restrict__ pk = pin + static_cast<size_t>(Kz) * plane;
        for (int g = tid; g < (TY + 2 * H) * LG; g += BLOCK)
        {
            // tx0, HP and stride are multiples of four: a piece lies in its row or outside it
            const int jl = g / LG, il = COLS * (g - jl * LG);
            const int I = tx0 - HP + il, J = ty0 - H + jl;
            V4 piece = {0.0f, 0.0f, 0.0f, 0.0f};
            if (I >= 0 && I < L.stride && J >= 0 && J < L.Ly)
            {
                piece = *reinterpret_cast<const V4 *>(pk + J * L.stride + I);
#pragma unroll
                for (int c = 0; c < COLS; ++c)
                    piece[c] = I + c < L.Lx ? piece[c] : 0.0f;
            }
            *reinterpret_cast<V4 *>(tile + jl * LW + il) = piece;
        }
        __syncthreads();

        // what a lane's four columns need in every row
        const int lx = lane & (ROW_LANES - 1), half = lane / ROW_LANES;
        const int I0 = tx0 + COLS * lx;
        int rx[COLS], lox[COLS], hix[COLS];
        float wx[COLS];
        bool valid[COLS];
#pragma unroll
        for (int c = 0; c < COLS; ++c)
        {
            valid[c] = I0 + c < L.Lx;
            rx[c] = valid[c] ? row_id(I0 + c, L.Lx, nb) : 0;
            lox[c] = valid[c] ? first_offset(rx[c], nb) : 1;
            hix[c] = valid[c] ? last_offset(rx[c], nb) : 0;
            wx[c] = valid[c] ? sWt[rx[c]] : 0.0f;
        }
        const int ctr = HP + COLS * lx; // LDS column of I0
        // the plane's row of the z line: the same for the whole workgroup
        const int rz = row_id(Kz, B.Lz, nb), loz = first_offset(rz, nb), hiz = last_offset(rz, nb);
        const float wz = sWt[rz];
        float ay[COLS];
#pragma unroll
        for (int c = 0; c < COLS; ++c)
            ay[c] = L.cy * (wx[c] * wz);

        V4 x[PASSES][NIN], zv[PASSES][NZ];
#pragma unroll
        for (int u = 0; u < PASSES; ++u)
        {
            // clamped, not guarded (blas1.hip, map_kernel)
            const int J = min(ty0 + ROWS * (wv + WAVES * u) + half, L.Ly - 1), I = min(I0, L.stride - COLS);
            const size_t i = (static_cast<size_t>(Kz) * plane + J * L.stride + I) / COLS;
#pragma unroll
            for (int s = 1; s < NIN; ++s)
                if (s != PSLOT)
                    x[u][s] = stream_load<NT>(reinterpret_cast<const V4 *>(a.in[s]) + i);
            if constexpr (NBT != 0)
            {
                // the z line of this lane's four columns, every plane clamped into the box; used in range only
                const V4 *zl = reinterpret_cast<const V4 *>(pk + J * L.stride + I);
#pragma unroll
                for (int d = -HM; d <= HM; ++d)
                    if (d != 0)
                        zv[u][d < 0 ? d + HM : d + HM - 1] = zl[static_cast<ptrdiff_t>(min(max(Kz + d, 0), B.Lz - 1) - Kz) * (plane / COLS)];
            }
        }
#pragma unroll
        for (int u = 0; u < PASSES; ++u)
        {
            const int jt = ROWS * (wv + WAVES * u) + half, J = ty0 + jt;
            if (J < L.Ly && I0 < L.stride)
            {
                const int ry = row_id(J, L.Ly, nb), loy = first_offset(ry, nb), hiy = last_offset(ry, nb);
                const float wy = sWt[ry];
                const float ax = L.cx * (wy * wz);
                const float *row = tile + (jt + H) * LW + ctr;
                float sx[COLS] = {0.0f, 0.0f, 0.0f, 0.0f}, sy[COLS] = {0.0f, 0.0f, 0.0f, 0.0f}, sz[COLS] = {0.0f, 0.0f, 0.0f, 0.0f};
                if constexpr (NBT != 0)
                {
                    float win[COLS + 2 * HP]; // columns I0 - HP .. I0 + COLS + HP - 1
#pragma unroll
                    for (int k = 0; k < COLS + 2 * HP; k += COLS)
                    {
                        const V4 piece = *reinterpret_cast<const V4 *>(row - HP + k);
#pragma unroll
                        for (int c = 0; c < COLS; ++c)
                            win[k + c] = piece[c];
                    }
#pragma unroll
                    for (int c = 0; c < COLS; ++c)
                    {
#pragma unroll
                        for (int d = -HM; d <= HM; ++d)
                            if (d >= lox[c] && d <= hix[c])
                                sx[c] = fmadd(sT[rx[c] * WP + d + H], win[HP + c + d], sx[c]);
                        if constexpr (PSLOT > 0)
                            x[u][PSLOT][c] = win[HP + c];
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
#pragma unroll
                    for (int d = -HM; d <= HM; ++d)
                        if (d >= loz && d <= hiz)
                        {
                            const float coef = sT[rz * WP + d + H];
                            const V4 piece = d == 0 ? V4{win[HP], win[HP + 1], win[HP + 2], win[HP + 3]} : zv[u][d < 0 ? d + HM : d + HM - 1];
#pragma unroll
                            for (int c = 0; c < COLS; ++c)
                                sz[c] = fmadd(coef, piece[c], sz[c]);
                        }
                }
                else
                {
#pragma unroll
                    for (int c = 0; c < COLS; ++c)
                    {
                        for (int d = lox[c]; d <= hix[c]; ++d)
                            sx[c] = fmadd(sT[rx[c] * WP + d + H], row[c + d], sx[c]);
                        if constexpr (PSLOT > 0)
                            x[u][PSLOT][c] = row[c];
                    }
                    for (int d = loy; d <= hiy; ++d)
                    {
                        const V4 piece = *reinterpret_cast<const V4 *>(row + d * LW);
                        const float coef = sT[ry * WP + d + H];
#pragma unroll
                        for (int c = 0; c < COLS; ++c)
                            sy[c] = fmadd(coef, piece[c], sy[c]);
                    }
                    // plane Kz + d at zl[d * plane / 4]; the centre is read like the others (the same value as the tile's)
                    const V4 *zl = reinterpret_cast<const V4 *>(pk + J * L.stride + I0);
                    for (int d = loz; d <= hiz; ++d)
                    {
                        const V4 piece = zl[static_cast<ptrdiff_t>(d) * (plane / COLS)];
                        const float coef = sT[rz * WP + d + H];
#pragma unroll
                        for (int c = 0; c < COLS; ++c)
                            sz[c] = fmadd(coef, piece[c], sz[c]);
                    }
                }
                V4 y[NOUT];
#pragma unroll
                for (int c = 0; c < COLS; ++c)
                {
                    float xe[NIN], ye[NOUT];
                    const float az = B.cz * (wx[c] * wy);
                    xe[0] = fmadd(ax, sx[c], fmadd(ay[c], sy[c], az * (valid[c] ? sz[c] : 0.0f)));
#pragma unroll
                    for (int s = 1; s < NIN; ++s)
                        xe[s] = x[u][s][c];
                    Stage::template apply<FORCED>(xe, ye, a.coef);
#pragma unroll
                    for (int s = 0; s < NOUT; ++s)
                        y[s][c] = ye[s];
                }
                const size_t i = (static_cast<size_t>(Kz) * plane + J * L.stride + I0) / COLS;
#pragma unroll
                for (int s = 0; s < NOUT; ++s)
                    stream_store<NT>(reinterpret_cast<V4 *>(a.out[s]) + i, y[s]);
            }
        }
    }

    // the family's launcher (wave_sweep_launch.hpp): one sweep on the entry points' leading arguments
    struct launch_box32
    {
        const cuddh_wave_box *D;
        void *stream;

        template <typename Stage, int PSLOT>
        int sweep(const float *const (&in)[Stage::NIN], const float *F, const float *G, float *const (&out)[Stage::NOUT],
                  const double (&coef)[MAX_COEF]) const
        {
            Box32 B;
            StageArgs32 a;
            if (!describe_box(D, COLS, B) || !stage_args<Stage>(in, F, G, out, coef, a))
                return invalid_value;
            const long long tiles = static_cast<long long>((B.L.stride + TX - 1) / TX) * ((B.L.Ly + TY - 1) / TY) * B.Lz;
            if (tiles > 0x7fffffffLL)
                return invalid_value;
            const int grid = static_cast<int>(tiles);
            dispatch_sweep(B.L.nb, NBasis<4, 5>{}, F != nullptr, static_cast<long long>(B.L.stride) * B.L.Ly * B.Lz * sizeof(float),
                           [&](auto forced_c, auto nt_c, auto nbt)
                           { hipLaunchKernelGGL((box32_kernel<Stage, PSLOT, decltype(forced_c)::value, decltype(nt_c)::value, decltype(nbt)::value>),
                                                dim3(grid), dim3(BLOCK), 0, as_stream(stream), B, a); });
            return launch_status();
        }
    };
} // namespace

extern "C"
{
    int cuddh_hip_wave_box32_tile_x(void) { return TX; }
    int cuddh_hip_wave_box32_tile_y(void) { return TY; }
    int cuddh_hip_wave_box32_tile_z(void) { return TZ; }

    int cuddh_hip_wave_box32_rk2_a(const cuddh_wave_box *box, double half_dt, double c, double s, const float *p, const float *q,
                                   const float *invm, const float *Hi, const float *F, const float *G, float *qh, float *ph, void *stream)
    {
        return rk2_a(launch_box32{box, stream}, half_dt, c, s, p, q, invm, Hi, F, G, qh, ph);
    }

    int cuddh_hip_wave_box32_rk2_b(const cuddh_wave_box *box, double dt, double c, double s, double filt, const float *ph, const float *qh,
                                   const float *invm, const float *Hi, const float *F, const float *G, float *p, float *q, float *u, float *v,
                                   void *stream)
    {
        return rk2_b(launch_box32{box, stream}, dt, c, s, filt, ph, qh, invm, Hi, F, G, p, q, u, v);
    }

    int cuddh_hip_wave_box32_rk4_1(const cuddh_wave_box *box, double half_dt, double c, double s, const float *p, const float *q,
                                   const float *invm, const float *Hi, const float *F, const float *G, float *ps, float *qs, float *aq, float *ap,
                                   void *stream)
    {
        return rk4_1(launch_box32{box, stream}, half_dt, c, s, p, q, invm, Hi, F, G, ps, qs, aq, ap);
    }

    int cuddh_hip_wave_box32_rk4_2(const cuddh_wave_box *box, double half_dt, double c, double s, const float *ps_in, const float *p,
                                   const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps_out, float *qs,
                                   float *aq, float *ap, void *stream)
    {
        return rk4_2(launch_box32{box, stream}, half_dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
    }

    int cuddh_hip_wave_box32_rk4_3(const cuddh_wave_box *box, double dt, double c, double s, const float *ps_in, const float *p,
                                   const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps_out, float *qs,
                                   float *aq, float *ap, void *stream)
    {
        return rk4_3(launch_box32{box, stream}, dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
    }

    int cuddh_hip_wave_box32_rk4_4(const cuddh_wave_box *box, double sixth_dt, double c, double s, double filt, const float *ps,
                                   const float *qs, const float *aq, const float *ap, const float *invm, const float *Hi, const float *F,
                                   const float *G, float *p, float *q, float *u, float *v, void *stream)
    {
        return rk4_4(launch_box32{box, stream}, sixth_dt, c, s, filt, ps, qs, aq, ap, invm, Hi, F, G, p, q, u, v);
    }
}
