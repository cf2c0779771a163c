// The lattice sweeps of wave_lattice.hip with state, stencil and stages stored and computed in fp32: the same
// Kronecker-sum stencil, the same rows and offset ranges (wave_lattice_common.hpp), the same stage formulas (wave_stages.hpp at
// R = float), every product-sum a fused multiply-add (__builtin_fmaf) in the same fixed order:
//   sx = sum_d T[rx][d] p(I + d, J),   sy = sum_d T[ry][d] p(I, J + d),   each from zero, d ascending over the node's range;
//   (K p)(I, J) = fma(cx Wt[ry], sx, (cy Wt[rx]) sy),   the two products formed in float.
// The description is the fp64 one: the host builds T and Wt in double (wave::describe) and rounds each entry, cx, cy and every
// scalar of the call to float once.  Results depend on (I, J) only: bitwise reproducible.
//
// Layout.  Rows have `stride` >= Lx floats, stride a multiple of 4, so that every row starts on a 16-byte boundary; the up to
// three columns from Lx on are padding that must hold zero state, zero load and invm = 0 (the march keeps them zero).  The
// stencil takes p(I, J) for 0 <= I < Lx, 0 <= J < Ly only, and zero elsewhere.
//
// Decomposition.  A workgroup of four wavefronts owns a tile of TX x TY = 128 x 16 nodes.  It stages the stencil input of the tile
// and its halo in LDS as floats by 16-byte loads (cached: the halo is some other tile's interior); the tile's first column sits
// at LDS column HP, the halo rounded up to a multiple of four, and LDS rows hold a multiple of four floats, so that every
// 16-byte piece of a row is aligned.  A lane owns four neighbouring columns, 32 lanes a row, a wavefront two rows per pass
// and two passes: one 16-byte load and one 16-byte store per stream and row, all of a lane's requests (clamped, not guarded)
// issued before its first store, non-temporal from 64 MB per vector.  The x-window of a lane's four columns is read as aligned
// 16-byte pieces, the y-window as one 16-byte piece per offset.  In rk2_a and rk4_1 the stencil input is also the stage's p: it
// is taken from the tile.  Workgroup ids are renumbered as in wave_lattice.hip.  n_basis 4 and 5 are compile-time; every other
// n_basis in [2, 8] shares an instantiation with loops of run-time length over LDS (no register arrays, hence no scratch).
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
    constexpr int COLS = 4;                                  // columns per lane: one 16-byte access per stream
    constexpr int TX = 128, TY = 16;                         // nodes per tile
    constexpr int ROW_LANES = TX / COLS, ROWS = WAVE / ROW_LANES; // lanes per row; rows per wavefront pass
    constexpr int PASSES = TY / (WAVES * ROWS);
    static_assert(ROW_LANES * ROWS == WAVE && PASSES * WAVES * ROWS == TY, "a wavefront pass covers whole rows; the passes cover the tile");

    using V4 = float __attribute__((ext_vector_type(4)));
    using Lattice32 = LatticeT<float>;
    using StageArgs32 = StageArgsT<float>;

    // PSLOT > 0: input PSLOT of the stage is the stencil input itself
    template <typename Stage, int PSLOT, bool FORCED, bool NT, int NBT>
    __global__ void __launch_bounds__(BLOCK) lattice32_kernel(Lattice32 L, StageArgs32 a)
    {
        constexpr int NIN = Stage::NIN + (FORCED ? 2 : 0), NOUT = Stage::NOUT;
        static_assert(NIN <= MAX_IN && NOUT <= MAX_OUT, "StageArgs32 holds every stage");
        constexpr int HM = (NBT ? NBT : NB_MAX) - 1, HP = (HM + COLS - 1) & ~(COLS - 1); // halo; the tile's first column sits at LDS column HP
        constexpr int LW = TX + 2 * HP, LG = LW / COLS;
        __shared__ __attribute__((aligned(16))) float tile[(TY + 2 * HM) * LW];
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
        const float *__restrict__ pin = a.in[0];
        for (int g = tid; g < (TY + 2 * H) * LG; g += BLOCK)
        {
            // tx0, HP and stride are multiples of four: a piece lies in its row or outside it
            const int jl = g / LG, il = COLS * (g - jl * LG);
            const int I = tx0 - HP + il, J = ty0 - H + jl;
            V4 piece = {0.0f, 0.0f, 0.0f, 0.0f};
            if (I >= 0 && I < L.stride && J >= 0 && J < L.Ly)
            {
                piece = *reinterpret_cast<const V4 *>(pin + J * L.stride + I);
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
            for (int s = 1; s < NIN; ++s)
                if (s != PSLOT)
                    x[u][s] = stream_load<NT>(reinterpret_cast<const V4 *>(a.in[s]) + i);
        }
#pragma unroll
        for (int u = 0; u < PASSES; ++u)
        {
            const int jt = ROWS * (wv + WAVES * u) + half, J = ty0 + jt;
            if (J < L.Ly && I0 < L.stride)
            {
                const int ry = row_id(J, L.Ly, nb), loy = first_offset(ry, nb), hiy = last_offset(ry, nb);
                const float wy = L.cx * sWt[ry];
                const float *row = tile + (jt + H) * LW + ctr;
                float sx[COLS] = {0.0f, 0.0f, 0.0f, 0.0f}, sy[COLS] = {0.0f, 0.0f, 0.0f, 0.0f};
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
                }
                V4 y[NOUT];
#pragma unroll
                for (int c = 0; c < COLS; ++c)
                {
                    float xe[NIN], ye[NOUT];
                    xe[0] = fmadd(wy, sx[c], wx[c] * sy[c]);
#pragma unroll
                    for (int s = 1; s < NIN; ++s)
                        xe[s] = x[u][s][c];
                    Stage::template apply<FORCED>(xe, ye, a.coef);
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

    // (the lattice vectors of one period leave through this one; they come in through load_kernel and begin_kernel of
    // wave_lattice_common.hpp)
    __global__ void __launch_bounds__(BLOCK) store32_kernel(int n, const int *__restrict__ slot, const float *__restrict__ x, double *__restrict__ y)
    {
        for (int g = blockIdx.x * BLOCK + threadIdx.x; g < n; g += gridDim.x * BLOCK)
            y[g] = static_cast<double>(x[slot[g]]);
    }

    // the family's launcher (wave_sweep_launch.hpp): one sweep on the entry points' leading arguments
    struct launch_lattice32
    {
        const cuddh_wave_lattice *D;
        void *stream;

        template <typename Stage, int PSLOT>
        int sweep(const float *const (&in)[Stage::NIN], const float *F, const float *G, float *const (&out)[Stage::NOUT],
                  const double (&coef)[MAX_COEF]) const
        {
            Lattice32 L;
            StageArgs32 a;
            if (!describe(D, COLS, L) || !stage_args<Stage>(in, F, G, out, coef, a))
                return invalid_value;
            const int grid = ((L.stride + TX - 1) / TX) * ((L.Ly + TY - 1) / TY);
            dispatch_sweep(L.nb, NBasis<4, 5>{}, F != nullptr, static_cast<long long>(L.stride) * L.Ly * sizeof(float),
                           [&](auto forced_c, auto nt_c, auto nbt)
                           { hipLaunchKernelGGL((lattice32_kernel<Stage, PSLOT, decltype(forced_c)::value, decltype(nt_c)::value, decltype(nbt)::value>),
                                                dim3(grid), dim3(BLOCK), 0, as_stream(stream), L, a); });
            return launch_status();
        }
    };
} // namespace

extern "C"
{
    int cuddh_hip_wave32_tile_x(void) { return TX; }
    int cuddh_hip_wave32_tile_y(void) { return TY; }

    int cuddh_hip_wave32_load(int n, const int *dof_of_slot, const double *x, float *y, void *stream)
    {
        if (n <= 0)
            return 0;
        hipLaunchKernelGGL(load_kernel<float>, dim3(stream_grid(n, LOAD_BLOCK)), dim3(LOAD_BLOCK), 0, as_stream(stream), n, dof_of_slot, x, y);
        return launch_status();
    }

    int cuddh_hip_wave32_begin(int n, double filt0, const int *dof_of_slot, const double *zu, const double *zv, float *p, float *q, float *u,
                               float *v, void *stream)
    {
        if (n <= 0)
            return 0;
        hipLaunchKernelGGL(begin_kernel<float>, dim3(stream_grid(n, LOAD_BLOCK)), dim3(LOAD_BLOCK), 0, as_stream(stream), n, static_cast<float>(filt0), dof_of_slot,
                           zu, zv, p, q, u, v);
        return launch_status();
    }

    int cuddh_hip_wave32_store(int ndof, const int *slot_of_dof, const float *x, double *y, void *stream)
    {
        if (ndof <= 0)
            return 0;
        hipLaunchKernelGGL(store32_kernel, dim3(stream_grid(ndof, BLOCK)), dim3(BLOCK), 0, as_stream(stream), ndof, slot_of_dof, x, y);
        return launch_status();
    }

    int cuddh_hip_wave32_rk2_a(const cuddh_wave_lattice *lattice, double half_dt, double c, double s, const float *p, const float *q,
                               const float *invm, const float *Hi, const float *F, const float *G, float *qh, float *ph, void *stream)
    {
        return rk2_a(launch_lattice32{lattice, stream}, half_dt, c, s, p, q, invm, Hi, F, G, qh, ph);
    }

    int cuddh_hip_wave32_rk2_b(const cuddh_wave_lattice *lattice, double dt, double c, double s, double filt, const float *ph, const float *qh,
                               const float *invm, const float *Hi, const float *F, const float *G, float *p, float *q, float *u, float *v,
                               void *stream)
    {
        return rk2_b(launch_lattice32{lattice, stream}, dt, c, s, filt, ph, qh, invm, Hi, F, G, p, q, u, v);
    }

    int cuddh_hip_wave32_rk4_1(const cuddh_wave_lattice *lattice, double half_dt, double c, double s, const float *p, const float *q,
                               const float *invm, const float *Hi, const float *F, const float *G, float *ps, float *qs, float *aq, float *ap,
                               void *stream)
    {
        return rk4_1(launch_lattice32{lattice, stream}, half_dt, c, s, p, q, invm, Hi, F, G, ps, qs, aq, ap);
    }

    int cuddh_hip_wave32_rk4_2(const cuddh_wave_lattice *lattice, double half_dt, double c, double s, const float *ps_in, const float *p,
                               const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps_out, float *qs,
                               float *aq, float *ap, void *stream)
    {
        return rk4_2(launch_lattice32{lattice, stream}, half_dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
    }

    int cuddh_hip_wave32_rk4_3(const cuddh_wave_lattice *lattice, double dt, double c, double s, const float *ps_in, const float *p,
                               const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps_out, float *qs,
                               float *aq, float *ap, void *stream)
    {
        return rk4_3(launch_lattice32{lattice, stream}, dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
    }

    int cuddh_hip_wave32_rk4_4(const cuddh_wave_lattice *lattice, double sixth_dt, double c, double s, double filt, const float *ps,
                               const float *qs, const float *aq, const float *ap, const float *invm, const float *Hi, const float *F,
                               const float *G, float *p, float *q, float *u, float *v, void *stream)
    {
        return rk4_4(launch_lattice32{lattice, stream}, sixth_dt, c, s, filt, ps, qs, aq, ap, invm, Hi, F, G, p, q, u, v);
    }
}
