// Level-1 kernels: streaming maps with 16-byte accesses and a deterministic
// two-stage reduction (wavefront shuffles, then LDS across the four waves of a
// workgroup, then one wavefront over the per-workgroup partials).
#include "common.hpp"

using namespace cuddh_k;

namespace
{
    constexpr int BLOCK = 256;
    constexpr int MAX_PARTIALS = 1024;

    template <typename T>
    struct Pack; // 16-byte vector of T
    template <>
    struct Pack<double>
    {
        using type = double2;
        static constexpr int N = 2;
    };
    template <>
    struct Pack<float>
    {
        using type = float4;
        static constexpr int N = 4;
    };
    template <>
    struct Pack<int>
    {
        using type = int4;
        static constexpr int N = 4;
    };

    inline bool aligned16(const void *p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

    // Access pattern of every streaming kernel here (profiles/r03/stream_copy_variants.txt, 1 GiB of doubles on MI355X): a
    // workgroup works on contiguous TILES of UNROLL x 256 sixteen-byte vectors, a thread's UNROLL accesses 256 vectors (4 KiB)
    // apart, and workgroups take tiles in order -- at any moment the chip reads one contiguous window.  A copy that way runs at
    // 6.2 TB/s (read + write); the former grid-stride form, whose four accesses per thread were a whole grid apart, at 4.4.
    // Vectors too large to stay in the 256 MB infinity cache anyway are read and written with the non-temporal hint.
    constexpr int UNROLL = 4;
    constexpr int TILE = UNROLL * BLOCK; // 16-byte vectors per tile
    constexpr long long NT_BYTES = 64LL << 20;

    template <bool NT, typename V>
    __device__ inline V stream_load(const V *p)
    {
        if constexpr (NT)
            return __builtin_nontemporal_load(p);
        else
            return *p;
    }
    template <bool NT, typename V>
    __device__ inline void stream_store(V *p, const V &v)
    {
        if constexpr (NT)
            __builtin_nontemporal_store(v, p);
        else
            *p = v;
    }
    inline int tile_grid(long long n_vectors, int cap)
    {
        long long g = (n_vectors + TILE - 1) / TILE;
        if (g > cap)
            g = cap;
        return static_cast<int>(g < 1 ? 1 : g);
    }

    // ---------------- y = f(x, y) element-wise; F is a functor T(T x, T y)
    template <typename T, typename F, bool READ_X, bool READ_Y, bool NT>
    __global__ void __launch_bounds__(BLOCK) map_kernel(int n, const T *__restrict__ x, T *__restrict__ y, F f, int vectorised)
    {
        using V = typename Pack<T>::type;
        using VE = T __attribute__((ext_vector_type(Pack<T>::N))); // (clang vector: what the non-temporal builtins take)
        constexpr int N = Pack<T>::N;
        static_assert(sizeof(V) == sizeof(VE), "16-byte vectors");
        int done = 0;
        if (vectorised)
        {
            const int nv = n / N;
            const int n_tiles = (nv + TILE - 1) / TILE;
            const VE *xv = reinterpret_cast<const VE *>(x);
            VE *yv = reinterpret_cast<VE *>(y);
            for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
            {
                const int base = tile * TILE + threadIdx.x;
                VE a[UNROLL], b[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u)
                {
                    // clamped, not guarded: a request under `if (i < nv)` is a basic block of its own and the tile's requests
                    // would go out one group at a time (see mgs_stage_kernel)
                    const int i = min(base + u * BLOCK, nv - 1);
                    if (READ_X)
                        a[u] = stream_load<NT>(xv + i);
                    if (READ_Y)
                        b[u] = stream_load<NT>(yv + i);
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u)
                {
                    const int i = base + u * BLOCK;
                    if (i < nv)
                    {
                        VE r;
#pragma unroll
                        for (int c = 0; c < N; ++c)
                            r[c] = f(READ_X ? a[u][c] : T(0), READ_Y ? b[u][c] : T(0));
                        stream_store<NT>(yv + i, r);
                    }
                }
            }
            done = nv * N;
        }
        const int tid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
        for (int i = done + tid; i < n; i += stride)
            y[i] = f(READ_X ? x[i] : T(0), READ_Y ? y[i] : T(0));
    }

    template <typename T, bool RX, bool RY, typename F>
    int launch_map(int n, const T *x, T *y, F f, void *stream)
    {
        if (n <= 0)
            return 0;
        const int vec = aligned16(y) && (!RX || aligned16(x));
        const int g = tile_grid(n / Pack<T>::N, 1 << 20);
        if (static_cast<long long>(n) * sizeof(T) >= NT_BYTES)
            hipLaunchKernelGGL((map_kernel<T, F, RX, RY, true>), dim3(g), dim3(BLOCK), 0, as_stream(stream), n, x, y, f, vec);
        else
            hipLaunchKernelGGL((map_kernel<T, F, RX, RY, false>), dim3(g), dim3(BLOCK), 0, as_stream(stream), n, x, y, f, vec);
        return launch_status();
    }

    // functors
    template <typename T>
    struct Axpby
    {
        T a, b;
        __device__ T operator()(T x, T y) const { return a * x + b * y; }
    };
    template <typename T>
    struct Ax
    {
        T a;
        __device__ T operator()(T x, T) const { return a * x; }
    };
    template <typename T>
    struct AxpbyDev
    {
        T sa;
        const T *a;
        T b;
        __device__ T operator()(T x, T y) const { return (sa * *a) * x + b * y; }
    };
    template <typename T>
    struct ScaleInvDev
    {
        const T *a;
        __device__ T operator()(T, T y) const { return y / *a; }
    };
    template <typename T>
    struct Scale
    {
        T a;
        __device__ T operator()(T, T y) const { return y * a; }
    };
    template <typename T>
    struct Const
    {
        T a;
        __device__ T operator()(T, T) const { return a; }
    };
    template <typename T>
    struct Ident
    {
        __device__ T operator()(T x, T) const { return x; }
    };
    struct Recip
    {
        __device__ double operator()(double, double y) const { return 1.0 / y; }
    };

    // ---------------- reductions
    template <typename T>
    __device__ inline T block_sum(T v)
    {
        __shared__ T part[BLOCK / WAVE];
        v = wave_sum(v);
        const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
        if (lane == 0)
            part[w] = v;
        __syncthreads();
        T s = T(0);
        if (threadIdx.x == 0)
        {
#pragma unroll
            for (int i = 0; i < BLOCK / WAVE; ++i)
                s += part[i];
        }
        return s; // valid in thread 0
    }

    // MODE 0: sum x*y   1: sum (x-y)^2   2: sum x*x (one stream: y is not read)
    template <typename T, int MODE, bool NT>
    __global__ void __launch_bounds__(BLOCK) reduce_stage1(int n, const T *__restrict__ x, const T *__restrict__ y, T *__restrict__ partial,
                                                           int vectorised)
    {
        using VE = T __attribute__((ext_vector_type(Pack<T>::N)));
        constexpr int N = Pack<T>::N;
        T acc = T(0);
        int done = 0;
        auto term = [&](T a, T b)
        {
            if (MODE == 0)
                acc += a * b;
            else if (MODE == 1)
            {
                const T d = a - b;
                acc += d * d;
            }
            else
                acc += a * a;
        };
        if (vectorised)
        {
            const int nv = n / N;
            const int n_tiles = (nv + TILE - 1) / TILE;
            const VE *xv = reinterpret_cast<const VE *>(x), *yv = reinterpret_cast<const VE *>(y);
            for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) // contiguous tiles, taken in order by the workgroups
            {
                const int base = tile * TILE + threadIdx.x;
                VE a[UNROLL], b[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u)
                {
                    const int i = min(base + u * BLOCK, nv - 1); // (clamped, not guarded: see map_kernel)
                    a[u] = stream_load<NT>(xv + i);
                    if (MODE != 2)
                        b[u] = stream_load<NT>(yv + i);
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u)
                    if (base + u * BLOCK < nv)
#pragma unroll
                        for (int c = 0; c < N; ++c)
                            term(a[u][c], MODE != 2 ? b[u][c] : T(0));
            }
            done = nv * N;
        }
        const int tid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
        for (int i = done + tid; i < n; i += stride)
            term(x[i], MODE != 2 ? y[i] : T(0));
        const T s = block_sum(acc);
        if (threadIdx.x == 0)
            partial[blockIdx.x] = s;
    }

    template <typename T, bool SQRT>
    __global__ void __launch_bounds__(BLOCK) reduce_stage2(int n_partial, const T *__restrict__ partial, T *__restrict__ result)
    {
        T acc = T(0);
        for (int i = threadIdx.x; i < n_partial; i += BLOCK)
            acc += partial[i];
        const T s = block_sum(acc);
        if (threadIdx.x == 0)
            *result = SQRT ? sqrt(s) : s;
    }

    template <typename T, int MODE, bool SQRT>
    int launch_reduce(int n, const T *x, const T *y, T *result, void *ws, void *stream)
    {
        if constexpr (MODE == 0)
            if (x == y) // <x, x>: one stream instead of two (the same products, bit for bit)
                return launch_reduce<T, 2, SQRT>(n, x, y, result, ws, stream);
        T *partial = static_cast<T *>(ws);
        const int g = tile_grid(n / Pack<T>::N, MAX_PARTIALS);
        const int vec = aligned16(x) && aligned16(y);
        if (static_cast<long long>(n) * sizeof(T) >= NT_BYTES)
            hipLaunchKernelGGL((reduce_stage1<T, MODE, true>), dim3(g), dim3(BLOCK), 0, as_stream(stream), n, x, y, partial, vec);
        else
            hipLaunchKernelGGL((reduce_stage1<T, MODE, false>), dim3(g), dim3(BLOCK), 0, as_stream(stream), n, x, y, partial, vec);
        hipLaunchKernelGGL((reduce_stage2<T, SQRT>), dim3(1), dim3(BLOCK), 0, as_stream(stream), g, partial, result);
        return launch_status();
    }

    // explicit fused multiply-adds in the Gram-Schmidt kernels: left to the compiler, the fp32 stage kernel got packed multiplies + adds
    // (two roundings) where the same expressions in another kernel became FMAs -- the results must not depend on that choice
    __device__ inline double fmadd(double a, double b, double c) { return __builtin_fma(a, b, c); }
    __device__ inline float fmadd(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

    // ---------------- fused modified Gram-Schmidt stage (one launch per projection instead of dot + reduce + axpy)
    // stage:  h = sum(pin)            (the coefficient <w, v_prev> whose partial sums the previous stage left behind)
    //         w <- w - h * v_prev     (skipped when v_prev == nullptr: first stage)
    //         pout[block] = partial sum of <w, v_next>   (v_next == nullptr: <w, w>, for the norm)
    // Every workgroup sums the same <= MAX_PARTIALS partials in the same order, so all of them use the same h.
    // PREV / NEXT: v_prev / v_next given (compile-time, so that no request sits under a run-time condition).  A workgroup's FIRST tile
    // is requested before the coefficient is summed -- the requests do not depend on it -- with clamped addresses and no branches,
    // and the <= 4 partial sums per thread go out with them: for vectors of a few MB (config 2: 9.5 MB) a stage is a chain of
    // dependent trips, not a bandwidth problem, and the former form (requests under `if (i < nv)` inside the tile loop, whose header
    // waits for everything outstanding; the partial sums in a loop of their own) made seven of them in a row
    // (profiles/r03/mgs_stage_small_vectors.txt).
    template <typename T, bool PREV, bool NEXT>
    __global__ void __launch_bounds__(BLOCK) mgs_stage_kernel(int n, T *__restrict__ w, const T *__restrict__ vprev, const T *__restrict__ vnext,
                                                              const T *__restrict__ pin, int npin, T *__restrict__ pout, T *__restrict__ hout,
                                                              int vectorised)
    {
        __shared__ T h_sh;
        using VE = T __attribute__((ext_vector_type(Pack<T>::N)));
        constexpr int N = Pack<T>::N;
        const int nv = vectorised ? n / N : 0;
        const int n_tiles = (nv + TILE - 1) / TILE;
        VE *wv = reinterpret_cast<VE *>(w);
        const VE *pv = reinterpret_cast<const VE *>(vprev), *nvv = reinterpret_cast<const VE *>(vnext);
        int tile = blockIdx.x;
        const bool first = tile < n_tiles; // (workgroup-uniform)
        VE a0[UNROLL], b0[UNROLL], c0[UNROLL];
        if (first)
        {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                const int i = min(tile * TILE + (int)threadIdx.x + u * BLOCK, nv - 1);
                a0[u] = wv[i];
                if constexpr (PREV)
                    b0[u] = pv[i];
                if constexpr (NEXT)
                    c0[u] = nvv[i];
            }
        }
        T h = T(0);
        if constexpr (PREV)
        {
            static_assert(MAX_PARTIALS <= 4 * BLOCK, "four partial sums per thread");
            T q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                q[k] = pin[min((int)threadIdx.x + k * BLOCK, npin - 1)];
            T a = T(0);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                a = (int)threadIdx.x + k * BLOCK < npin ? a + q[k] : a; // (the order of the former loop)
            const T s = block_sum(a);
            if (threadIdx.x == 0)
            {
                h_sh = s;
                if (blockIdx.x == 0)
                    *hout = s;
            }
            __syncthreads();
            h = h_sh;
        }
        T acc = T(0);
        const int tid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
        if (first)
        {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                const int i = tile * TILE + (int)threadIdx.x + u * BLOCK;
                if (i < nv)
                {
#pragma unroll
                    for (int e = 0; e < N; ++e)
                    {
                        if constexpr (PREV)
                            a0[u][e] = fmadd(-h, b0[u][e], a0[u][e]);
                        acc = fmadd(a0[u][e], NEXT ? c0[u][e] : a0[u][e], acc);
                    }
                    if constexpr (PREV)
                        wv[i] = a0[u];
                }
            }
            tile += gridDim.x;
        }
        // further tiles (vectors of more than MAX_PARTIALS tiles, 16 MB: enough workgroups in flight to hide the trips)
        for (; tile < n_tiles; tile += gridDim.x)
        {
            const int base = tile * TILE + threadIdx.x;
            VE a[UNROLL], b[UNROLL], c[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                const int i = min(base + u * BLOCK, nv - 1); // (clamped, not guarded: all requests of a tile go out together)
                a[u] = wv[i];
                if constexpr (PREV)
                    b[u] = pv[i];
                if constexpr (NEXT)
                    c[u] = nvv[i];
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                const int i = base + u * BLOCK;
                if (i < nv)
                {
#pragma unroll
                    for (int e = 0; e < N; ++e)
                    {
                        if constexpr (PREV)
                            a[u][e] = fmadd(-h, b[u][e], a[u][e]);
                        acc = fmadd(a[u][e], NEXT ? c[u][e] : a[u][e], acc);
                    }
                    if constexpr (PREV)
                        wv[i] = a[u];
                }
            }
        }
        for (int i = nv * N + tid; i < n; i += stride)
        {
            T wi = w[i];
            if constexpr (PREV)
            {
                wi = fmadd(-h, vprev[i], wi);
                w[i] = wi;
            }
            acc = fmadd(wi, NEXT ? vnext[i] : wi, acc);
        }
        __syncthreads(); // block_sum reuses its LDS scratch
        const T s = block_sum(acc);
        if (threadIdx.x == 0)
            pout[blockIdx.x] = s;
    }

    // nrm = sqrt(sum(pin));  *hout = nrm;  w <- w / nrm
    template <typename T>
    __global__ void __launch_bounds__(BLOCK) mgs_finish_kernel(int n, T *__restrict__ w, const T *__restrict__ pin, int npin, T *__restrict__ hout,
                                                               int vectorised)
    {
        __shared__ T nrm_sh;
        using VE = T __attribute__((ext_vector_type(Pack<T>::N)));
        constexpr int N = Pack<T>::N;
        const int nv = vectorised ? n / N : 0;
        const int n_tiles = (nv + TILE - 1) / TILE;
        VE *wv = reinterpret_cast<VE *>(w);
        int tile = blockIdx.x;
        const bool first = tile < n_tiles; // the first tile is requested before the norm is summed (see mgs_stage_kernel)
        VE a0[UNROLL];
        if (first)
        {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                a0[u] = wv[min(tile * TILE + (int)threadIdx.x + u * BLOCK, nv - 1)];
        }
        T q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            q[k] = pin[min((int)threadIdx.x + k * BLOCK, npin - 1)];
        T a = T(0);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            a = (int)threadIdx.x + k * BLOCK < npin ? a + q[k] : a;
        const T s = block_sum(a);
        if (threadIdx.x == 0)
        {
            nrm_sh = sqrt(s);
            if (blockIdx.x == 0)
                *hout = nrm_sh;
        }
        __syncthreads();
        const T nrm = nrm_sh;
        const int tid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
        if (first)
        {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                const int i = tile * TILE + (int)threadIdx.x + u * BLOCK;
                if (i < nv)
                {
#pragma unroll
                    for (int c = 0; c < N; ++c)
                        a0[u][c] = a0[u][c] / nrm;
                    wv[i] = a0[u];
                }
            }
            tile += gridDim.x;
        }
        for (; tile < n_tiles; tile += gridDim.x)
        {
            const int base = tile * TILE + threadIdx.x;
            VE av[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                av[u] = wv[min(base + u * BLOCK, nv - 1)];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                if (base + u * BLOCK < nv)
                {
#pragma unroll
                    for (int c = 0; c < N; ++c)
                        av[u][c] = av[u][c] / nrm;
                    wv[base + u * BLOCK] = av[u];
                }
        }
        for (int i = nv * N + tid; i < n; i += stride)
            w[i] = w[i] / nrm;
    }

    inline int mgs_grid(int n) { return tile_grid(n / 2, MAX_PARTIALS); } // (n / 2: at least as many tiles as either precision has)

    template <typename T>
    int launch_mgs_stage(int n, T *w, const T *vprev, const T *vnext, const T *pin, T *pout, T *hout, void *stream)
    {
        const int g = mgs_grid(n);
        const int vec = aligned16(w) && (!vprev || aligned16(vprev)) && (!vnext || aligned16(vnext));
        const dim3 grid(g), block(BLOCK);
        hipStream_t st = as_stream(stream);
        if (vprev && vnext)
            hipLaunchKernelGGL((mgs_stage_kernel<T, true, true>), grid, block, 0, st, n, w, vprev, vnext, pin, g, pout, hout, vec);
        else if (vprev)
            hipLaunchKernelGGL((mgs_stage_kernel<T, true, false>), grid, block, 0, st, n, w, vprev, vnext, pin, g, pout, hout, vec);
        else if (vnext)
            hipLaunchKernelGGL((mgs_stage_kernel<T, false, true>), grid, block, 0, st, n, w, vprev, vnext, pin, g, pout, hout, vec);
        else
            hipLaunchKernelGGL((mgs_stage_kernel<T, false, false>), grid, block, 0, st, n, w, vprev, vnext, pin, g, pout, hout, vec);
        return launch_status();
    }

    template <typename T>
    int launch_mgs_finish(int n, T *w, const T *pin, T *hout, void *stream)
    {
        const int g = mgs_grid(n);
        hipLaunchKernelGGL((mgs_finish_kernel<T>), dim3(g), dim3(BLOCK), 0, as_stream(stream), n, w, pin, g, hout, aligned16(w) ? 1 : 0);
        return launch_status();
    }

    // ---------------- classical Gram-Schmidt pass against all k1 basis vectors at once (CGS2: krylov.cpp::queue_step_cgs2)
    // Every coefficient of a pass is an inner product with the SAME w, so a pass is one launch whatever k1 is:
    //   UPDATE    c[j] = sum_p cin[j cstride + p] (p < ncin) for every j < k1, by every workgroup in the same order;
    //             workgroup 0 writes hout[j] = (hacc ? hacc[j] : 0) + c[j];  w <- w - sum_j c[j] v_j, per element in ascending j
    //   DOTS 1    pout row 1 + j <- per-workgroup partial sums of <w, v_j> (the updated w), row 0 <- those of <w, w>
    //   DOTS 2    row 0 only: what mgs_finish_kernel reads
    // Rows of pout are CGS_ROW apart.  A tile of w stays in registers while the basis streams past it in chunks of CGS_KC
    // vectors; an UPDATE + DOTS 1 pass reads each tile of V a second time for the dots of the updated w (it cannot be kept: k1 x 16 KiB).
    // The per-j sums cannot be registers indexed at run time: a chunk's CGS_KC accumulators are reduced per wavefront and added
    // to LDS (k1 + 1 rows x 4 waves), in tile order by one lane per wave, so the order is fixed.
    constexpr int CGS_KC = 4;
    constexpr int CGS_KMAX = 512;
    constexpr int CGS_ROW = MAX_PARTIALS;
    constexpr int NWAVES = BLOCK / WAVE;

    // c[j] = sum_p cin[j cstride + p], p < ncin <= 4 BLOCK, for j < rows, in the order in which mgs_stage_kernel and
    // mgs_finish_kernel sum their partials (<= 4 per thread in ascending p, wave_sum, the four waves in order): the UPDATE
    // prologue and cgs_reduce_kernel both get their sums here, and row 0 of a pass summed here is mgs_finish's own sum.
    // part: rows x NWAVES of LDS scratch.  Ends with a barrier: c is valid in every thread.
    template <typename T>
    __device__ inline void cgs_sum_rows(const T *__restrict__ cin, size_t cstride, int ncin, int rows, T *__restrict__ c, T *__restrict__ part)
    {
        static_assert(MAX_PARTIALS <= 4 * BLOCK, "four partial sums per thread");
        const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
        for (int j0 = 0; j0 < rows; j0 += CGS_KC)
        {
            T q[CGS_KC][4];
#pragma unroll
            for (int r = 0; r < CGS_KC; ++r)
            {
                const T *row = cin + static_cast<size_t>(min(j0 + r, rows - 1)) * cstride;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    q[r][k] = row[min((int)threadIdx.x + k * BLOCK, ncin - 1)];
            }
#pragma unroll
            for (int r = 0; r < CGS_KC; ++r)
            {
                T a = T(0);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    a = (int)threadIdx.x + k * BLOCK < ncin ? a + q[r][k] : a;
                a = wave_sum(a);
                if (lane == 0 && j0 + r < rows)
                    part[(j0 + r) * NWAVES + wv] = a;
            }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < rows; j += BLOCK)
        {
            T s = T(0);
#pragma unroll
            for (int i = 0; i < NWAVES; ++i)
                s += part[j * NWAVES + i];
            c[j] = s;
        }
        __syncthreads();
    }

    template <typename T, bool UPDATE, int DOTS>
    __global__ void __launch_bounds__(BLOCK) cgs_pass_kernel(int n, T *__restrict__ w, const T *__restrict__ V, size_t ldv, int k1, const T *__restrict__ cin,
                                                             int ncin, size_t cstride, const T *__restrict__ hacc, T *__restrict__ hout, T *__restrict__ pout,
                                                             int vectorised)
    {
        static_assert(DOTS == 1 || (DOTS == 2 && UPDATE), "pass A: dots; pass B: update + dots; pass C: update + <w, w>");
        __shared__ T c_sh[UPDATE ? CGS_KMAX : 1];
        __shared__ T d_sh[CGS_KMAX * NWAVES]; // per-wave sums of <w, v_j> (before that: scratch of the prologue)
        using VE = T __attribute__((ext_vector_type(Pack<T>::N)));
        constexpr int N = Pack<T>::N;
        const int nv = vectorised ? n / N : 0;
        const int n_tiles = (nv + TILE - 1) / TILE;
        const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
        VE *wv = reinterpret_cast<VE *>(w);
        auto basis = [&](int j) { return reinterpret_cast<const VE *>(V + static_cast<size_t>(min(j, k1 - 1)) * ldv); }; // (clamped: see below)

        // requests of a tile: w, and a chunk of CGS_KC basis vectors; clamped addresses (element and basis vector), no branches
        auto request_w = [&](int tile, VE(&a)[UNROLL])
        {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                a[u] = wv[min(tile * TILE + (int)threadIdx.x + u * BLOCK, nv - 1)];
        };
        auto request_chunk = [&](int tile, int j0, VE(&b)[CGS_KC][UNROLL])
        {
#pragma unroll
            for (int q = 0; q < CGS_KC; ++q)
            {
                const VE *vj = basis(j0 + q);
#pragma unroll
                for (int u = 0; u < UNROLL; ++u)
                    b[q][u] = vj[min(tile * TILE + (int)threadIdx.x + u * BLOCK, nv - 1)];
            }
        };
        // a chunk's sums of this thread, reduced per wavefront and added to the rows of d_sh by lane 0
        auto deposit = [&](int j0, const T(&acc)[CGS_KC])
        {
#pragma unroll
            for (int q = 0; q < CGS_KC; ++q)
            {
                const T s = wave_sum(acc[q]);
                if (lane == 0 && j0 + q < k1)
                    d_sh[(j0 + q) * NWAVES + wave] += s;
            }
        };

        int tile = blockIdx.x;
        const bool first = tile < n_tiles; // (workgroup-uniform)
        VE a[UNROLL], b[CGS_KC][UNROLL];
        if (first) // a workgroup's FIRST tile is requested before the coefficients are summed (see mgs_stage_kernel)
        {
            request_w(tile, a);
            request_chunk(tile, 0, b);
        }
        if constexpr (UPDATE)
        {
            cgs_sum_rows(cin, cstride, ncin, k1, c_sh, d_sh);
            if (blockIdx.x == 0)
                for (int j = threadIdx.x; j < k1; j += BLOCK)
                    hout[j] = (hacc ? hacc[j] : T(0)) + c_sh[j];
        }
        if constexpr (DOTS == 1)
        {
            for (int i = threadIdx.x; i < k1 * NWAVES; i += BLOCK)
                d_sh[i] = T(0);
            __syncthreads();
        }

        T ww = T(0);
        bool requested = first;
        for (; tile < n_tiles; tile += gridDim.x)
        {
            const int base = tile * TILE + threadIdx.x;
            if (!requested)
            {
                request_w(tile, a);
                request_chunk(tile, 0, b);
            }
            requested = false;
            if constexpr (UPDATE)
            {
                for (int j0 = 0; j0 < k1; j0 += CGS_KC)
                {
                    if (j0 > 0)
                        request_chunk(tile, j0, b);
#pragma unroll
                    for (int q = 0; q < CGS_KC; ++q)
                        if (j0 + q < k1) // (uniform)
                        {
                            const T c = c_sh[j0 + q];
#pragma unroll
                            for (int u = 0; u < UNROLL; ++u)
#pragma unroll
                                for (int e = 0; e < N; ++e)
                                    a[u][e] = fmadd(-c, b[q][u][e], a[u][e]);
                        }
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u)
                    if (base + u * BLOCK < nv)
                        wv[base + u * BLOCK] = a[u];
            }
            if constexpr (DOTS == 1)
            {
                for (int j0 = 0; j0 < k1; j0 += CGS_KC)
                {
                    if (UPDATE || j0 > 0)
                        request_chunk(tile, j0, b);
                    T acc[CGS_KC];
#pragma unroll
                    for (int q = 0; q < CGS_KC; ++q)
                    {
                        acc[q] = T(0);
#pragma unroll
                        for (int u = 0; u < UNROLL; ++u)
                            if (base + u * BLOCK < nv)
#pragma unroll
                                for (int e = 0; e < N; ++e)
                                    acc[q] = fmadd(a[u][e], b[q][u][e], acc[q]);
                    }
                    deposit(j0, acc);
                }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                if (base + u * BLOCK < nv)
#pragma unroll
                    for (int e = 0; e < N; ++e)
                        ww = fmadd(a[u][e], a[u][e], ww);
        }

        // scalar tail (everything, when an operand is not 16-byte aligned): a thread's elements are its own in every loop below,
        // so it reads back only what it wrote itself
        const int tid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
        const int i0 = nv * N + tid;
        if constexpr (UPDATE)
            for (int i = i0; i < n; i += stride)
            {
                T wi = w[i];
                for (int j = 0; j < k1; ++j)
                    wi = fmadd(-c_sh[j], V[static_cast<size_t>(j) * ldv + i], wi);
                w[i] = wi;
            }
        if (nv * N < n) // (uniform)
        {
            if constexpr (DOTS == 1)
                for (int j0 = 0; j0 < k1; j0 += CGS_KC)
                {
                    T acc[CGS_KC];
#pragma unroll
                    for (int q = 0; q < CGS_KC; ++q)
                        acc[q] = T(0);
                    for (int i = i0; i < n; i += stride)
                    {
                        const T wi = w[i];
#pragma unroll
                        for (int q = 0; q < CGS_KC; ++q)
                            acc[q] = fmadd(wi, V[static_cast<size_t>(min(j0 + q, k1 - 1)) * ldv + i], acc[q]);
                    }
                    deposit(j0, acc);
                }
            for (int i = i0; i < n; i += stride)
                ww = fmadd(w[i], w[i], ww);
        }

        __syncthreads();
        if constexpr (DOTS == 1)
            for (int j = threadIdx.x; j < k1; j += BLOCK)
            {
                T s = T(0);
#pragma unroll
                for (int i = 0; i < NWAVES; ++i)
                    s += d_sh[j * NWAVES + i];
                pout[static_cast<size_t>(1 + j) * CGS_ROW + blockIdx.x] = s;
            }
        const T s = block_sum(ww);
        if (threadIdx.x == 0)
            pout[blockIdx.x] = s;
    }

    // out[j] = sum of row 1 + j of a pass's partials (<w, v_j>), j < k1;  out[k1] = sum of row 0 (<w, w>)
    template <typename T>
    __global__ void __launch_bounds__(BLOCK) cgs_reduce_kernel(int k1, const T *__restrict__ partials, int npart, T *__restrict__ out)
    {
        __shared__ T c_sh[CGS_KMAX + 1];
        __shared__ T part[(CGS_KMAX + 1) * NWAVES];
        cgs_sum_rows(partials, static_cast<size_t>(CGS_ROW), npart, k1 + 1, c_sh, part);
        for (int j = threadIdx.x; j <= k1; j += BLOCK)
            out[j == 0 ? k1 : j - 1] = c_sh[j];
    }

    template <typename T>
    int launch_cgs_pass(int n, T *w, const T *V, long long ldv, int k1, int update, int dots, const T *cin, int ncin, long long cstride, const T *hacc,
                        T *hout, T *pout, void *stream)
    {
        const bool form = (!update && dots == 1) || (update && (dots == 1 || dots == 2));
        if (n < 0 || k1 < 1 || k1 > CGS_KMAX || !form || (k1 > 1 && ldv < n) || (update && (ncin < 1 || ncin > MAX_PARTIALS || cstride < 0)))
            return static_cast<int>(hipErrorInvalidValue);
        if (n == 0)
            return 0;
        const int g = mgs_grid(n);
        const int vec = aligned16(w) && aligned16(V) && (k1 == 1 || ldv % Pack<T>::N == 0);
        const dim3 grid(g), block(BLOCK);
        hipStream_t st = as_stream(stream);
        const size_t ld = static_cast<size_t>(ldv), cs = static_cast<size_t>(cstride);
        if (!update)
            hipLaunchKernelGGL((cgs_pass_kernel<T, false, 1>), grid, block, 0, st, n, w, V, ld, k1, cin, ncin, cs, hacc, hout, pout, vec);
        else if (dots == 1)
            hipLaunchKernelGGL((cgs_pass_kernel<T, true, 1>), grid, block, 0, st, n, w, V, ld, k1, cin, ncin, cs, hacc, hout, pout, vec);
        else
            hipLaunchKernelGGL((cgs_pass_kernel<T, true, 2>), grid, block, 0, st, n, w, V, ld, k1, cin, ncin, cs, hacc, hout, pout, vec);
        return launch_status();
    }

    template <typename T>
    int launch_cgs_reduce(int n, int k1, const T *partials, T *out, void *stream)
    {
        if (n < 0 || k1 < 0 || k1 > CGS_KMAX)
            return static_cast<int>(hipErrorInvalidValue);
        if (n == 0)
            return 0;
        hipLaunchKernelGGL((cgs_reduce_kernel<T>), dim3(1), dim3(BLOCK), 0, as_stream(stream), k1, partials, mgs_grid(n), out);
        return launch_status();
    }

    // ---------------- solution update of an augmented GMRES cycle (krylov.cpp, augment > 0)
    //   d = sum_j coef[j] V_j + sum_p coef[nvc + p] Z_p   per element: from 0, one fused multiply-add per column, V in ascending j, then Z in ascending p
    //   dx <- d;  x <- x + d;  pout[block] = partial sum of d^2   (row 0 of a cgs_pass buffer: cgs_reduce with k1 = 0 finishes it)
    // One launch instead of a chain of nvc + nz axpby on x: x is read and written once, (nvc + nz + 3) n scalars move instead of
    // 3 (nvc + nz) n.  Tiles, clamped requests and the chunking of the columns (CGS_KC at a time, the V columns and the Z columns as
    // one sequence) as in cgs_pass_kernel; every operand is touched once, so vectors beyond the infinity cache go with the
    // non-temporal hint (map_kernel).  The coefficients sit in LDS.  dx overlaps no input.
    template <typename T, bool NT>
    __global__ void __launch_bounds__(BLOCK) krylov_update_kernel(int n, T *__restrict__ x, T *__restrict__ dx, const T *__restrict__ V, size_t ldv, int nvc,
                                                                  const T *__restrict__ Z, size_t ldz, int nz, const T *__restrict__ coef,
                                                                  T *__restrict__ pout, int vectorised)
    {
        __shared__ T c_sh[CGS_KMAX];
        using VE = T __attribute__((ext_vector_type(Pack<T>::N)));
        constexpr int N = Pack<T>::N;
        const int nc = nvc + nz;
        const int nv = vectorised ? n / N : 0;
        const int n_tiles = (nv + TILE - 1) / TILE;
        VE *xv = reinterpret_cast<VE *>(x), *dv = reinterpret_cast<VE *>(dx);
        // column j of the sequence V_0 .. V_{nvc-1}, Z_0 .. Z_{nz-1} (clamped to the last one: a chunk's requests carry no branch)
        auto column = [&](int j)
        {
            j = min(j, nc - 1);
            return j < nvc ? V + static_cast<size_t>(j) * ldv : Z + static_cast<size_t>(j - nvc) * ldz;
        };
        auto request_chunk = [&](int tile, int j0, VE(&b)[CGS_KC][UNROLL])
        {
#pragma unroll
            for (int q = 0; q < CGS_KC; ++q)
            {
                const VE *uj = reinterpret_cast<const VE *>(column(j0 + q));
#pragma unroll
                for (int u = 0; u < UNROLL; ++u)
                    b[q][u] = stream_load<NT>(uj + min(tile * TILE + (int)threadIdx.x + u * BLOCK, nv - 1));
            }
        };

        for (int j = threadIdx.x; j < nc; j += BLOCK)
            c_sh[j] = coef[j];
        __syncthreads();

        T dd = T(0);
        for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
        {
            const int base = tile * TILE + threadIdx.x;
            VE a[UNROLL], d[UNROLL], b[CGS_KC][UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                a[u] = stream_load<NT>(xv + min(base + u * BLOCK, nv - 1));
#pragma unroll
                for (int e = 0; e < N; ++e)
                    d[u][e] = T(0);
            }
            for (int j0 = 0; j0 < nc; j0 += CGS_KC)
            {
                request_chunk(tile, j0, b);
#pragma unroll
                for (int q = 0; q < CGS_KC; ++q)
                    if (j0 + q < nc) // (uniform)
                    {
                        const T c = c_sh[j0 + q];
#pragma unroll
                        for (int u = 0; u < UNROLL; ++u)
#pragma unroll
                            for (int e = 0; e < N; ++e)
                                d[u][e] = fmadd(c, b[q][u][e], d[u][e]);
                    }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                if (base + u * BLOCK < nv)
                {
#pragma unroll
                    for (int e = 0; e < N; ++e)
                    {
                        a[u][e] = a[u][e] + d[u][e];
                        dd = fmadd(d[u][e], d[u][e], dd);
                    }
                    stream_store<NT>(dv + base + u * BLOCK, d[u]);
                    stream_store<NT>(xv + base + u * BLOCK, a[u]);
                }
        }

        // scalar tail (everything, when an operand is not 16-byte aligned)
        const int tid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
        for (int i = nv * N + tid; i < n; i += stride)
        {
            T d = T(0);
            for (int j = 0; j < nvc; ++j)
                d = fmadd(c_sh[j], V[static_cast<size_t>(j) * ldv + i], d);
            for (int p = 0; p < nz; ++p)
                d = fmadd(c_sh[nvc + p], Z[static_cast<size_t>(p) * ldz + i], d);
            dx[i] = d;
            x[i] = x[i] + d;
            dd = fmadd(d, d, dd);
        }

        const T s = block_sum(dd);
        if (threadIdx.x == 0)
            pout[blockIdx.x] = s;
    }

    template <typename T>
    int launch_krylov_update(int n, T *x, T *dx, const T *V, long long ldv, int nvc, const T *Z, long long ldz, int nz, const T *coef, T *pout, void *stream)
    {
        if (n < 0 || nvc < 1 || nz < 0 || nvc + nz > CGS_KMAX || (nvc > 1 && ldv < n) || (nz > 1 && ldz < n))
            return static_cast<int>(hipErrorInvalidValue);
        if (n == 0)
            return 0;
        const int g = mgs_grid(n);
        const int vec = aligned16(x) && aligned16(dx) && aligned16(V) && (nvc == 1 || ldv % Pack<T>::N == 0) &&
                        (nz == 0 || (aligned16(Z) && (nz == 1 || ldz % Pack<T>::N == 0)));
        const dim3 grid(g), block(BLOCK);
        hipStream_t st = as_stream(stream);
        const size_t lv = static_cast<size_t>(ldv), lz = static_cast<size_t>(ldz);
        if (static_cast<long long>(n) * sizeof(T) >= NT_BYTES)
            hipLaunchKernelGGL((krylov_update_kernel<T, true>), grid, block, 0, st, n, x, dx, V, lv, nvc, Z, lz, nz, coef, pout, vec);
        else
            hipLaunchKernelGGL((krylov_update_kernel<T, false>), grid, block, 0, st, n, x, dx, V, lv, nvc, Z, lz, nz, coef, pout, vec);
        return launch_status();
    }

    // ---------------- complex arithmetic on split vectors (krylov.cpp, GmresOptions::arithmetic = complex)
    // A vector of n = 2 h scalars stands for h complex numbers, real parts at [0, h), imaginary parts at [h, 2 h).  The fused
    // Gram-Schmidt stage and the cycle update below are mgs_stage_kernel and krylov_update_kernel with a complex coefficient:
    //   stage:   c = (sum of row 0 of pin) + i (sum of row 1)     (rows CPLX_ROW apart; <v_prev, w> left behind by the previous stage)
    //            w <- w - c v_prev:   w_r -= c_r v_r - c_i v_i,   w_i -= c_r v_i + c_i v_r       (skipped when v_prev == nullptr)
    //            pout row 0 / row 1 [block] = partial sums of Re / Im <v_next, w> = (v_r w_r + v_i w_i) + i (v_r w_i - v_i w_r)
    //            (v_next == nullptr: row 0 = those of |w|^2 -- what mgs_finish_kernel on the 2 h scalars reads -- and row 1 = 0)
    //   update:  x <- x + sum_j y_j v_j, y_j = coef[2 j] + i coef[2 j + 1], per element in ascending j
    // A tile is CUNROLL x 256 sixteen-byte vectors of EACH half: the bytes of a tile, the requests in flight per thread and the
    // grid are those of the real kernels on the same 2 h scalars, and so is the number of launches per Arnoldi step.  The
    // imaginary half starts h scalars behind the real one: 16-byte accesses need h to be a multiple of the vector width (and
    // aligned operands); anything else takes the element-wise path for the whole vector, chosen on the host.
    constexpr int CUNROLL = UNROLL / 2;
    constexpr int CTILE = CUNROLL * BLOCK; // 16-byte vectors of one half per tile
    constexpr int CPLX_ROW = MAX_PARTIALS;

    // sums of the two rows of partials, in mgs_stage_kernel's order; valid in thread 0
    template <typename T>
    __device__ inline void cplx_sum_partials(const T *__restrict__ pin, int npin, T &sr, T &si)
    {
        static_assert(MAX_PARTIALS <= 4 * BLOCK, "four partial sums per thread");
        T q[2][4];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                q[c][k] = pin[c * CPLX_ROW + min((int)threadIdx.x + k * BLOCK, npin - 1)];
        T a[2] = {T(0), T(0)};
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                a[c] = (int)threadIdx.x + k * BLOCK < npin ? a[c] + q[c][k] : a[c];
        sr = block_sum(a[0]);
        __syncthreads(); // block_sum reuses its LDS scratch
        si = block_sum(a[1]);
    }

    template <typename T, bool PREV, bool NEXT>
    __global__ void __launch_bounds__(BLOCK) cmgs_stage_kernel(int h, T *__restrict__ w, const T *__restrict__ vprev, const T *__restrict__ vnext,
                                                               const T *__restrict__ pin, int npin, T *__restrict__ pout, T *__restrict__ hout,
                                                               int vectorised)
    {
        __shared__ T c_sh[2];
        using VE = T __attribute__((ext_vector_type(Pack<T>::N)));
        constexpr int N = Pack<T>::N;
        const int nv = vectorised ? h / N : 0; // vectors of one half
        const int n_tiles = (nv + CTILE - 1) / CTILE;
        VE *wv[2] = {reinterpret_cast<VE *>(w), reinterpret_cast<VE *>(w + h)};
        const VE *pv[2] = {reinterpret_cast<const VE *>(vprev), reinterpret_cast<const VE *>(vprev + h)};
        const VE *nx[2] = {reinterpret_cast<const VE *>(vnext), reinterpret_cast<const VE *>(vnext + h)};

        // requests of a tile: both halves of w, v_prev and v_next; clamped addresses, no branches (see mgs_stage_kernel)
        auto request = [&](int tile, VE(&a)[2][CUNROLL], VE(&b)[2][CUNROLL], VE(&c)[2][CUNROLL])
        {
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int u = 0; u < CUNROLL; ++u)
                {
                    const int i = min(tile * CTILE + (int)threadIdx.x + u * BLOCK, nv - 1);
                    a[p][u] = wv[p][i];
                    if constexpr (PREV)
                        b[p][u] = pv[p][i];
                    if constexpr (NEXT)
                        c[p][u] = nx[p][i];
                }
        };
        T cr = T(0), ci = T(0), accr = T(0), acci = T(0);
        // one complex element: the projection, then its terms of the next inner product
        auto element = [&](T &wr, T &wi, T pr, T pi, T nr, T ni)
        {
            if constexpr (PREV)
            {
                wr = fmadd(ci, pi, fmadd(-cr, pr, wr));
                wi = fmadd(-ci, pr, fmadd(-cr, pi, wi));
            }
            if constexpr (NEXT)
            {
                accr = fmadd(ni, wi, fmadd(nr, wr, accr));
                acci = fmadd(-ni, wr, fmadd(nr, wi, acci));
            }
            else
                accr = fmadd(wi, wi, fmadd(wr, wr, accr));
        };
        auto use = [&](int tile, VE(&a)[2][CUNROLL], VE(&b)[2][CUNROLL], VE(&c)[2][CUNROLL])
        {
#pragma unroll
            for (int u = 0; u < CUNROLL; ++u)
            {
                const int i = tile * CTILE + (int)threadIdx.x + u * BLOCK;
                if (i < nv)
                {
#pragma unroll
                    for (int e = 0; e < N; ++e)
                    {
                        T wr = a[0][u][e], wi = a[1][u][e]; // (a vector's element does not bind to a reference)
                        element(wr, wi, PREV ? b[0][u][e] : T(0), PREV ? b[1][u][e] : T(0), NEXT ? c[0][u][e] : T(0), NEXT ? c[1][u][e] : T(0));
                        a[0][u][e] = wr;
                        a[1][u][e] = wi;
                    }
                    if constexpr (PREV)
                    {
                        wv[0][i] = a[0][u];
                        wv[1][i] = a[1][u];
                    }
                }
            }
        };

        int tile = blockIdx.x;
        const bool first = tile < n_tiles; // (workgroup-uniform)
        VE a0[2][CUNROLL], b0[2][CUNROLL], c0[2][CUNROLL];
        if (first) // a workgroup's FIRST tile is requested before the coefficient is summed (see mgs_stage_kernel)
            request(tile, a0, b0, c0);
        if constexpr (PREV)
        {
            T sr, si;
            cplx_sum_partials(pin, npin, sr, si);
            if (threadIdx.x == 0)
            {
                c_sh[0] = sr;
                c_sh[1] = si;
                if (blockIdx.x == 0)
                {
                    hout[0] = sr;
                    hout[1] = si;
                }
            }
            __syncthreads();
            cr = c_sh[0];
            ci = c_sh[1];
        }
        if (first)
        {
            use(tile, a0, b0, c0);
            tile += gridDim.x;
        }
        for (; tile < n_tiles; tile += gridDim.x)
        {
            VE a[2][CUNROLL], b[2][CUNROLL], c[2][CUNROLL];
            request(tile, a, b, c);
            use(tile, a, b, c);
        }
        const int tid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
        for (int i = nv * N + tid; i < h; i += stride)
        {
            T wr = w[i], wi = w[h + i];
            element(wr, wi, PREV ? vprev[i] : T(0), PREV ? vprev[h + i] : T(0), NEXT ? vnext[i] : T(0), NEXT ? vnext[h + i] : T(0));
            if constexpr (PREV)
            {
                w[i] = wr;
                w[h + i] = wi;
            }
        }
        __syncthreads(); // block_sum reuses its LDS scratch
        const T sr = block_sum(accr);
        __syncthreads();
        const T si = block_sum(acci);
        if (threadIdx.x == 0)
        {
            pout[blockIdx.x] = sr;
            pout[CPLX_ROW + blockIdx.x] = si;
        }
    }

    inline int cplx_grid(int h) { return mgs_grid(2 * h); } // (the real chain's grid on the same scalars: mgs_finish_kernel reads row 0)

    template <typename T>
    int launch_cmgs_stage(int h, T *w, const T *vprev, const T *vnext, const T *pin, T *pout, T *hout, void *stream)
    {
        if (h < 0 || h > (1 << 30) - 1)
            return static_cast<int>(hipErrorInvalidValue);
        if (h == 0)
            return 0;
        const int g = cplx_grid(h);
        const int vec = h % Pack<T>::N == 0 && aligned16(w) && (!vprev || aligned16(vprev)) && (!vnext || aligned16(vnext));
        const dim3 grid(g), block(BLOCK);
        hipStream_t st = as_stream(stream);
        if (vprev && vnext)
            hipLaunchKernelGGL((cmgs_stage_kernel<T, true, true>), grid, block, 0, st, h, w, vprev, vnext, pin, g, pout, hout, vec);
        else if (vprev)
            hipLaunchKernelGGL((cmgs_stage_kernel<T, true, false>), grid, block, 0, st, h, w, vprev, vnext, pin, g, pout, hout, vec);
        else if (vnext)
            hipLaunchKernelGGL((cmgs_stage_kernel<T, false, true>), grid, block, 0, st, h, w, vprev, vnext, pin, g, pout, hout, vec);
        else
            hipLaunchKernelGGL((cmgs_stage_kernel<T, false, false>), grid, block, 0, st, h, w, vprev, vnext, pin, g, pout, hout, vec);
        return launch_status();
    }

    // x <- x + sum_j (coef[2 j] + i coef[2 j + 1]) v_j, v_j = V + j ldv (its halves h apart), j < k1 <= CGS_KMAX: one launch, x read
    // and written once, the columns in chunks of CGS_KC past a tile of x in registers (krylov_update_kernel)
    template <typename T, bool NT>
    __global__ void __launch_bounds__(BLOCK) ckrylov_update_kernel(int h, T *__restrict__ x, const T *__restrict__ V, size_t ldv, int k1,
                                                                   const T *__restrict__ coef, int vectorised)
    {
        __shared__ T c_sh[2 * CGS_KMAX];
        using VE = T __attribute__((ext_vector_type(Pack<T>::N)));
        constexpr int N = Pack<T>::N;
        const int nv = vectorised ? h / N : 0;
        const int n_tiles = (nv + CTILE - 1) / CTILE;
        VE *xv[2] = {reinterpret_cast<VE *>(x), reinterpret_cast<VE *>(x + h)};
        auto request_chunk = [&](int tile, int j0, VE(&b)[CGS_KC][2][CUNROLL])
        {
#pragma unroll
            for (int q = 0; q < CGS_KC; ++q)
            {
                const T *vj = V + static_cast<size_t>(min(j0 + q, k1 - 1)) * ldv; // (clamped: a chunk's requests carry no branch)
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int u = 0; u < CUNROLL; ++u)
                        b[q][p][u] = stream_load<NT>(reinterpret_cast<const VE *>(vj + static_cast<size_t>(p) * h) +
                                                     min(tile * CTILE + (int)threadIdx.x + u * BLOCK, nv - 1));
            }
        };

        for (int j = threadIdx.x; j < 2 * k1; j += BLOCK)
            c_sh[j] = coef[j];
        __syncthreads();

        for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
        {
            const int base = tile * CTILE + threadIdx.x;
            VE a[2][CUNROLL], b[CGS_KC][2][CUNROLL];
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int u = 0; u < CUNROLL; ++u)
                    a[p][u] = stream_load<NT>(xv[p] + min(base + u * BLOCK, nv - 1));
            for (int j0 = 0; j0 < k1; j0 += CGS_KC)
            {
                request_chunk(tile, j0, b);
#pragma unroll
                for (int q = 0; q < CGS_KC; ++q)
                    if (j0 + q < k1) // (uniform)
                    {
                        const T yr = c_sh[2 * (j0 + q)], yi = c_sh[2 * (j0 + q) + 1];
#pragma unroll
                        for (int u = 0; u < CUNROLL; ++u)
#pragma unroll
                            for (int e = 0; e < N; ++e)
                            {
                                a[0][u][e] = fmadd(-yi, b[q][1][u][e], fmadd(yr, b[q][0][u][e], a[0][u][e]));
                                a[1][u][e] = fmadd(yi, b[q][0][u][e], fmadd(yr, b[q][1][u][e], a[1][u][e]));
                            }
                    }
            }
#pragma unroll
            for (int u = 0; u < CUNROLL; ++u)
                if (base + u * BLOCK < nv)
                {
                    stream_store<NT>(xv[0] + base + u * BLOCK, a[0][u]);
                    stream_store<NT>(xv[1] + base + u * BLOCK, a[1][u]);
                }
        }

        // scalar tail (everything, when an operand is not 16-byte aligned or h is no multiple of the vector width)
        const int tid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
        for (int i = nv * N + tid; i < h; i += stride)
        {
            T xr = x[i], xi = x[h + i];
            for (int j = 0; j < k1; ++j)
            {
                const T vr = V[static_cast<size_t>(j) * ldv + i], vi = V[static_cast<size_t>(j) * ldv + h + i];
                xr = fmadd(-c_sh[2 * j + 1], vi, fmadd(c_sh[2 * j], vr, xr));
                xi = fmadd(c_sh[2 * j + 1], vr, fmadd(c_sh[2 * j], vi, xi));
            }
            x[i] = xr;
            x[h + i] = xi;
        }
    }

    template <typename T>
    int launch_ckrylov_update(int h, T *x, const T *V, long long ldv, int k1, const T *coef, void *stream)
    {
        if (h < 0 || h > (1 << 30) - 1 || k1 < 1 || k1 > CGS_KMAX || (k1 > 1 && ldv < 2LL * h))
            return static_cast<int>(hipErrorInvalidValue);
        if (h == 0)
            return 0;
        const int g = cplx_grid(h);
        const int vec = h % Pack<T>::N == 0 && aligned16(x) && aligned16(V) && (k1 == 1 || ldv % Pack<T>::N == 0);
        const dim3 grid(g), block(BLOCK);
        hipStream_t st = as_stream(stream);
        const size_t lv = static_cast<size_t>(ldv);
        if (2LL * h * static_cast<long long>(sizeof(T)) >= NT_BYTES)
            hipLaunchKernelGGL((ckrylov_update_kernel<T, true>), grid, block, 0, st, h, x, V, lv, k1, coef, vec);
        else
            hipLaunchKernelGGL((ckrylov_update_kernel<T, false>), grid, block, 0, st, h, x, V, lv, k1, coef, vec);
        return launch_status();
    }

    // ---------------- indexed maps
    __global__ void __launch_bounds__(BLOCK) gather_kernel(int n, const int *__restrict__ proj, const double *__restrict__ x, double *__restrict__ y)
    {
        for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK)
            y[i] = x[proj[i]];
    }

    __global__ void __launch_bounds__(BLOCK) scatter_add_kernel(int n, const int *__restrict__ proj, const double *__restrict__ x, double *__restrict__ y)
    {
        // proj is injective (FaceSpace dof -> distinct H1 dof), so a plain read-modify-write is race free
        for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK)
            y[proj[i]] += x[i];
    }

    __global__ void __launch_bounds__(BLOCK) zero_indexed_kernel(int n, const int *__restrict__ proj, double *__restrict__ x)
    {
        for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK)
            x[proj[i]] = 0.0;
    }

    // trace exchange of the multi-GPU DDH path (slot t stands for entries t and n_half + t of a trace vector):
    // pack: buf[i] = v[slot[i]], buf[n + i] = v[n_half + slot[i]] and, with clear != 0, v <- 0 there (the slots belong to the
    // receiving rank); unpack: v[slot[i]] = buf[i], v[n_half + slot[i]] = buf[n + i]
    template <typename T>
    __global__ void __launch_bounds__(BLOCK) trace_pack_kernel(int n, int n_half, const int *__restrict__ slot, T *__restrict__ v, T *__restrict__ buf, int clear)
    {
        for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK)
        {
            const int t = slot[i];
            buf[i] = v[t];
            buf[n + i] = v[n_half + t];
            if (clear)
            {
                v[t] = T(0);
                v[n_half + t] = T(0);
            }
        }
    }

    template <typename T>
    __global__ void __launch_bounds__(BLOCK) trace_unpack_kernel(int n, int n_half, const int *__restrict__ slot, const T *__restrict__ buf, T *__restrict__ v)
    {
        for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK)
        {
            const int t = slot[i];
            v[t] = buf[i];
            v[n_half + t] = buf[n + i];
        }
    }

    // halo exchange of the partitioned operator apply: entries t and n_half + t of a local [u; v] vector travel as the PAIR
    // (buf[2 i], buf[2 i + 1]), so the messages for several neighbours are contiguous pieces of one buffer packed by one launch
    __global__ void __launch_bounds__(BLOCK) halo_pack_kernel(int n, int n_half, const int *__restrict__ ids, double *__restrict__ v, double2 *__restrict__ buf,
                                                              int clear)
    {
        for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK)
        {
            const int t = ids[i];
            buf[i] = make_double2(v[t], v[n_half + t]);
            if (clear)
            {
                v[t] = 0.0;
                v[n_half + t] = 0.0;
            }
        }
    }

    __global__ void __launch_bounds__(BLOCK) halo_unpack_kernel(int n, int n_half, const int *__restrict__ ids, const double2 *__restrict__ buf,
                                                                double *__restrict__ v, int add)
    {
        for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK)
        {
            const int t = ids[i]; // the ids of one unpack are distinct: a dof has one owner and, per sender, appears once
            const double2 b = buf[i];
            v[t] = add ? v[t] + b.x : b.x;
            v[n_half + t] = add ? v[n_half + t] + b.y : b.y;
        }
    }

    // y[r] = (accumulate ? y[r] : 0) + sum_{k in [off[r], off[r+1])} x[src[k]], the terms added in the order they are listed
    __global__ void __launch_bounds__(BLOCK) csr_sum_kernel(int n_rows, const int *__restrict__ off, const int *__restrict__ src, const double *__restrict__ x,
                                                            double *__restrict__ y, int accumulate)
    {
        for (int r = blockIdx.x * BLOCK + threadIdx.x; r < n_rows; r += gridDim.x * BLOCK)
        {
            double s = accumulate ? y[r] : 0.0;
            for (int k = off[r]; k < off[r + 1]; ++k)
                s += x[src[k]];
            y[r] = s;
        }
    }

    __global__ void __launch_bounds__(BLOCK) diag_scale_kernel(int n, int accumulate, double c, const double *__restrict__ p, const double *x, double *y)
    {
        // x may alias y (DiagInvMassMatrix is applied in place by the DDH example)
        for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK)
        {
            const double v = c * p[i] * x[i];
            y[i] = accumulate ? y[i] + v : v;
        }
    }
} // namespace

extern "C"
{
    size_t cuddh_hip_reduce_ws_bytes(void) { return 2 * MAX_PARTIALS * sizeof(double); }

    int cuddh_hip_mgs_stage_f64(int n, double *w, const double *vprev, const double *vnext, const double *pin, double *pout, double *hout, void *s)
    {
        return launch_mgs_stage<double>(n, w, vprev, vnext, pin, pout, hout, s);
    }
    int cuddh_hip_mgs_stage_f32(int n, float *w, const float *vprev, const float *vnext, const float *pin, float *pout, float *hout, void *s)
    {
        return launch_mgs_stage<float>(n, w, vprev, vnext, pin, pout, hout, s);
    }
    int cuddh_hip_mgs_finish_f64(int n, double *w, const double *pin, double *hout, void *s) { return launch_mgs_finish<double>(n, w, pin, hout, s); }
    int cuddh_hip_mgs_finish_f32(int n, float *w, const float *pin, float *hout, void *s) { return launch_mgs_finish<float>(n, w, pin, hout, s); }

    size_t cuddh_hip_cgs_ws_bytes(int k1) { return k1 < 0 ? 0 : (static_cast<size_t>(k1) + 1) * CGS_ROW * sizeof(double); }
    int cuddh_hip_cgs_partials(int n) { return mgs_grid(n); }
    int cuddh_hip_cgs_pass_f64(int n, double *w, const double *V, long long ldv, int k1, int update, int dots, const double *cin, int ncin, long long cstride,
                               const double *hacc, double *hout, double *pout, void *s)
    {
        return launch_cgs_pass<double>(n, w, V, ldv, k1, update, dots, cin, ncin, cstride, hacc, hout, pout, s);
    }
    int cuddh_hip_cgs_pass_f32(int n, float *w, const float *V, long long ldv, int k1, int update, int dots, const float *cin, int ncin, long long cstride,
                               const float *hacc, float *hout, float *pout, void *s)
    {
        return launch_cgs_pass<float>(n, w, V, ldv, k1, update, dots, cin, ncin, cstride, hacc, hout, pout, s);
    }
    int cuddh_hip_cgs_reduce_f64(int n, int k1, const double *partials, double *out, void *s) { return launch_cgs_reduce<double>(n, k1, partials, out, s); }
    int cuddh_hip_cgs_reduce_f32(int n, int k1, const float *partials, float *out, void *s) { return launch_cgs_reduce<float>(n, k1, partials, out, s); }
    int cuddh_hip_krylov_update_f64(int n, double *x, double *dx, const double *V, long long ldv, int nv, const double *Z, long long ldz, int nz,
                                    const double *coef, double *pout, void *s)
    {
        return launch_krylov_update<double>(n, x, dx, V, ldv, nv, Z, ldz, nz, coef, pout, s);
    }
    int cuddh_hip_krylov_update_f32(int n, float *x, float *dx, const float *V, long long ldv, int nv, const float *Z, long long ldz, int nz,
                                    const float *coef, float *pout, void *s)
    {
        return launch_krylov_update<float>(n, x, dx, V, ldv, nv, Z, ldz, nz, coef, pout, s);
    }

    size_t cuddh_hip_cmgs_ws_bytes(void) { return 4 * MAX_PARTIALS * sizeof(double); }
    int cuddh_hip_cmgs_stage_f64(int h, double *w, const double *vprev, const double *vnext, const double *pin, double *pout, double *hout, void *s)
    {
        return launch_cmgs_stage<double>(h, w, vprev, vnext, pin, pout, hout, s);
    }
    int cuddh_hip_cmgs_stage_f32(int h, float *w, const float *vprev, const float *vnext, const float *pin, float *pout, float *hout, void *s)
    {
        return launch_cmgs_stage<float>(h, w, vprev, vnext, pin, pout, hout, s);
    }
    int cuddh_hip_ckrylov_update_f64(int h, double *x, const double *V, long long ldv, int k1, const double *coef, void *s)
    {
        return launch_ckrylov_update<double>(h, x, V, ldv, k1, coef, s);
    }
    int cuddh_hip_ckrylov_update_f32(int h, float *x, const float *V, long long ldv, int k1, const float *coef, void *s)
    {
        return launch_ckrylov_update<float>(h, x, V, ldv, k1, coef, s);
    }

    int cuddh_hip_axpby_f64(int n, double a, const double *x, double b, double *y, void *s)
    {
        if (b == 0.0)
            return launch_map<double, true, false>(n, x, y, Ax<double>{a}, s);
        return launch_map<double, true, true>(n, x, y, Axpby<double>{a, b}, s);
    }
    int cuddh_hip_axpby_f32(int n, float a, const float *x, float b, float *y, void *s)
    {
        if (b == 0.0f)
            return launch_map<float, true, false>(n, x, y, Ax<float>{a}, s);
        return launch_map<float, true, true>(n, x, y, Axpby<float>{a, b}, s);
    }
    int cuddh_hip_axpby_dev_f64(int n, double sa, const double *a, const double *x, double b, double *y, void *s)
    {
        return launch_map<double, true, true>(n, x, y, AxpbyDev<double>{sa, a, b}, s);
    }
    int cuddh_hip_axpby_dev_f32(int n, float sa, const float *a, const float *x, float b, float *y, void *s)
    {
        return launch_map<float, true, true>(n, x, y, AxpbyDev<float>{sa, a, b}, s);
    }
    int cuddh_hip_scal_inv_dev_f64(int n, const double *a, double *x, void *s)
    {
        return launch_map<double, false, true>(n, static_cast<const double *>(nullptr), x, ScaleInvDev<double>{a}, s);
    }
    int cuddh_hip_scal_inv_dev_f32(int n, const float *a, float *x, void *s)
    {
        return launch_map<float, false, true>(n, static_cast<const float *>(nullptr), x, ScaleInvDev<float>{a}, s);
    }

    int cuddh_hip_dot_f64(int n, const double *x, const double *y, double *r, void *ws, void *s) { return launch_reduce<double, 0, false>(n, x, y, r, ws, s); }
    int cuddh_hip_dot_f32(int n, const float *x, const float *y, float *r, void *ws, void *s) { return launch_reduce<float, 0, false>(n, x, y, r, ws, s); }
    int cuddh_hip_nrm2_f64(int n, const double *x, double *r, void *ws, void *s) { return launch_reduce<double, 2, true>(n, x, x, r, ws, s); }
    int cuddh_hip_nrm2_f32(int n, const float *x, float *r, void *ws, void *s) { return launch_reduce<float, 2, true>(n, x, x, r, ws, s); }
    int cuddh_hip_sqdist_f64(int n, const double *x, const double *y, double *r, void *ws, void *s) { return launch_reduce<double, 1, false>(n, x, y, r, ws, s); }
    int cuddh_hip_sqdist_f32(int n, const float *x, const float *y, float *r, void *ws, void *s) { return launch_reduce<float, 1, false>(n, x, y, r, ws, s); }

    int cuddh_hip_copy_f64(int n, const double *x, double *y, void *s) { return launch_map<double, true, false>(n, x, y, Ident<double>{}, s); }
    int cuddh_hip_copy_f32(int n, const float *x, float *y, void *s) { return launch_map<float, true, false>(n, x, y, Ident<float>{}, s); }
    int cuddh_hip_copy_i32(int n, const int *x, int *y, void *s) { return launch_map<int, true, false>(n, x, y, Ident<int>{}, s); }

    int cuddh_hip_scal_f64(int n, double a, double *x, void *s) { return launch_map<double, false, true>(n, static_cast<const double *>(nullptr), x, Scale<double>{a}, s); }
    int cuddh_hip_scal_f32(int n, float a, float *x, void *s) { return launch_map<float, false, true>(n, static_cast<const float *>(nullptr), x, Scale<float>{a}, s); }

    int cuddh_hip_fill_f64(int n, double a, double *x, void *s) { return launch_map<double, false, false>(n, static_cast<const double *>(nullptr), x, Const<double>{a}, s); }
    int cuddh_hip_fill_f32(int n, float a, float *x, void *s) { return launch_map<float, false, false>(n, static_cast<const float *>(nullptr), x, Const<float>{a}, s); }
    int cuddh_hip_fill_i32(int n, int a, int *x, void *s) { return launch_map<int, false, false>(n, static_cast<const int *>(nullptr), x, Const<int>{a}, s); }

    int cuddh_hip_reciprocal_f64(int n, double *x, void *s) { return launch_map<double, false, true>(n, static_cast<const double *>(nullptr), x, Recip{}, s); }

    int cuddh_hip_diag_scale_f64(int n, int accumulate, double c, const double *p, const double *x, double *y, void *s)
    {
        if (n <= 0)
            return 0;
        hipLaunchKernelGGL(diag_scale_kernel, dim3(stream_grid(n, BLOCK)), dim3(BLOCK), 0, as_stream(s), n, accumulate, c, p, x, y);
        return launch_status();
    }

    int cuddh_hip_gather_f64(int n, const int *proj, const double *x, double *y, void *s)
    {
        if (n <= 0)
            return 0;
        hipLaunchKernelGGL(gather_kernel, dim3(stream_grid(n, BLOCK)), dim3(BLOCK), 0, as_stream(s), n, proj, x, y);
        return launch_status();
    }
    int cuddh_hip_scatter_add_f64(int n, const int *proj, const double *x, double *y, void *s)
    {
        if (n <= 0)
            return 0;
        hipLaunchKernelGGL(scatter_add_kernel, dim3(stream_grid(n, BLOCK)), dim3(BLOCK), 0, as_stream(s), n, proj, x, y);
        return launch_status();
    }
    int cuddh_hip_trace_pack_f32(int n, int n_half, const int *slot, float *v, float *buf, int clear, void *s)
    {
        if (n > 0)
            hipLaunchKernelGGL((trace_pack_kernel<float>), dim3(stream_grid(n, BLOCK)), dim3(BLOCK), 0, as_stream(s), n, n_half, slot, v, buf, clear);
        return n > 0 ? launch_status() : 0;
    }
    int cuddh_hip_trace_pack_f64(int n, int n_half, const int *slot, double *v, double *buf, int clear, void *s)
    {
        if (n > 0)
            hipLaunchKernelGGL((trace_pack_kernel<double>), dim3(stream_grid(n, BLOCK)), dim3(BLOCK), 0, as_stream(s), n, n_half, slot, v, buf, clear);
        return n > 0 ? launch_status() : 0;
    }
    int cuddh_hip_trace_unpack_f32(int n, int n_half, const int *slot, const float *buf, float *v, void *s)
    {
        if (n > 0)
            hipLaunchKernelGGL((trace_unpack_kernel<float>), dim3(stream_grid(n, BLOCK)), dim3(BLOCK), 0, as_stream(s), n, n_half, slot, buf, v);
        return n > 0 ? launch_status() : 0;
    }
    int cuddh_hip_trace_unpack_f64(int n, int n_half, const int *slot, const double *buf, double *v, void *s)
    {
        if (n > 0)
            hipLaunchKernelGGL((trace_unpack_kernel<double>), dim3(stream_grid(n, BLOCK)), dim3(BLOCK), 0, as_stream(s), n, n_half, slot, buf, v);
        return n > 0 ? launch_status() : 0;
    }
    int cuddh_hip_halo_pack_f64(int n, int n_half, const int *ids, double *v, double *buf, int clear, void *s)
    {
        if (n > 0)
            hipLaunchKernelGGL(halo_pack_kernel, dim3(stream_grid(n, BLOCK)), dim3(BLOCK), 0, as_stream(s), n, n_half, ids, v, reinterpret_cast<double2 *>(buf), clear);
        return n > 0 ? launch_status() : 0;
    }
    int cuddh_hip_halo_unpack_f64(int n, int n_half, const int *ids, const double *buf, double *v, int add, void *s)
    {
        if (n > 0)
            hipLaunchKernelGGL(halo_unpack_kernel, dim3(stream_grid(n, BLOCK)), dim3(BLOCK), 0, as_stream(s), n, n_half, ids, reinterpret_cast<const double2 *>(buf), v, add);
        return n > 0 ? launch_status() : 0;
    }
    int cuddh_hip_csr_sum_f64(int n_rows, const int *off, const int *src, const double *x, double *y, int accumulate, void *s)
    {
        if (n_rows > 0)
            hipLaunchKernelGGL(csr_sum_kernel, dim3(stream_grid(n_rows, BLOCK)), dim3(BLOCK), 0, as_stream(s), n_rows, off, src, x, y, accumulate);
        return n_rows > 0 ? launch_status() : 0;
    }
    int cuddh_hip_zero_indexed_f64(int n, const int *proj, double *x, void *s)
    {
        if (n <= 0)
            return 0;
        hipLaunchKernelGGL(zero_indexed_kernel, dim3(stream_grid(n, BLOCK)), dim3(BLOCK), 0, as_stream(s), n, proj, x);
        return launch_status();
    }
}
