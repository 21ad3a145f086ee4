// nfm_rt_mm.hip -- the real transforms of nfm_rt.hip for long axes (N up to NFM_RT_MAX_N) as a matrix product
// on the matrix cores:  y = diag(post) B diag(pre) x  with the same Plan, the same table of 2 cos / 2 sin in LDS
// and the same k-ordered fma chain per output; only the contraction differs.
//
// A workgroup of four waves owns kLines = 32 lines.  It stages them whole in LDS (pre applied on the way in), so
// `out` may alias `x`, then forms the ceil(N / 16) x 2 result tiles of 16 x 16 with v_mfma_*_16x16x4: wave w owns
// the output tiles w, w + 4, w + 8, w + 12 of both line tiles (8 independent accumulators), one k-step is 2 data
// reads + 4 coefficient gathers for 8 matrix instructions.  `post` is applied to the accumulators, which go
// straight to memory.
//   inner > 1   Y[k][l] = sum_n B[k][n] X[n][l]: the coefficients are the A operand, the result's lane index
//               (column) is the line, which runs along memory.  LDS image [n][32], the two halves of odd rows
//               swapped (conflict-free operand reads).
//   inner == 1  (axis last) Yt[l][k] = sum_n X[l][n] Bt[n][k]: the data is the A operand, the result's lane
//               index is k, which runs along memory.  LDS image [32][pitch], pitch = 2 mod 32.
// In both, lane (c = lane & 15, q = lane >> 4) feeds B[16 kt + c][4 step + q] and X[line 16 lt + c][4 step + q];
// the coefficient is tab[(a_k + n s_k) mod P], gathered with the incremental index of `lines<>`.  Rows n >= N of
// both operands and lines past the end of the batch are zeros (never read from memory, never written).
#include "nfm_rt_mm.hpp"

namespace nfm {
namespace rt {

constexpr int kLines = 32;  // lines per workgroup: two result tiles wide
constexpr int kWaves = 4;
constexpr int kKT = 4;      // output tiles per wave: kWaves * kKT * 16 = NFM_RT_MAX_N
constexpr int kLT = kLines / 16;
static_assert(kWaves * kKT * 16 >= NFM_RT_MAX_N, "every output of the longest line has a wave");

template <typename T>
struct Mfma;
template <>
struct Mfma<float> {
    typedef float acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mac(float a, float b, acc_t c)
    {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    // C/D: col = lane & 15, row = 4 (lane >> 4) + reg
    static __device__ __forceinline__ int row(int q, int r) { return 4 * q + r; }
};
template <>
struct Mfma<double> {
    typedef double acc_t __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ acc_t mac(double a, double b, acc_t c)
    {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    // the float64 instruction has its own C/D map: col = lane & 15, row = (lane >> 4) + 4 reg
    static __device__ __forceinline__ int row(int q, int r) { return q + 4 * r; }
};

// row pitch of the axis-last image: >= n4 and 2 mod 32, so that the 16 lines x 2 terms a half-wave reads sit on
// 32 different banks (bank pairs for float64)
__host__ __device__ constexpr int last_pitch(int n4) { return ((n4 - 2 + 31) & ~31) + 2; }

template <typename T>
struct Tile {
    const Plan &p;
    const T *tab, *xs;
    const int64_t *lbase;
    T *O;
    int64_t inner, l0;
    int nl, pitch, wave, lane;
};

// NJ output tiles x kLT line tiles of one wave: contraction over the staged terms, `post`, store
template <typename T, bool LAST, int NJ>
__device__ __forceinline__ void tiles(const Tile<T> &g)
{
    using M = Mfma<T>;
    using acc_t = typename M::acc_t;
    const int N = g.p.N, P = g.p.P;
    const int c = g.lane & 15, q = g.lane >> 4;
    const T *xp[kLT];
#pragma unroll
    for (int t = 0; t < kLT; ++t)
        xp[t] = g.xs + (LAST ? (16 * t + c) * g.pitch + q : q * kLines + ((16 * t + c) ^ ((q & 1) << 4)));
    const int xstep = LAST ? 4 : 4 * kLines;
    int idx[NJ], step[NJ];
    acc_t acc[NJ][kLT];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = 16 * (g.wave + kWaves * j) + c;
        const int kk = k < N ? k : N - 1; // (outputs past the end repeat the last one, unwritten)
        const int s = g.p.s1 * kk + g.p.s0;
        idx[j] = (g.p.a1 * kk + g.p.a0 + q * s) % P;
        step[j] = (4 * s) % P;
#pragma unroll
        for (int t = 0; t < kLT; ++t) acc[j][t] = acc_t{T(0), T(0), T(0), T(0)};
    }
    // one k-step: terms 4 i + q.  `live` is false only for the terms past N of the last step, whose
    // coefficients are zeros like the data they meet
    auto kstep = [&](bool live) {
        T d[kLT], cf[NJ];
#pragma unroll
        for (int t = 0; t < kLT; ++t) {
            d[t] = *xp[t];
            xp[t] += xstep;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            cf[j] = g.tab[idx[j]];
            idx[j] += step[j];
            if (idx[j] >= P) idx[j] -= P;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const T cj = live ? cf[j] : T(0);
#pragma unroll
            for (int t = 0; t < kLT; ++t)
                acc[j][t] = LAST ? M::mac(d[t], cj, acc[j][t]) : M::mac(cj, d[t], acc[j][t]);
        }
    };
    const int whole = N >> 2;
#pragma unroll 2
    for (int i = 0; i < whole; ++i) kstep(true);
    if (N & 3) kstep(q < (N & 3));

    const T post_first = (T)g.p.post_first, post_mid = (T)g.p.post_mid, post_last = (T)g.p.post_last;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
        for (int t = 0; t < kLT; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = M::row(q, r);
                const int k = 16 * (g.wave + kWaves * j) + (LAST ? c : row), line = 16 * t + (LAST ? row : c);
                if (k >= N) continue;
                const T y = acc[j][t][r] * (k == 0 ? post_first : (k == N - 1 ? post_last : post_mid));
                if constexpr (LAST) {
                    if (line < g.nl) NFM_STG(y, g.O + (g.l0 + line) * N + k);
                } else {
                    const int64_t base = g.lbase[line];
                    if (base >= 0) NFM_STG(y, g.O + base + k * g.inner);
                }
            }
        }
    }
}

template <typename T, bool LAST>
__global__ __launch_bounds__(kWaves * 64) void rt_mm_kernel(const Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.p.N, P = a.p.P;
    const int N4 = (N + 3) & ~3; // whole k-steps
    T *tab = reinterpret_cast<T *>(smem);
    T *xs = tab + table_len(P);
    for (int m = tid; m < P; m += kWaves * 64) tab[m] = table_entry<T>(a.p, m);
    const T pre_first = (T)a.p.pre_first, pre_last = (T)a.p.pre_last;
    const T *X = static_cast<const T *>(a.x);
    T *O = static_cast<T *>(a.o);
    const int64_t total = LAST ? a.outer : a.outer * a.inner;
    const int64_t l0 = (int64_t)blockIdx.x * kLines;
    const int nl = (int)(total - l0 < kLines ? total - l0 : kLines);
    const int pitch = last_pitch(N4);
    int64_t *lbase = reinterpret_cast<int64_t *>(xs + N4 * kLines); // inner > 1: where a line starts, -1: no line

    // stage the lines: every term of every line of the tile, zeros where there is nothing
    if constexpr (LAST) {
        for (int line = wave; line < kLines; line += kWaves)
            for (int n = lane; n < N4; n += 64) {
                T v = T(0);
                if (line < nl && n < N) {
                    v = NFM_LDG(X + (l0 + line) * N + n);
                    if (n == 0) v *= pre_first;
                    if (n == N - 1) v *= pre_last;
                }
                xs[line * pitch + n] = v;
            }
    } else {
        const int line = tid & (kLines - 1);
        const bool live = line < nl;
        const int64_t g = live ? l0 + line : 0, o = g / a.inner;
        const int64_t base = o * N * a.inner + (g - o * a.inner);
        if (tid < kLines) lbase[line] = live ? base : -1;
        for (int n = tid / kLines; n < N4; n += kWaves * 64 / kLines) {
            T v = T(0);
            if (live && n < N) {
                v = NFM_LDG(X + base + n * a.inner);
                if (n == 0) v *= pre_first;
                if (n == N - 1) v *= pre_last;
            }
            xs[n * kLines + (line ^ ((n & 1) << 4))] = v;
        }
    }
    __syncthreads();

    // the tiles this wave owns: a switch on a wave-uniform count keeps the accumulators statically indexed and
    // the k-loop free of branches
    const int nkt = (N + 15) >> 4;
    const int nj = nkt > wave ? (nkt - wave + kWaves - 1) / kWaves : 0;
    const Tile<T> g{a.p, tab, xs, lbase, O, a.inner, l0, nl, pitch, wave, lane};
    switch (nj) {
    case 1: tiles<T, LAST, 1>(g); break;
    case 2: tiles<T, LAST, 2>(g); break;
    case 3: tiles<T, LAST, 3>(g); break;
    case 4: tiles<T, LAST, 4>(g); break;
    default: break;
    }
}

template <typename T, bool LAST>
static int launch_mm(const Args &a, hipStream_t st)
{
    const int n4 = (a.p.N + 3) & ~3;
    const size_t image = LAST ? (size_t)kLines * last_pitch(n4) * sizeof(T)
                              : (size_t)kLines * n4 * sizeof(T) + kLines * sizeof(int64_t);
    const size_t lds = (size_t)table_len(a.p.P) * sizeof(T) + image;
    if (lds > kLdsOptIn) return NFM_ESIZE;
    if (lds > kLdsPlain) {
        static std::atomic<uint64_t> have{0};
        const int rc = lds_opt_in(have, reinterpret_cast<const void *>(&rt_mm_kernel<T, LAST>), kLdsOptIn);
        if (rc != NFM_OK) return rc;
    }
    const int64_t total = LAST ? a.outer : a.outer * a.inner;
    const int64_t blocks = (total + kLines - 1) / kLines;
    if (blocks > 0x7fffffffLL) return NFM_ESIZE;
    hipLaunchKernelGGL((rt_mm_kernel<T, LAST>), dim3((unsigned)blocks), dim3(kWaves * 64), lds, st, a);
    return launch_status();
}

int dispatch_mm(int dtype, const Args &a, void *stream)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return a.inner == 1 ? launch_mm<T, true>(a, st) : launch_mm<T, false>(a, st);
    });
}

} // namespace rt
} // namespace nfm
