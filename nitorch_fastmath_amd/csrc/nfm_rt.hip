// nfm_rt.hip -- DCT / DST of types I, II, III along the middle axis of an (outer, N, inner) view (reference
// `realtransforms.py`), one line per lane as a direct sum: every input element is read from memory once,
// every output element written once, `out` may alias `x` (a workgroup holds its lines before it writes).
//   inner > 1   lanes run along `inner`; a lane owns VEC neighbouring lines (16-byte accesses) when the
//               vector width divides `inner`, one line otherwise.  The lines sit in LDS as [n][lane][VEC]
//               (lane-major columns: conflict-free), outputs go straight to memory.
//   inner == 1  (axis last) a tile of contiguous lines goes through LDS (tile_in / tile_out, odd row pitch),
//               the outputs through a second image.
// Each workgroup builds the table of 2 cos / 2 sin(pi m / D) in LDS in its prologue; the transform reads it at
// wave-uniform addresses.  N is a kernel argument: six kernels in all.  The arithmetic is in nfm_rt_ops.hpp.
#include "nfm_rt_mm.hpp"
#include "nfm_simplex_ops.hpp" // tile_in / tile_out

namespace nfm {
namespace rt {

using simplex::tile_in;
using simplex::tile_out;

// lengths the kernels are dispatched for (nfm_rt_max_len); longer axes are the caller's (NFM_RT_EFALLBACK)
#ifndef NFM_RT_MAX_LEN_F32
#define NFM_RT_MAX_LEN_F32 64
#endif
#ifndef NFM_RT_MAX_LEN_F64
#define NFM_RT_MAX_LEN_F64 64
#endif
static_assert(NFM_RT_MAX_LEN_F32 >= 1 && NFM_RT_MAX_LEN_F32 <= NFM_RT_MAX_N, "float32 cap");
static_assert(NFM_RT_MAX_LEN_F64 >= 1 && NFM_RT_MAX_LEN_F64 <= NFM_RT_MAX_N, "float64 cap");

// lengths the facade routes to the matrix-instruction kernel (nfm_rt_mm_max_len): per dtype the largest of
// {128, 256} at which it is not slower than the torch.fft composition in both layouts, 64 (route off) if neither
#ifndef NFM_RT_MM_MAX_LEN_F32
#define NFM_RT_MM_MAX_LEN_F32 256
#endif
#ifndef NFM_RT_MM_MAX_LEN_F64
#define NFM_RT_MM_MAX_LEN_F64 256
#endif
constexpr bool mm_cap_ok(int n) { return n == 64 || n == 128 || n == 256; }
static_assert(mm_cap_ok(NFM_RT_MM_MAX_LEN_F32) && mm_cap_ok(NFM_RT_MM_MAX_LEN_F64), "routing cap: 64, 128 or 256");

template <typename T, int VEC>
struct Pack {
    typedef T type __attribute__((ext_vector_type(VEC)));                        // LDS side
    typedef T gtype __attribute__((ext_vector_type(VEC), aligned(sizeof(T))));   // element-aligned: global side
};

// terms of VEC lines in LDS, `stride` elements from one term to the next
template <typename T, int VEC>
struct LdsLines {
    const T *base;
    int stride;
    __device__ __forceinline__ void get(int n, T (&v)[VEC]) const
    {
        if constexpr (VEC == 1) {
            v[0] = base[n * stride];
        } else {
            const typename Pack<T, VEC>::type w = *reinterpret_cast<const typename Pack<T, VEC>::type *>(base + n * stride);
#pragma unroll
            for (int k = 0; k < VEC; ++k) v[k] = w[k];
        }
    }
};

template <typename T>
struct LdsRowOut {
    T *row;
    __device__ __forceinline__ void put(int k, const T (&v)[1]) { row[k] = v[0]; }
};

template <typename T, int VEC>
struct GlobalOut {
    T *O;
    int64_t inner;
    __device__ __forceinline__ void put(int k, const T (&v)[VEC])
    {
        if constexpr (VEC == 1) {
            NFM_STG(v[0], O + k * inner);
        } else {
            using G = typename Pack<T, VEC>::gtype;
            G w;
#pragma unroll
            for (int j = 0; j < VEC; ++j) w[j] = v[j];
            NFM_STG(w, reinterpret_cast<G *>(O + k * inner));
        }
    }
};

template <typename T, int VEC, bool LAST>
__global__ __launch_bounds__(256) void rt_kernel(const Args a)
{
    static_assert(!LAST || VEC == 1, "axis-last tiles hold one line per lane");
    constexpr int KB = VEC == 1 ? 8 : (VEC == 2 ? 4 : 4);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = a.p.N;
    T *tab = reinterpret_cast<T *>(smem);
    T *xs = tab + table_len(a.p.P);
    for (int m = tid; m < a.p.P; m += nt) tab[m] = table_entry<T>(a.p, m);
    const T pre_first = (T)a.p.pre_first, pre_last = (T)a.p.pre_last;
    if constexpr (LAST) {
        const int pitch = N | 1;
        T *ys = xs + nt * pitch;
        const int64_t v0 = (int64_t)blockIdx.x * nt;
        const int nv = (int)(a.outer - v0 < nt ? a.outer - v0 : nt);
        tile_in(xs, static_cast<const T *>(a.x) + v0 * N, N, pitch, nv * N, nt);
        __syncthreads();
        if (tid < nv) {
            T *row = xs + tid * pitch; // lane-owned
            row[0] *= pre_first;
            row[N - 1] *= pre_last;
            const LdsLines<T, 1> in{row, 1};
            LdsRowOut<T> out{ys + tid * pitch};
            lines<T, 1, KB>(a.p, tab, in, out);
        }
        __syncthreads();
        tile_out(ys, static_cast<T *>(a.o) + v0 * N, N, pitch, nv * N, nt);
    } else {
        const int64_t ipv = a.inner / VEC; // VEC divides inner
        const int64_t gid = (int64_t)blockIdx.x * nt + tid;
        const bool live = gid < a.outer * ipv;
        const int64_t o = live ? gid / ipv : 0, i = live ? (gid - o * ipv) * VEC : 0;
        T *mine = xs + tid * VEC; // term n of this lane's lines at mine[n * nt * VEC]: lane-owned
        if (live) {
            const T *A = static_cast<const T *>(a.x) + o * N * a.inner + i;
            for (int n = 0; n < N; ++n) {
                const T f = (n == 0 ? pre_first : T(1)) * (n == N - 1 ? pre_last : T(1));
                if constexpr (VEC == 1) {
                    mine[n * nt] = NFM_LDG(A + n * a.inner) * f;
                } else {
                    using G = typename Pack<T, VEC>::gtype;
                    using V = typename Pack<T, VEC>::type;
                    const G w = NFM_LDG(reinterpret_cast<const G *>(A + n * a.inner));
                    V s;
#pragma unroll
                    for (int k = 0; k < VEC; ++k) s[k] = w[k] * f;
                    *reinterpret_cast<V *>(mine + n * nt * VEC) = s;
                }
            }
        }
        __syncthreads(); // the table
        if (live) {
            const LdsLines<T, VEC> in{mine, nt * VEC};
            GlobalOut<T, VEC> out{static_cast<T *>(a.o) + o * N * a.inner + i, a.inner};
            lines<T, VEC, KB>(a.p, tab, in, out);
        }
    }
}

// lanes per workgroup for `per_lane` bytes of LDS a lane plus `fixed` for the table: 0 when nothing fits
static int pick_lanes(size_t per_lane, size_t fixed, bool &opt_in)
{
    opt_in = false;
    for (int nt : {256, 128, 64})
        if (fixed + nt * per_lane <= 40 * 1024) return nt;
    for (int nt : {64, 32, 16})
        if (fixed + nt * per_lane <= kLdsPlain) return nt;
    opt_in = true;
    for (int nt : {64, 32, 16})
        if (fixed + nt * per_lane <= kLdsOptIn) return nt;
    return 0;
}

template <typename T, int VEC, bool LAST>
static int launch(const Args &a, int64_t units, size_t per_lane, hipStream_t st)
{
    const size_t fixed = (size_t)table_len(a.p.P) * sizeof(T);
    bool opt_in;
    const int nt = pick_lanes(per_lane, fixed, opt_in);
    if (nt == 0) return NFM_ESIZE;
    if (opt_in) {
        static std::atomic<uint64_t> have{0};
        const int rc = lds_opt_in(have, reinterpret_cast<const void *>(&rt_kernel<T, VEC, LAST>), kLdsOptIn);
        if (rc != NFM_OK) return rc;
    }
    const int64_t blocks = (units + nt - 1) / nt;
    if (blocks > 0x7fffffffLL) return NFM_ESIZE;
    hipLaunchKernelGGL((rt_kernel<T, VEC, LAST>), dim3((unsigned)blocks), dim3(nt), fixed + nt * per_lane, st, a);
    return launch_status();
}

template <typename T>
static int dispatch(const Args &a, void *stream)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr int kVec = VecOf<T>::N;
    const size_t line = (size_t)a.p.N * sizeof(T);
    if (a.inner == 1) return launch<T, 1, true>(a, a.outer, 2 * (size_t)(a.p.N | 1) * sizeof(T), st);
    if (a.inner % kVec == 0) return launch<T, kVec, false>(a, a.outer * (a.inner / kVec), kVec * line, st);
    return launch<T, 1, false>(a, a.outer * a.inner, line, st);
}

// the same lines on the calling thread, for tensors in host memory
template <typename T>
struct HostIn {
    const T *buf;
    void get(int n, T (&v)[1]) const { v[0] = buf[n]; }
};
template <typename T>
struct HostOut {
    T *buf;
    void put(int k, const T (&v)[1]) { buf[k] = v[0]; }
};

template <typename T>
static int run_host(const Args &a)
{
    const int N = a.p.N;
    T tab[2 * 2 * NFM_RT_MAX_N + 4], in[NFM_RT_MAX_N], res[NFM_RT_MAX_N];
    for (int m = 0; m < a.p.P; ++m) tab[m] = table_entry<T>(a.p, m);
    const T *X = static_cast<const T *>(a.x);
    T *O = static_cast<T *>(a.o);
    for (int64_t o = 0; o < a.outer; ++o)
        for (int64_t i = 0; i < a.inner; ++i) {
            const int64_t at = o * N * a.inner + i;
            for (int n = 0; n < N; ++n) in[n] = X[at + n * a.inner];
            in[0] *= (T)a.p.pre_first;
            in[N - 1] *= (T)a.p.pre_last;
            const HostIn<T> hi{in};
            HostOut<T> ho{res};
            lines<T, 1, 8>(a.p, tab, hi, ho);
            for (int k = 0; k < N; ++k) O[at + k * a.inner] = res[k];
        }
    return NFM_OK;
}

static int max_len(int dtype) { return dtype == NFM_F64 ? NFM_RT_MAX_LEN_F64 : NFM_RT_MAX_LEN_F32; }

enum Path { kLane, kHost, kMm }; // who runs the checked call; only the lane kernels have a cap below NFM_RT_MAX_N

static int entry(int dtype, int kind, int type, int norm, int transpose, int64_t N, int64_t outer, int64_t inner,
                 const void *x, void *out, Path path, void *stream)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (N < 0 || outer < 0 || inner < 0) return NFM_EINVAL;
    if (kind != NFM_RT_DCT && kind != NFM_RT_DST) return NFM_EINVAL;
    if (type < 1 || type > 3) return NFM_EINVAL;
    if (norm < NFM_RT_BACKWARD || norm > NFM_RT_ORTHO_SCIPY) return NFM_EINVAL;
    if (transpose != 0 && transpose != 1) return NFM_EINVAL;
    if (N < 1 || (N == 1 && kind == NFM_RT_DCT && type == 1)) return NFM_EINVAL;
    if (outer > 0 && inner > 0 && (outer > INT64_MAX / inner || outer * inner > INT64_MAX / N)) return NFM_ESIZE;
    if (N > (path == kLane ? max_len(dtype) : NFM_RT_MAX_N)) return NFM_RT_EFALLBACK;
    const bool nonempty = outer > 0 && inner > 0;
    const size_t elem = dtype == NFM_F32 ? 4 : 8;
    for (const void *ptr : {x, static_cast<const void *>(out)}) {
        if (ptr == nullptr && nonempty) return NFM_EINVAL;
        if (reinterpret_cast<uintptr_t>(ptr) % elem != 0) return NFM_EALIGN;
    }
    if (!nonempty) return NFM_OK;
    Args a;
    a.p = make_plan(kind, type, norm, transpose, (int)N);
    a.outer = outer, a.inner = inner;
    a.x = x, a.o = out;
    if (path == kHost) return by_dtype(dtype, [&](auto t) { return run_host<decltype(t)>(a); });
    if (path == kMm) return dispatch_mm(dtype, a, stream);
    return by_dtype(dtype, [&](auto t) { return dispatch<decltype(t)>(a, stream); });
}

} // namespace rt
} // namespace nfm

using namespace nfm;

extern "C" {

int nfm_rt_max_len(int dtype)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    return rt::max_len(dtype);
}

int nfm_rt_transform(int dtype, int kind, int type, int norm, int transpose, int64_t N, int64_t outer, int64_t inner,
                     const void *x, void *out, void *stream)
{
    return rt::entry(dtype, kind, type, norm, transpose, N, outer, inner, x, out, rt::kLane, stream);
}

int nfm_rt_transform_host(int dtype, int kind, int type, int norm, int transpose, int64_t N, int64_t outer,
                          int64_t inner, const void *x, void *out)
{
    return rt::entry(dtype, kind, type, norm, transpose, N, outer, inner, x, out, rt::kHost, nullptr);
}

int nfm_rt_mm_max_len(int dtype)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    return dtype == NFM_F64 ? NFM_RT_MM_MAX_LEN_F64 : NFM_RT_MM_MAX_LEN_F32;
}

int nfm_rt_transform_mm(int dtype, int kind, int type, int norm, int transpose, int64_t N, int64_t outer,
                        int64_t inner, const void *x, void *out, void *stream)
{
    return rt::entry(dtype, kind, type, norm, transpose, N, outer, inner, x, out, rt::kMm, stream);
}

} // extern "C"
