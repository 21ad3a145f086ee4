// nfm_reduce.hip -- NaN-omitting reductions (reference `reduce.py`).
//
// Full reduction (`dim=None`): the reference makes up to four passes over memory
// (clone, isnan, masked_fill, sum: reduce.py:502-510); here it is ONE streaming pass.
//   kernel 1: 2048 workgroups x 256 lanes grid-stride over 16-byte vectors, four
//             independent loads in flight per lane, NaN -> identity by select,
//             per-lane accumulators (double for sums), 64-lane wavefront
//             shuffle-reduce, one LDS hop across the 4 waves, one partial per workgroup;
//   kernel 2: one workgroup folds the 2048 partials in the same fixed order.
// The launch geometry never depends on n, so results are bitwise reproducible.
#include "nfm_reduce_common.hpp"

namespace nfm {


template <int OP>
__device__ __forceinline__ double block_reduce(double v, double *lds)
{
    v = wave_reduce<OP>(v);
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    constexpr int nw = kRedThreads / kWave;
    double r = RedOp<OP>::identity();
    if (threadIdx.x == 0) {
        r = lds[0];
#pragma unroll
        for (int w = 1; w < nw; ++w) r = RedOp<OP>::merge(r, lds[w]);
    }
    return r; // valid in thread 0
}

template <typename T, int OP>
__global__ __launch_bounds__(kRedThreads) void reduce_all_k1(const T *__restrict__ x, int64_t n,
                                                              double *__restrict__ partial)
{
    using V = typename VecOf<T>::type;
    constexpr int VEC = VecOf<T>::N;
    __shared__ double lds[kRedThreads / kWave];

    // split [0, n) into an unaligned head, 16-byte vectors, and a tail
    const uintptr_t addr = reinterpret_cast<uintptr_t>(x);
    int64_t head = ((16 - (addr & 15)) & 15) / (int64_t)sizeof(T);
    if (head > n) head = n;
    const int64_t nvec = (n - head) / VEC;
    const int64_t tail0 = head + nvec * VEC;
    const V *xv = reinterpret_cast<const V *>(x + head);

    double a0 = RedOp<OP>::identity(), a1 = a0, a2 = a0, a3 = a0;
    const int64_t stride = (int64_t)gridDim.x * kRedThreads;
    int64_t q = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
    for (; q + 3 * stride < nvec; q += 4 * stride) {
        const V v0 = __builtin_nontemporal_load(xv + q);
        const V v1 = __builtin_nontemporal_load(xv + q + stride);
        const V v2 = __builtin_nontemporal_load(xv + q + 2 * stride);
        const V v3 = __builtin_nontemporal_load(xv + q + 3 * stride);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            RedOp<OP>::fold(a0, v0[k]);
            RedOp<OP>::fold(a1, v1[k]);
            RedOp<OP>::fold(a2, v2[k]);
            RedOp<OP>::fold(a3, v3[k]);
        }
    }
    for (; q < nvec; q += stride) {
        const V v0 = xv[q];
#pragma unroll
        for (int k = 0; k < VEC; ++k) RedOp<OP>::fold(a0, v0[k]);
    }
    // head and tail elements (fewer than 2 * VEC): one lane each, first workgroup
    const int64_t gid = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
    if (gid < head) RedOp<OP>::fold(a1, x[gid]);
    if (gid < n - tail0) RedOp<OP>::fold(a2, x[tail0 + gid]);

    double acc = RedOp<OP>::merge(RedOp<OP>::merge(a0, a1), RedOp<OP>::merge(a2, a3));
    acc = block_reduce<OP>(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

template <int OP>
__global__ __launch_bounds__(kRedThreads) void reduce_all_k2(const double *__restrict__ partial, int nparts,
                                                              void *out, int out_dtype)
{
    __shared__ double lds[kRedThreads / kWave];
    double acc = RedOp<OP>::identity();
    for (int p = threadIdx.x; p < nparts; p += kRedThreads) acc = RedOp<OP>::merge(acc, partial[p]);
    acc = block_reduce<OP>(acc, lds);
    if (threadIdx.x == 0) {
        if (out_dtype == NFM_F32) *static_cast<float *>(out) = (float)acc;
        else *static_cast<double *>(out) = acc;
    }
}

// moments of the whole array: the streaming structure of reduce_all_k1 with one MomCore per load in
// flight; a workgroup leaves [n, s, q, K] and the second kernel merges the workgroups' records
template <typename T>
__device__ __forceinline__ MomCore<T> mom_block(MomCore<T> t, MomCore<T> *lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t.merge(t.shfl(off));
    if (threadIdx.x % kWave == 0) lds[threadIdx.x / kWave] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        t = lds[0];
        for (int w = 1; w < kRedThreads / kWave; ++w) t.merge(lds[w]);
    }
    return t; // valid in thread 0
}

// fold one vector / one element; `unset`: the accumulator has seen no finite value yet and looks for
// its shift in what it is about to fold (MomCore::seed)
template <typename T>
__device__ __forceinline__ void fold_vec(MomCore<T> &m, bool &unset, typename VecOf<T>::type v)
{
    constexpr int VEC = VecOf<T>::N;
    T c[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) c[k] = v[k];
    if (unset) unset = m.seed(c);
#pragma unroll
    for (int k = 0; k < VEC; ++k) m.fold(c[k]);
}
template <typename T>
__device__ __forceinline__ void fold_one(MomCore<T> &m, bool &unset, T v)
{
    const T c[1] = {v};
    if (unset) unset = m.seed(c);
    m.fold(v);
}

template <typename T>
__global__ __launch_bounds__(kRedThreads) void moments_all_k1(const T *__restrict__ x, int64_t n,
                                                               double *__restrict__ partial)
{
    using V = typename VecOf<T>::type;
    constexpr int VEC = VecOf<T>::N;
    __shared__ MomCore<T> lds[kRedThreads / kWave];
    // same streaming structure as reduce_all_k1: unaligned head, 16-byte vectors, tail
    const uintptr_t addr = reinterpret_cast<uintptr_t>(x);
    int64_t head = ((16 - (addr & 15)) & 15) / (int64_t)sizeof(T);
    if (head > n) head = n;
    const int64_t nvec = (n - head) / VEC;
    const int64_t tail0 = head + nvec * VEC;
    const V *xv = reinterpret_cast<const V *>(x + head);
    MomCore<T> m, m1, m2, m3;
    m.init(x, n, 1);
    m1 = m2 = m3 = m;
    bool u = m.unset(), u1 = u, u2 = u, u3 = u;
    const int64_t stride = (int64_t)gridDim.x * kRedThreads;
    int64_t q = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
    for (; q + 3 * stride < nvec; q += 4 * stride) {
        const V v0 = __builtin_nontemporal_load(xv + q);
        const V v1 = __builtin_nontemporal_load(xv + q + stride);
        const V v2 = __builtin_nontemporal_load(xv + q + 2 * stride);
        const V v3 = __builtin_nontemporal_load(xv + q + 3 * stride);
        fold_vec(m, u, v0);
        fold_vec(m1, u1, v1);
        fold_vec(m2, u2, v2);
        fold_vec(m3, u3, v3);
    }
    for (; q < nvec; q += stride) fold_vec(m, u, xv[q]);
    const int64_t gid = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
    if (gid < head) fold_one(m1, u1, x[gid]);
    if (gid < n - tail0) fold_one(m2, u2, x[tail0 + gid]);
    m.merge(m1);
    m2.merge(m3);
    m.merge(m2);
    m = mom_block(m, lds);
    if (threadIdx.x == 0) m.save(partial + 4 * blockIdx.x);
}

template <typename T>
__global__ __launch_bounds__(kRedThreads) void moments_all_k2(const double *__restrict__ partial, int nparts,
                                                               double *out)
{
    __shared__ MomCore<T> lds[kRedThreads / kWave];
    MomCore<T> m;
    m.init_empty();
    for (int p = threadIdx.x; p < nparts; p += kRedThreads) {
        MomCore<T> u;
        u.load(partial + 4 * p);
        m.merge(u);
    }
    m = mom_block(m, lds);
    if (threadIdx.x == 0) m.save(out);
}

template <typename T, int OP>
static int reduce_all_t(int out_dtype, int64_t n, const void *x, void *ws, void *out, hipStream_t s)
{
    double *partial = static_cast<double *>(ws);
    hipLaunchKernelGGL((reduce_all_k1<T, OP>), dim3(kRedBlocks), dim3(kRedThreads), 0, s,
                       static_cast<const T *>(x), n, partial);
    hipLaunchKernelGGL((reduce_all_k2<OP>), dim3(1), dim3(kRedThreads), 0, s, partial, kRedBlocks, out, out_dtype);
    return launch_status();
}

// full-reduction moments (called by nfm_reduce_moments / nfm_reduce_stat in nfm_reduce_dim.hip)
int moments_all_launch(int dtype, const void *x, int64_t n, void *workspace, double *out, hipStream_t s)
{
    double *partial = static_cast<double *>(workspace);
    if (dtype == NFM_F32) {
        hipLaunchKernelGGL((moments_all_k1<float>), dim3(kRedBlocks), dim3(kRedThreads), 0, s,
                           static_cast<const float *>(x), n, partial);
        hipLaunchKernelGGL((moments_all_k2<float>), dim3(1), dim3(kRedThreads), 0, s, partial, kRedBlocks, out);
    } else {
        hipLaunchKernelGGL((moments_all_k1<double>), dim3(kRedBlocks), dim3(kRedThreads), 0, s,
                           static_cast<const double *>(x), n, partial);
        hipLaunchKernelGGL((moments_all_k2<double>), dim3(1), dim3(kRedThreads), 0, s, partial, kRedBlocks, out);
    }
    return launch_status();
}

} // namespace nfm

using namespace nfm;

extern "C" {

size_t nfm_reduce_workspace_bytes(void) { return (size_t)kRedBlocks * 4 * sizeof(double); } // moments: [n, s, q, K] per workgroup

int nfm_reduce_all(int dtype, int op, int out_dtype, int64_t n, const void *x, void *workspace,
                   size_t workspace_bytes, void *out, void *stream)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (out_dtype != NFM_F32 && out_dtype != NFM_F64) return NFM_EDTYPE;
    if (n < 0 || out == nullptr || workspace == nullptr || (n > 0 && x == nullptr)) return NFM_EINVAL;
    if (workspace_bytes < nfm_reduce_workspace_bytes()) return NFM_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(x) % (dtype == NFM_F32 ? 4 : 8) != 0) return NFM_EALIGN;
    if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) return NFM_EALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == NFM_F32) {
        NFM_SWITCH_OP(op, return (reduce_all_t<float, OP>(out_dtype, n, x, workspace, out, s)))
    } else {
        NFM_SWITCH_OP(op, return (reduce_all_t<double, OP>(out_dtype, n, x, workspace, out, s)))
    }
    return NFM_EINVAL;
}

const char *nfm_strerror(int code)
{
    switch (code) {
    case NFM_OK: return "success";
    case NFM_EINVAL: return "invalid argument (null pointer, negative size or bad flag)";
    case NFM_EDTYPE: return "unsupported dtype code";
    case NFM_ESIZE: return "matrix order outside 1..16 or batch too large";
    case NFM_EALIGN: return "pointer not aligned to the element size";
    case NFM_EWORKSPACE: return "workspace too small";
    case NFM_RT_EFALLBACK: return "line longer than the transform kernels serve";
    default: return code > 0 ? hipGetErrorString(static_cast<hipError_t>(code)) : "unknown error";
    }
}

int nfm_version(void) { return NFM_VERSION; }

} // extern "C"
