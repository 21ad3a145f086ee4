// nfm_stochastic.hip -- the library side of the stochastic estimators (reference `stochastic.py`):
// trace estimation (Hutchinson, Hutch++), power iteration.  The operator belongs to the caller; what the
// reference does AROUND it -- drawing probes, inner products, the deflation of Hutch++, the QR of a tall
// n x m matrix, normalising -- is streaming work over whole fields, and here it is three kernels:
//
//   nfm_stoch_fill     counter-based +-1 / normal probes (Philox4x32-10): an element depends on
//                      (seed, element index) alone, one pass, 16-byte stores;
//   nfm_stoch_gram     out[j q + k] (+)= <X_j, Y_k> for up to 8 x 8 vectors, every vector read ONCE,
//                      products and sums in double, two stages with a fixed plan: bitwise reproducible;
//   nfm_stoch_combine  Z_k = sigma (Y_k - sum_j X_j C[j q + k]), C and sigma read from DEVICE memory
//                      (no host round trip between a gram and the update that uses it).
//
// Vectors are addressed by element index, in slots of one 16-byte vector (4 floats / 2 doubles), through
// the element-aligned vector type (VecOf::gtype): a lane folds the same elements in the same order
// whatever the alignment of the pointers, so a row of an odd-length stack gives the bits of an aligned copy.
#include "nfm_reduce_common.hpp"
#include "nfm_stochastic_ops.hpp"

namespace nfm {
namespace stoch {

constexpr int kThreads = kRedThreads;
constexpr int kMaxVecs = NFM_STOCH_MAX_VECS;

// ------------------------------------------------------------------------------------------- fill
// A workgroup produces a chunk of the element axis into LDS, one Philox call per unit (Rademacher: 128
// elements = 4 words of bits; Gaussian: 4 elements), then streams it out with aligned 16-byte stores.
// Chunks are aligned in ELEMENT space (to the unit), stores in ADDRESS space: a vector may start anywhere
// in a unit and run into the next one, so a chunk holds one unit more than it owns.
template <typename T, int KIND>
struct Gen;

template <typename T>
struct Gen<T, NFM_STOCH_RADEMACHER> {
    using L = uint32_t;
    static constexpr int UE = 128, kUnits = kThreads, kLdsPerUnit = 4;
    static __device__ __forceinline__ void produce(L *lds, int u, uint64_t unit, uint32_t k0, uint32_t k1)
    {
        const U4 w = rademacher_group(unit, k0, k1);
        lds[4 * u + 0] = w.w0;
        lds[4 * u + 1] = w.w1;
        lds[4 * u + 2] = w.w2;
        lds[4 * u + 3] = w.w3;
    }
    static __device__ __forceinline__ T fetch(const L *lds, int p) { return sign_of_bit<T>((lds[p >> 5] >> (p & 31)) & 1u); }
    static __device__ __forceinline__ T single(uint64_t e, uint32_t k0, uint32_t k1)
    {
        const U4 w = rademacher_group(e >> 7, k0, k1);
        const int b = (int)(e & 127), wi = b >> 5;
        const uint32_t word = wi == 0 ? w.w0 : (wi == 1 ? w.w1 : (wi == 2 ? w.w2 : w.w3));
        return sign_of_bit<T>((word >> (b & 31)) & 1u);
    }
};

template <typename T>
struct Gen<T, NFM_STOCH_GAUSSIAN> {
    using L = T;
    static constexpr int UE = 4, kUnits = 2 * kThreads, kLdsPerUnit = 4;
    static __device__ __forceinline__ void produce(L *lds, int u, uint64_t unit, uint32_t k0, uint32_t k1)
    {
        T e0, e1, e2, e3;
        gaussian_quad<T>(unit, k0, k1, e0, e1, e2, e3);
        lds[4 * u + 0] = e0;
        lds[4 * u + 1] = e1;
        lds[4 * u + 2] = e2;
        lds[4 * u + 3] = e3;
    }
    static __device__ __forceinline__ T fetch(const L *lds, int p) { return lds[p]; }
    static __device__ __forceinline__ T single(uint64_t e, uint32_t k0, uint32_t k1)
    {
        T e0, e1, e2, e3;
        gaussian_quad<T>(e >> 2, k0, k1, e0, e1, e2, e3);
        const int b = (int)(e & 3);
        return b == 0 ? e0 : (b == 1 ? e1 : (b == 2 ? e2 : e3));
    }
};

template <typename T, int KIND>
__global__ __launch_bounds__(kThreads) void fill_kernel(T *out, int64_t n, uint64_t offset, uint32_t k0, uint32_t k1,
                                                         int64_t nchunks)
{
    using G = Gen<T, KIND>;
    using V = typename VecOf<T>::type;
    constexpr int VEC = VecOf<T>::N;
    constexpr int64_t CH = (int64_t)G::kUnits * G::UE; // elements a chunk owns
    __shared__ typename G::L lds[(G::kUnits + 1) * G::kLdsPerUnit];

    // [0, n) = unaligned head, 16-byte vectors, tail
    const uintptr_t addr = reinterpret_cast<uintptr_t>(out);
    int64_t head = ((16 - (addr & 15)) & 15) / (int64_t)sizeof(T);
    if (head > n) head = n;
    const int64_t nvec = (n - head) / VEC;
    const int64_t tail0 = head + nvec * VEC;
    V *ov = reinterpret_cast<V *>(out + head);
    const uint64_t ebase0 = offset & ~(uint64_t)(G::UE - 1);
    const uint64_t evec0 = offset + (uint64_t)head; // element index of the first vector

    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const uint64_t ebase = ebase0 + (uint64_t)c * CH;
        __syncthreads(); // the previous chunk has been read
        for (int u = threadIdx.x; u < G::kUnits + 1; u += kThreads) G::produce(lds, u, ebase / G::UE + u, k0, k1);
        __syncthreads();
        // the vectors whose FIRST element lies in [ebase, ebase + CH)
        const uint64_t eend = ebase + CH;
        const int64_t q_lo = ebase > evec0 ? (int64_t)((ebase - evec0 + VEC - 1) / VEC) : 0;
        int64_t q_hi = eend > evec0 ? (int64_t)((eend - evec0 + VEC - 1) / VEC) : 0;
        if (q_hi > nvec) q_hi = nvec;
        for (int64_t q = q_lo + threadIdx.x; q < q_hi; q += kThreads) {
            const int p = (int)(evec0 + (uint64_t)q * VEC - ebase); // 0 <= p < CH; p + VEC - 1 < CH + UE
            V v;
#pragma unroll
            for (int k = 0; k < VEC; ++k) v[k] = G::fetch(lds, p + k);
            NFM_STG(v, ov + q);
        }
    }
    // head and tail elements (fewer than 2 * VEC): one lane each, first workgroup
    if (blockIdx.x == 0) {
        const int64_t t = threadIdx.x;
        if (t < head) out[t] = G::single(offset + (uint64_t)t, k0, k1);
        if (t < n - tail0) out[tail0 + t] = G::single(offset + (uint64_t)(tail0 + t), k0, k1);
    }
}

template <typename T, int KIND>
static int fill_t(uint64_t seed, uint64_t offset, int64_t n, void *out, hipStream_t s)
{
    using G = Gen<T, KIND>;
    constexpr int64_t CH = (int64_t)G::kUnits * G::UE;
    const uint64_t lead = offset & (uint64_t)(G::UE - 1);
    const int64_t nchunks = (int64_t)((lead + (uint64_t)n + CH - 1) / CH);
    const int64_t grid = nchunks < (1 << 20) ? nchunks : (1 << 20);
    hipLaunchKernelGGL((fill_kernel<T, KIND>), dim3((unsigned)grid), dim3(kThreads), 0, s, static_cast<T *>(out), n, offset,
                       (uint32_t)seed, (uint32_t)(seed >> 32), nchunks);
    return launch_status();
}

// ------------------------------------------------------------------------------------------- gram
struct GramPtrs {
    const void *x[kMaxVecs];
    const void *y[kMaxVecs];
};

// one slot (VEC consecutive elements) of vector `ptr`; `left` < VEC: the last, partial slot (zeros past n)
template <typename T>
__device__ __forceinline__ typename VecOf<T>::type load_slot(const void *ptr, int64_t slot)
{
    using VG = typename VecOf<T>::gtype;
    return NFM_LDG(reinterpret_cast<const VG *>(static_cast<const T *>(ptr)) + slot);
}
template <typename T>
__device__ __forceinline__ typename VecOf<T>::type load_part(const void *ptr, int64_t slot, int left)
{
    constexpr int VEC = VecOf<T>::N;
    const T *p = static_cast<const T *>(ptr) + slot * VEC;
    typename VecOf<T>::type v;
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = e < left ? p[e] : T(0);
    return v;
}

template <typename T, int P, int Q>
__device__ __forceinline__ void gram_fold(double (&acc)[P][Q], const typename VecOf<T>::type (&xv)[P],
                                          const typename VecOf<T>::type (&yv)[Q])
{
    constexpr int VEC = VecOf<T>::N;
#pragma unroll
    for (int e = 0; e < VEC; ++e)
#pragma unroll
        for (int j = 0; j < P; ++j)
#pragma unroll
            for (int k = 0; k < Q; ++k) acc[j][k] = __builtin_fma((double)xv[j][e], (double)yv[k][e], acc[j][k]);
}

// stage 1: workgroup b leaves its P x Q partial sums at partial[(j Q + k) gridDim.x + b].  The form (P, Q)
// serves any p <= P, q <= Q: vectors past (p, q) are not read (their accumulators are never written out).
template <typename T, int P, int Q>
__global__ __launch_bounds__(kThreads) void gram_k1(GramPtrs a, int p, int q, int64_t n, double *__restrict__ partial)
{
    using V = typename VecOf<T>::type;
    constexpr int VEC = VecOf<T>::N;
    constexpr int U = (P + Q <= 2) ? 4 : ((P + Q <= 4) ? 2 : 1); // slots in flight per lane
    __shared__ double lds[P * Q * (kThreads / kWave)];
    double acc[P][Q];
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
        for (int k = 0; k < Q; ++k) acc[j][k] = 0.0;

    const int64_t nfull = n / VEC;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    int64_t s = gid;
    for (; s + (U - 1) * stride < nfull; s += U * stride) {
        V xv[U][P], yv[U][Q];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int j = 0; j < P; ++j) xv[u][j] = j < p ? load_slot<T>(a.x[j], s + u * stride) : V(T(0));
#pragma unroll
            for (int k = 0; k < Q; ++k) yv[u][k] = k < q ? load_slot<T>(a.y[k], s + u * stride) : V(T(0));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) gram_fold<T, P, Q>(acc, xv[u], yv[u]);
    }
    for (; s < nfull; s += stride) {
        V xv[P], yv[Q];
#pragma unroll
        for (int j = 0; j < P; ++j) xv[j] = j < p ? load_slot<T>(a.x[j], s) : V(T(0));
#pragma unroll
        for (int k = 0; k < Q; ++k) yv[k] = k < q ? load_slot<T>(a.y[k], s) : V(T(0));
        gram_fold<T, P, Q>(acc, xv, yv);
    }
    // the last, partial slot belongs to the lane whose turn it is
    const int left = (int)(n - nfull * VEC);
    if (left > 0 && gid == nfull % stride) {
        V xv[P], yv[Q];
#pragma unroll
        for (int j = 0; j < P; ++j) xv[j] = j < p ? load_part<T>(a.x[j], nfull, left) : V(T(0));
#pragma unroll
        for (int k = 0; k < Q; ++k) yv[k] = k < q ? load_part<T>(a.y[k], nfull, left) : V(T(0));
        gram_fold<T, P, Q>(acc, xv, yv);
    }

    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    constexpr int nw = kThreads / kWave;
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const double v = wave_reduce<NFM_RED_SUM>(acc[j][k]);
            if (lane == 0) lds[(j * Q + k) * nw + wave] = v;
        }
    __syncthreads();
    if (threadIdx.x < P * Q) {
        double r = lds[threadIdx.x * nw];
#pragma unroll
        for (int w = 1; w < nw; ++w) r += lds[threadIdx.x * nw + w];
        partial[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = r;
    }
}

// stage 2: one workgroup, a wave per output, the slabs in a fixed order
__global__ __launch_bounds__(kThreads) void gram_k2(const double *__restrict__ partial, int nblk, int Qf, int p, int q,
                                                     double *out, int accumulate)
{
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    for (int o = wave; o < p * q; o += kThreads / kWave) {
        const int j = o / q, k = o - j * q;
        const double *slab = partial + (int64_t)(j * Qf + k) * nblk;
        double acc = 0.0;
        for (int b = lane; b < nblk; b += kWave) acc += slab[b];
        acc = wave_reduce<NFM_RED_SUM>(acc);
        if (lane == 0) out[o] = accumulate ? out[o] + acc : acc;
    }
}

// the instantiated forms: P x 1 and P x P for P in {1, 2, 4, 8}
inline int form_of(int m) { return m <= 1 ? 1 : (m <= 2 ? 2 : (m <= 4 ? 4 : 8)); }

inline int gram_blocks(int64_t n, int vec)
{
    const int64_t slots = n / vec + 1;
    const int64_t b = (slots + kThreads - 1) / kThreads;
    return (int)(b < kRedBlocks ? b : kRedBlocks);
}

template <typename T, int P, int Q>
static void gram_launch(const GramPtrs &a, int p, int q, int64_t n, double *partial, int nblk, hipStream_t s)
{
    hipLaunchKernelGGL((gram_k1<T, P, Q>), dim3(nblk), dim3(kThreads), 0, s, a, p, q, n, partial);
}

template <typename T>
static int gram_t(int p, int q, int64_t n, const void *const *x, const void *const *y, void *ws, double *out,
                  int accumulate, hipStream_t s)
{
    GramPtrs a = {};
    // a single X against several Y: the roles swap (the outputs are the same q numbers in the same order)
    if (p == 1 && q > 1) {
        for (int k = 0; k < q; ++k) a.x[k] = y[k];
        a.y[0] = x[0];
        p = q;
        q = 1;
    } else {
        for (int j = 0; j < p; ++j) a.x[j] = x[j];
        for (int k = 0; k < q; ++k) a.y[k] = y[k];
    }
    double *partial = static_cast<double *>(ws);
    const int nblk = n > 0 ? gram_blocks(n, VecOf<T>::N) : 0;
    const int Pf = form_of(p > q ? p : q), Qf = q == 1 ? 1 : Pf;
    if (nblk > 0) {
        if (Qf == 1) {
            switch (Pf) {
            case 1: gram_launch<T, 1, 1>(a, p, q, n, partial, nblk, s); break;
            case 2: gram_launch<T, 2, 1>(a, p, q, n, partial, nblk, s); break;
            case 4: gram_launch<T, 4, 1>(a, p, q, n, partial, nblk, s); break;
            default: gram_launch<T, 8, 1>(a, p, q, n, partial, nblk, s); break;
            }
        } else {
            switch (Pf) {
            case 2: gram_launch<T, 2, 2>(a, p, q, n, partial, nblk, s); break;
            case 4: gram_launch<T, 4, 4>(a, p, q, n, partial, nblk, s); break;
            default: gram_launch<T, 8, 8>(a, p, q, n, partial, nblk, s); break;
            }
        }
    }
    hipLaunchKernelGGL(gram_k2, dim3(1), dim3(kThreads), 0, s, partial, nblk, Qf, p, q, out, accumulate);
    return launch_status();
}

// ---------------------------------------------------------------------------------------- combine
struct CombPtrs {
    const void *x[kMaxVecs];
    const void *y[kMaxVecs];
    void *z[kMaxVecs];
};

template <typename T>
__device__ __forceinline__ void store_slot(void *ptr, int64_t slot, typename VecOf<T>::type v)
{
    using VG = typename VecOf<T>::gtype;
    NFM_STG(static_cast<VG>(v), reinterpret_cast<VG *>(static_cast<T *>(ptr)) + slot);
}

// Z_k = sigma (Y_k - sum_j X_j C[j q + k]) on one slot; `left` < VEC: the partial slot, element by element
template <typename T, int P, int Q, bool PART>
__device__ __forceinline__ void combine_slot(const CombPtrs &a, int p, int q, int64_t slot, int left,
                                             const double (&cm)[P ? P : 1][Q], double sigma, bool drop)
{
    using V = typename VecOf<T>::type;
    constexpr int VEC = VecOf<T>::N;
    V xv[P ? P : 1], yv[Q];
#pragma unroll
    for (int j = 0; j < P; ++j)
        xv[j] = j < p ? (PART ? load_part<T>(a.x[j], slot, left) : load_slot<T>(a.x[j], slot)) : V(T(0));
#pragma unroll
    for (int k = 0; k < Q; ++k)
        yv[k] = k < q ? (PART ? load_part<T>(a.y[k], slot, left) : load_slot<T>(a.y[k], slot)) : V(T(0));
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        if (k < q) {
            V zv;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                double acc = (double)yv[k][e];
#pragma unroll
                for (int j = 0; j < P; ++j) acc = __builtin_fma(-(double)xv[j][e], cm[j][k], acc);
                zv[e] = drop ? T(0) : (T)(sigma * acc);
            }
            if constexpr (PART) {
                T *z = static_cast<T *>(a.z[k]) + slot * VEC;
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (e < left) z[e] = zv[e];
            } else {
                store_slot<T>(a.z[k], slot, zv);
            }
        }
    }
}

template <typename T, int P, int Q>
__global__ __launch_bounds__(kThreads) void combine_kernel(CombPtrs a, int p, int q, int64_t n, const double *__restrict__ c,
                                                            int scale_op, const double *__restrict__ s_ref,
                                                            const double *__restrict__ s_ptr)
{
    constexpr int VEC = VecOf<T>::N;
    double sigma = 1.0;
    bool drop = false;
    if (scale_op != NFM_STOCH_SCALE_NONE) {
        const double sv = *s_ptr;
        sigma = 1.0 / sqrt(sv);
        if (scale_op == NFM_STOCH_SCALE_RSQRT_OR_DROP) {
            const double tol = 64.0 * (sizeof(T) == 4 ? 0x1p-23 : 0x1p-52);
            // a column the projections reduced below 64 eps of its length, or whose norm is not a number
            const bool keep = sv > tol * tol * *s_ref && sv > 0.0 && sv < __builtin_inf();
            drop = !keep;
        }
    }
    double cm[P ? P : 1][Q];
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
        for (int k = 0; k < Q; ++k) cm[j][k] = (j < p && k < q) ? c[j * q + k] : 0.0;

    const int64_t nfull = n / VEC;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    for (int64_t s = gid; s < nfull; s += stride) combine_slot<T, P, Q, false>(a, p, q, s, VEC, cm, sigma, drop);
    const int left = (int)(n - nfull * VEC);
    if (left > 0 && gid == nfull % stride) combine_slot<T, P, Q, true>(a, p, q, nfull, left, cm, sigma, drop);
}

template <typename T, int P, int Q>
static void combine_launch(const CombPtrs &a, int p, int q, int64_t n, const double *c, int scale_op, const double *s_ref,
                           const double *sp, hipStream_t s)
{
    const int64_t slots = n / VecOf<T>::N + 1;
    int64_t grid = (slots + kThreads - 1) / kThreads;
    if (grid > (1 << 18)) grid = 1 << 18;
    hipLaunchKernelGGL((combine_kernel<T, P, Q>), dim3((unsigned)grid), dim3(kThreads), 0, s, a, p, q, n, c, scale_op, s_ref,
                       sp);
}

template <typename T>
static int combine_t(int p, int q, int64_t n, const void *const *x, const double *c, const void *const *y, void *const *z,
                     int scale_op, const double *s_ref, const double *sp, hipStream_t s)
{
    CombPtrs a = {};
    for (int j = 0; j < p; ++j) a.x[j] = x[j];
    for (int k = 0; k < q; ++k) {
        a.y[k] = y[k];
        a.z[k] = z[k];
    }
    if (q == 1) {
        switch (p == 0 ? 0 : form_of(p)) {
        case 0: combine_launch<T, 0, 1>(a, p, q, n, c, scale_op, s_ref, sp, s); break;
        case 1: combine_launch<T, 1, 1>(a, p, q, n, c, scale_op, s_ref, sp, s); break;
        case 2: combine_launch<T, 2, 1>(a, p, q, n, c, scale_op, s_ref, sp, s); break;
        case 4: combine_launch<T, 4, 1>(a, p, q, n, c, scale_op, s_ref, sp, s); break;
        default: combine_launch<T, 8, 1>(a, p, q, n, c, scale_op, s_ref, sp, s); break;
        }
    } else {
        switch (form_of(p > q ? p : q)) {
        case 2: combine_launch<T, 2, 2>(a, p, q, n, c, scale_op, s_ref, sp, s); break;
        case 4: combine_launch<T, 4, 4>(a, p, q, n, c, scale_op, s_ref, sp, s); break;
        default: combine_launch<T, 8, 8>(a, p, q, n, c, scale_op, s_ref, sp, s); break;
        }
    }
    return launch_status();
}

inline bool aligned_to(const void *p, size_t e) { return reinterpret_cast<uintptr_t>(p) % e == 0; }

} // namespace stoch
} // namespace nfm

using namespace nfm;
using namespace nfm::stoch;

extern "C" {

int nfm_stoch_philox_host(const uint32_t *counter, const uint32_t *key, uint32_t *out)
{
    if (counter == nullptr || key == nullptr || out == nullptr) return NFM_EINVAL;
    const U4 r = philox4x32_10(U4{counter[0], counter[1], counter[2], counter[3]}, key[0], key[1]);
    out[0] = r.w0;
    out[1] = r.w1;
    out[2] = r.w2;
    out[3] = r.w3;
    return NFM_OK;
}

int nfm_stoch_fill(int dtype, int kind, uint64_t seed, int64_t offset, int64_t n, void *out, void *stream)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (kind != NFM_STOCH_RADEMACHER && kind != NFM_STOCH_GAUSSIAN) return NFM_EINVAL;
    if (n < 0 || offset < 0 || offset > INT64_MAX - n) return NFM_EINVAL;
    if (n == 0) return NFM_OK;
    if (out == nullptr) return NFM_EINVAL;
    if (!aligned_to(out, dtype == NFM_F32 ? 4 : 8)) return NFM_EALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return kind == NFM_STOCH_RADEMACHER ? fill_t<T, NFM_STOCH_RADEMACHER>(seed, (uint64_t)offset, n, out, s)
                                            : fill_t<T, NFM_STOCH_GAUSSIAN>(seed, (uint64_t)offset, n, out, s);
    });
}

size_t nfm_stoch_gram_workspace_bytes(int p, int q)
{
    if (p < 1 || p > kMaxVecs || q < 1 || q > kMaxVecs) return 0;
    const int m = p > q ? p : q, Pf = form_of(m), Qf = (p == 1 || q == 1) ? 1 : Pf;
    return (size_t)kRedBlocks * Pf * Qf * sizeof(double);
}

int nfm_stoch_gram(int dtype, int p, int q, int64_t n, const void *const *x, const void *const *y, void *workspace,
                   size_t workspace_bytes, double *out, int accumulate, void *stream)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (n < 0) return NFM_EINVAL;
    if (p < 1 || p > kMaxVecs || q < 1 || q > kMaxVecs) return NFM_ESIZE;
    if (n == 0 && accumulate) return NFM_OK;
    if (out == nullptr || workspace == nullptr || x == nullptr || y == nullptr) return NFM_EINVAL;
    if (workspace_bytes < nfm_stoch_gram_workspace_bytes(p, q)) return NFM_EWORKSPACE;
    const size_t e = dtype == NFM_F32 ? 4 : 8;
    for (int j = 0; j < p; ++j) {
        if (n > 0 && x[j] == nullptr) return NFM_EINVAL;
        if (!aligned_to(x[j], e)) return NFM_EALIGN;
    }
    for (int k = 0; k < q; ++k) {
        if (n > 0 && y[k] == nullptr) return NFM_EINVAL;
        if (!aligned_to(y[k], e)) return NFM_EALIGN;
    }
    if (!aligned_to(out, 8) || !aligned_to(workspace, 8)) return NFM_EALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto t) { return gram_t<decltype(t)>(p, q, n, x, y, workspace, out, accumulate, s); });
}

int nfm_stoch_combine(int dtype, int p, int q, int64_t n, const void *const *x, const double *c, const void *const *y,
                      void *const *z, int scale_op, const double *s_ref, const double *s, void *stream)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (n < 0) return NFM_EINVAL;
    if (p < 0 || p > kMaxVecs || q < 1 || q > kMaxVecs) return NFM_ESIZE;
    if (scale_op != NFM_STOCH_SCALE_NONE && scale_op != NFM_STOCH_SCALE_RSQRT && scale_op != NFM_STOCH_SCALE_RSQRT_OR_DROP)
        return NFM_EINVAL;
    if (n == 0) return NFM_OK;
    if (y == nullptr || z == nullptr || (p > 0 && (x == nullptr || c == nullptr))) return NFM_EINVAL;
    if (scale_op != NFM_STOCH_SCALE_NONE && s == nullptr) return NFM_EINVAL;
    if (scale_op == NFM_STOCH_SCALE_RSQRT_OR_DROP && s_ref == nullptr) return NFM_EINVAL;
    const size_t e = dtype == NFM_F32 ? 4 : 8;
    for (int j = 0; j < p; ++j) {
        if (x[j] == nullptr) return NFM_EINVAL;
        if (!aligned_to(x[j], e)) return NFM_EALIGN;
    }
    for (int k = 0; k < q; ++k) {
        if (y[k] == nullptr || z[k] == nullptr) return NFM_EINVAL;
        if (!aligned_to(y[k], e) || !aligned_to(z[k], e)) return NFM_EALIGN;
    }
    if (!aligned_to(c, 8) || !aligned_to(s, 8) || !aligned_to(s_ref, 8)) return NFM_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return by_dtype(dtype,
                    [&](auto t) { return combine_t<decltype(t)>(p, q, n, x, c, y, z, scale_op, s_ref, s, st); });
}

} // extern "C"
