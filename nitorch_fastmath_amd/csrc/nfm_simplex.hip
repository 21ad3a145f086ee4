// nfm_simplex.hip -- softmax / log_softmax / logsumexp / logit with an implicit class, and their
// backward passes (reference `simplex.py`), one voxel per lane over an (outer, classes, inner) view.
//   reg_kernel    K' = 1..17 classes in registers (K <= 16 with or without an implicit class): every input
//                 element is read once, every output element written once.
//                   inner > 1 (channel-first): lanes along `inner`, 16-byte accesses when the vector width
//                   divides `inner`, one element per access otherwise;
//                   inner == 1 (class axis last): a tile of 256 records goes through LDS (tile_in / tile_out).
//   sweep_kernel  K' up to NFM_SIMPLEX_MAX_K + 1, at run time: the same arithmetic in three sweeps over the
//                 class axis (max; sum of exponentials; outputs).  Channel-first re-reads memory (the tile
//                 of a workgroup stays in L2), class-last keeps the tile in LDS and writes the output over it.
// The arithmetic is in nfm_simplex_ops.hpp.  The implicit class is never stored on the input side; on the
// output side it is written at its index or not at all.
#include "nfm_simplex_ops.hpp"

namespace nfm {
namespace simplex {

constexpr int kTile = 256;
constexpr int kRegMax = 17; // K' of the register kernels

// -------------------------------------------------------------------------------- register kernels
template <typename T, int KP, int VEC>
struct RegIO {
    static constexpr bool kInPlace = false;
    T (&xa)[KP];
    T (&xg)[KP];
    T e[KP];
    T lse;
    int bcast;
    __device__ __forceinline__ RegIO(T (&a_)[KP], T (&g_)[KP], int bcast_) : xa(a_), xg(g_), bcast(bcast_) {}
    __device__ __forceinline__ T a(int j) const { return xa[j]; }
    __device__ __forceinline__ T g(int j) const { return bcast ? xg[0] : xg[j]; }
    __device__ __forceinline__ void stash(int j, T v) { e[j] = v; }
    __device__ __forceinline__ T ex(int j, T) const { return e[j]; }
    __device__ __forceinline__ void put(int j, T v) { xa[j] = v; } // the result takes the input's registers
    __device__ __forceinline__ void put_lse(T v) { lse = v; }
};

template <typename T, int VEC>
struct Pack {
    typedef T type __attribute__((ext_vector_type(VEC), aligned(sizeof(T))));
};

template <typename T, int VEC>
__device__ __forceinline__ void ldv(const T *p, T (&v)[VEC])
{
    if constexpr (VEC == 1) {
        v[0] = NFM_LDG(p);
    } else {
        using W = typename Pack<T, VEC>::type;
        const W w = NFM_LDG(reinterpret_cast<const W *>(p));
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = w[k];
    }
}

template <typename T, int VEC>
__device__ __forceinline__ void stv(T *p, const T (&v)[VEC])
{
    if constexpr (VEC == 1) {
        NFM_STG(v[0], p);
    } else {
        using W = typename Pack<T, VEC>::type;
        W w;
#pragma unroll
        for (int k = 0; k < VEC; ++k) w[k] = v[k];
        NFM_STG(w, reinterpret_cast<W *>(p));
    }
}

template <typename T, int KP, int VEC, bool AOS, bool BWD>
__global__ __launch_bounds__(kTile) void reg_kernel(const Args p)
{
    static_assert(!AOS || VEC == 1, "class-last tiles hold one voxel per lane");
    constexpr int kPitch = KP | 1;
    __shared__ T lds[AOS ? kTile * kPitch : 1];
    const int idx = p.idx;
    const int tid = threadIdx.x;
    T xa[VEC][KP], xg[VEC][KP];
    const int ng = BWD ? (p.bcast_g ? 1 : KP) : 0;
    int64_t o = 0, i = 0, v0 = 0;
    int nv = 0;
    bool live = true;
    if constexpr (AOS) {
        v0 = (int64_t)blockIdx.x * kTile;
        nv = (int)(p.outer - v0 < kTile ? p.outer - v0 : kTile);
        live = tid < nv;
        tile_in(lds, static_cast<const T *>(p.a) + v0 * p.ca, p.ca, kPitch, nv * p.ca, kTile);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KP; ++j)
            xa[0][j] = (p.miss_a && j == idx) ? T(0) : lds[tid * kPitch + comp_of(j, p.miss_a, idx)];
        if constexpr (BWD) {
            __syncthreads();
            tile_in(lds, static_cast<const T *>(p.g) + v0 * p.cg, p.cg, kPitch, nv * p.cg, kTile);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < KP; ++j)
                if (j < ng) xg[0][j] = (p.miss_g && j == idx) ? T(0) : lds[tid * kPitch + comp_of(j, p.miss_g, idx)];
        }
    } else {
        const int64_t ipv = p.inner / VEC; // VEC divides inner
        const int64_t gid = (int64_t)blockIdx.x * kTile + tid;
        if (gid >= p.outer * ipv) return;
        o = gid / ipv;
        i = (gid - o * ipv) * VEC;
        const T *A = static_cast<const T *>(p.a) + o * p.ca * p.inner + i;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            T v[VEC];
            if (p.miss_a && j == idx) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) v[k] = T(0);
            } else {
                ldv<T, VEC>(A + comp_of(j, p.miss_a, idx) * p.inner, v);
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) xa[k][j] = v[k];
        }
        if constexpr (BWD) {
            const T *G = static_cast<const T *>(p.g) + o * p.cg * p.inner + i;
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                if (j < ng) {
                    T v[VEC];
                    if (p.miss_g && j == idx) {
#pragma unroll
                        for (int k = 0; k < VEC; ++k) v[k] = T(0);
                    } else {
                        ldv<T, VEC>(G + comp_of(j, p.miss_g, idx) * p.inner, v);
                    }
#pragma unroll
                    for (int k = 0; k < VEC; ++k) xg[k][j] = v[k];
                }
            }
        }
    }
    T lse[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        RegIO<T, KP, VEC> io(xa[k], xg[k], p.bcast_g);
        io.lse = T(0);
        apply<T, KP, BWD>(p, io);
        lse[k] = io.lse;
    }
    const bool has_o = p.o != nullptr;
    if constexpr (AOS) {
        if (has_o) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < KP; ++j)
                if (!(p.miss_o && j == idx)) lds[tid * kPitch + comp_of(j, p.miss_o, idx)] = xa[0][j];
            __syncthreads();
            tile_out(lds, static_cast<T *>(p.o) + v0 * p.co, p.co, kPitch, nv * p.co, kTile);
        }
        if (!BWD && p.l && live) NFM_STG(lse[0], static_cast<T *>(p.l) + v0 + tid);
    } else {
        if (has_o) {
            T *O = static_cast<T *>(p.o) + o * p.co * p.inner + i;
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                if (!(p.miss_o && j == idx)) {
                    T v[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; ++k) v[k] = xa[k][j];
                    stv<T, VEC>(O + comp_of(j, p.miss_o, idx) * p.inner, v);
                }
            }
        }
        if (!BWD && p.l) stv<T, VEC>(static_cast<T *>(p.l) + o * p.inner + i, lse);
    }
}

// -------------------------------------------------------------------------------- runtime-K' kernels
template <typename T>
struct SweepIO {
    static constexpr bool kInPlace = true; // (only the LDS variant overwrites; downward order is harmless otherwise)
    const T *A;
    const T *G;
    T *O;
    int64_t sa, sg, so; // distance between classes
    int miss_a, miss_g, miss_o, idx, bcast;
    T lse;
    __device__ __forceinline__ T a(int j) const { return (miss_a && j == idx) ? T(0) : A[comp_of(j, miss_a, idx) * sa]; }
    __device__ __forceinline__ T g(int j) const
    {
        if (bcast) return G[0];
        return (miss_g && j == idx) ? T(0) : G[comp_of(j, miss_g, idx) * sg];
    }
    __device__ __forceinline__ void stash(int, T) {}
    __device__ __forceinline__ T ex(int j, T m) const { return exp_t(a(j) - m); }
    __device__ __forceinline__ void put(int j, T v) { O[comp_of(j, miss_o, idx) * so] = v; }
    __device__ __forceinline__ void put_lse(T v) { lse = v; }
};

template <typename T, bool AOS, bool BWD>
__global__ __launch_bounds__(kTile) void sweep_kernel(const Args p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, nt = blockDim.x;
    SweepIO<T> io;
    io.miss_a = p.miss_a, io.miss_g = p.miss_g, io.miss_o = p.miss_o, io.idx = p.idx, io.bcast = p.bcast_g;
    io.lse = T(0);
    io.G = nullptr;
    if constexpr (AOS) {
        const int pitch = p.kp | 1;
        T *la = reinterpret_cast<T *>(smem), *lg = la + nt * pitch;
        const int64_t v0 = (int64_t)blockIdx.x * nt;
        const int nv = (int)(p.outer - v0 < nt ? p.outer - v0 : nt);
        tile_in(la, static_cast<const T *>(p.a) + v0 * p.ca, p.ca, pitch, nv * p.ca, nt);
        if constexpr (BWD) tile_in(lg, static_cast<const T *>(p.g) + v0 * p.cg, p.cg, pitch, nv * p.cg, nt);
        __syncthreads();
        io.A = la + tid * pitch;
        io.G = lg + tid * pitch;
        io.O = la + tid * pitch; // in place: lane-owned row
        io.sa = io.sg = io.so = 1;
        if (tid < nv) apply<T, 0, BWD>(p, io);
        __syncthreads();
        if (p.o) tile_out(la, static_cast<T *>(p.o) + v0 * p.co, p.co, pitch, nv * p.co, nt);
        if (!BWD && p.l && tid < nv) static_cast<T *>(p.l)[v0 + tid] = io.lse;
    } else {
        const int64_t gid = (int64_t)blockIdx.x * nt + tid;
        if (gid >= p.outer * p.inner) return;
        const int64_t o = gid / p.inner, i = gid - o * p.inner;
        io.A = static_cast<const T *>(p.a) + o * p.ca * p.inner + i;
        if constexpr (BWD) io.G = static_cast<const T *>(p.g) + o * p.cg * p.inner + i;
        io.O = p.o ? static_cast<T *>(p.o) + o * p.co * p.inner + i : nullptr; // logsumexp has no class output
        io.sa = io.sg = io.so = p.inner;
        apply<T, 0, BWD>(p, io);
        if (!BWD && p.l) static_cast<T *>(p.l)[o * p.inner + i] = io.lse;
    }
}

// -------------------------------------------------------------------------------- host side
template <typename T, int KP, bool BWD>
static int launch_reg(const Args &p, hipStream_t st)
{
    constexpr int kVec = VecOf<T>::N;
    if (p.inner == 1) {
        const int64_t blocks = (p.outer + kTile - 1) / kTile;
        if (blocks > 0x7fffffffLL) return NFM_ESIZE;
        hipLaunchKernelGGL((reg_kernel<T, KP, 1, true, BWD>), dim3((unsigned)blocks), dim3(kTile), 0, st, p);
    } else if (p.inner % kVec == 0) {
        const int64_t blocks = (p.outer * (p.inner / kVec) + kTile - 1) / kTile;
        if (blocks > 0x7fffffffLL) return NFM_ESIZE;
        hipLaunchKernelGGL((reg_kernel<T, KP, kVec, false, BWD>), dim3((unsigned)blocks), dim3(kTile), 0, st, p);
    } else {
        const int64_t blocks = (p.outer * p.inner + kTile - 1) / kTile;
        if (blocks > 0x7fffffffLL) return NFM_ESIZE;
        hipLaunchKernelGGL((reg_kernel<T, KP, 1, false, BWD>), dim3((unsigned)blocks), dim3(kTile), 0, st, p);
    }
    return launch_status();
}

template <typename T, bool BWD>
static int launch_sweep(const Args &p, hipStream_t st)
{
    if (p.inner == 1) {
        // LDS: one image (two for a backward pass) of nt rows of K' | 1 elements, at most 48 KiB
        const size_t row = (size_t)(p.kp | 1) * sizeof(T) * (BWD ? 2 : 1);
        int nt = kTile;
        while (nt > 64 && nt * row > 48 * 1024) nt /= 2;
        if (nt * row > 64 * 1024) return NFM_ESIZE;
        const int64_t blocks = (p.outer + nt - 1) / nt;
        if (blocks > 0x7fffffffLL) return NFM_ESIZE;
        hipLaunchKernelGGL((sweep_kernel<T, true, BWD>), dim3((unsigned)blocks), dim3(nt), nt * row, st, p);
    } else {
        const int64_t blocks = (p.outer * p.inner + kTile - 1) / kTile;
        if (blocks > 0x7fffffffLL) return NFM_ESIZE;
        hipLaunchKernelGGL((sweep_kernel<T, false, BWD>), dim3((unsigned)blocks), dim3(kTile), 0, st, p);
    }
    return launch_status();
}

template <typename T, bool BWD>
static int dispatch(const Args &p, void *stream)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
#define NFM_SX(KPv) \
    case KPv: return launch_reg<T, KPv, BWD>(p, st);
    switch (p.kp) {
        NFM_SX(1) NFM_SX(2) NFM_SX(3) NFM_SX(4) NFM_SX(5) NFM_SX(6) NFM_SX(7) NFM_SX(8) NFM_SX(9)
        NFM_SX(10) NFM_SX(11) NFM_SX(12) NFM_SX(13) NFM_SX(14) NFM_SX(15) NFM_SX(16) NFM_SX(17)
    default: break;
    }
#undef NFM_SX
    static_assert(kRegMax == 17, "the switch above lists the register kernels");
    return launch_sweep<T, BWD>(p, st);
}

static int check_ptr(const void *ptr, size_t elem, bool needed)
{
    if (ptr == nullptr) return needed ? NFM_EINVAL : NFM_OK;
    return reinterpret_cast<uintptr_t>(ptr) % elem == 0 ? NFM_OK : NFM_EALIGN;
}

// the checks both entry points share; fills the class bookkeeping of `p`
static int prepare(Args &p, int dtype, int flags, int implicit_index, int64_t outer, int64_t K, int64_t inner)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (outer < 0 || K < 0 || inner < 0) return NFM_EINVAL;
    if (flags & ~(NFM_SIMPLEX_IMPLICIT_IN | NFM_SIMPLEX_IMPLICIT_OUT)) return NFM_EINVAL;
    if (K < 1) return NFM_EINVAL;
    if (K > NFM_SIMPLEX_MAX_K) return NFM_ESIZE;
    const int in = (flags & NFM_SIMPLEX_IMPLICIT_IN) ? 1 : 0, out = (flags & NFM_SIMPLEX_IMPLICIT_OUT) ? 1 : 0;
    p.kp = (int)K + in;
    if (implicit_index < 0 || implicit_index >= p.kp) return NFM_EINVAL;
    if (p.kp - out < 1) return NFM_EINVAL; // an output without classes
    if (outer > 0 && inner > 0 && (outer > INT64_MAX / inner || outer * inner > INT64_MAX / (p.kp + 1)))
        return NFM_ESIZE;
    p.idx = implicit_index;
    p.outer = outer;
    p.inner = inner;
    p.miss_a = p.miss_g = p.miss_o = 0;
    p.ca = p.cg = p.co = 0;
    p.bcast_g = 0;
    p.a = p.g = nullptr;
    p.o = p.l = nullptr;
    return NFM_OK;
}

} // namespace simplex
} // namespace nfm

using namespace nfm;
using nfm::simplex::Args;

extern "C" {

int nfm_simplex_forward(int dtype, int op, int flags, int implicit_index, int64_t outer, int64_t K, int64_t inner,
                        const void *x, void *out, void *lse, void *stream)
{
    Args p;
    int rc = simplex::prepare(p, dtype, flags, implicit_index, outer, K, inner);
    if (rc) return rc;
    if (op != NFM_SIMPLEX_SOFTMAX && op != NFM_SIMPLEX_LOG_SOFTMAX && op != NFM_SIMPLEX_LOGSUMEXP &&
        op != NFM_SIMPLEX_LOGIT)
        return NFM_EINVAL;
    const bool nonempty = outer > 0 && inner > 0;
    const size_t elem = dtype == NFM_F32 ? 4 : 8;
    const bool only_lse = op == NFM_SIMPLEX_LOGSUMEXP;
    if (lse != nullptr && op != NFM_SIMPLEX_SOFTMAX && !only_lse) return NFM_EINVAL;
    if ((rc = simplex::check_ptr(x, elem, nonempty))) return rc;
    if ((rc = simplex::check_ptr(out, elem, nonempty && !only_lse))) return rc;
    if ((rc = simplex::check_ptr(lse, elem, nonempty && only_lse))) return rc;
    if (!nonempty) return NFM_OK;
    const int in = (flags & NFM_SIMPLEX_IMPLICIT_IN) ? 1 : 0, outf = (flags & NFM_SIMPLEX_IMPLICIT_OUT) ? 1 : 0;
    p.op = op;
    p.miss_a = in;
    p.miss_o = outf;
    p.ca = p.kp - in;
    p.co = p.kp - outf;
    p.a = x;
    p.o = only_lse ? nullptr : out;
    p.l = lse;
    return by_dtype(dtype, [&](auto t) { return simplex::dispatch<decltype(t), false>(p, stream); });
}

int nfm_simplex_backward(int dtype, int op, int flags, int implicit_index, int64_t outer, int64_t K, int64_t inner,
                         const void *saved, const void *grad_output, void *grad_input, void *stream)
{
    Args p;
    int rc = simplex::prepare(p, dtype, flags, implicit_index, outer, K, inner);
    if (rc) return rc;
    if (op != NFM_SIMPLEX_SOFTMAX_BWD && op != NFM_SIMPLEX_LOGSUMEXP_BWD && op != NFM_SIMPLEX_LOG_SOFTMAX_BWD)
        return NFM_EINVAL;
    const bool nonempty = outer > 0 && inner > 0;
    const size_t elem = dtype == NFM_F32 ? 4 : 8;
    if ((rc = simplex::check_ptr(saved, elem, nonempty))) return rc;
    if ((rc = simplex::check_ptr(grad_output, elem, nonempty))) return rc;
    if ((rc = simplex::check_ptr(grad_input, elem, nonempty))) return rc;
    if (!nonempty) return NFM_OK;
    const int in = (flags & NFM_SIMPLEX_IMPLICIT_IN) ? 1 : 0, outf = (flags & NFM_SIMPLEX_IMPLICIT_OUT) ? 1 : 0;
    p.op = op;
    p.miss_o = in; // the gradient has the input's classes
    p.co = p.kp - in;
    if (op == NFM_SIMPLEX_SOFTMAX_BWD) { // saved = the output
        p.miss_a = p.miss_g = outf;
        p.ca = p.cg = p.kp - outf;
    } else { // saved = the input
        p.miss_a = in;
        p.ca = p.kp - in;
        if (op == NFM_SIMPLEX_LOGSUMEXP_BWD) {
            p.bcast_g = 1;
            p.cg = 1;
        } else {
            p.miss_g = outf;
            p.cg = p.kp - outf;
        }
    }
    p.a = saved;
    p.g = grad_output;
    p.o = grad_input;
    return by_dtype(dtype, [&](auto t) { return simplex::dispatch<decltype(t), true>(p, stream); });
}

} // extern "C"
