// nfm_simplex_ops.hpp -- arithmetic of the simplex functions (reference `simplex.py`): softmax,
// log_softmax, logsumexp, logit and their backward passes over the K' classes of ONE voxel.
//
// K' ("kp") is the number of classes the arithmetic sees: the K stored logits plus, for an implicit
// input, the hidden zero-logit class, which takes its place at `idx` among the K' classes.  Every
// tensor either stores all K' classes or lacks class `idx` (miss_a / miss_g / miss_o); a lacking
// class reads as 0 and is not written.  The arithmetic is written ONCE, against an accessor `IO`, and
// instantiated by the register kernels (K' a compile-time constant, classes in VGPRs) and by the
// runtime-K' kernels (classes re-read from memory or LDS): every variant and every layout runs the
// same operations in the same order, so results are bit-identical whichever kernel served a call.
// No multiply-add is contracted (pragma below), every sum runs in class-index order.
#pragma once
#include "nfm_common.hpp"

#pragma clang fp contract(off)

namespace nfm {
namespace simplex {

struct Args {
    int op;                     // NFM_SIMPLEX_*
    int kp;                     // K': classes the arithmetic sees
    int idx;                    // position of the implicit class among the K'
    int miss_a, miss_g, miss_o; // the tensor lacks class idx
    int ca, cg, co;             // classes stored per tensor (cg == 1: one value per voxel, broadcast)
    int bcast_g;
    int64_t outer, inner;       // the (outer, classes, inner) view shared by all tensors
    const void *a;              // forward: input; backward: saved tensor
    const void *g;              // backward: grad_output
    void *o;                    // forward: output; backward: grad_input
    void *l;                    // forward: per-voxel logsumexp (outer, inner), may be null
};

__device__ __forceinline__ float exp_t(float x) { return expf(x); }
__device__ __forceinline__ double exp_t(double x) { return exp(x); }
__device__ __forceinline__ float log_t(float x) { return logf(x); }
__device__ __forceinline__ double log_t(double x) { return log(x); }

// component of class j in a tensor that lacks class idx (miss) or not
__device__ __forceinline__ int comp_of(int j, int miss, int idx) { return j - ((miss && j > idx) ? 1 : 0); }

// IO: a(j), g(j) -- class j of the two inputs (0 where the tensor lacks it); stash(j, e) / ex(j, m) -- keep
// or recompute exp(a(j) - m); put(j, v) -- class j of the output; put_lse(v).  IO::kInPlace: the output
// overwrites input `a` (lane-owned LDS row), so the last loop runs downwards when the output is the longer.
template <typename T, int KPC, bool BWD, class IO>
__device__ __forceinline__ void apply(const Args &p, IO &io)
{
    const int KP = KPC ? KPC : p.kp;
    const int idx = p.idx;
    const bool desc = IO::kInPlace && p.miss_a && !p.miss_o;
#define NFM_SX_ALL(j) _Pragma("unroll") for (int j = 0; j < KP; ++j)
#define NFM_SX_OUT(j)                                                                      \
    _Pragma("unroll") for (int j##_ = 0; j##_ < KP; ++j##_)                                 \
        if (const int j = desc ? KP - 1 - j##_ : j##_; !(p.miss_o && j == idx))
    const int op = p.op;
    if (op == NFM_SIMPLEX_LOGIT) {
        if constexpr (!BWD) {
            T ref;
            if (p.miss_a) { // hidden class: 1 - sum, clamped like the reference (NaN stays NaN)
                T sp = T(0);
                NFM_SX_ALL(j) if (j != idx) sp = sp + io.a(j);
                T ex = T(1) - sp;
                ex = (ex < T(1e-8)) ? T(1e-8) : ex;
                ref = log_t(ex);
            } else {
                T pi = T(0);
                NFM_SX_ALL(j) if (j == idx) pi = io.a(j);
                ref = log_t(pi);
            }
            NFM_SX_OUT(j) io.put(j, (p.miss_a && j == idx) ? T(0) : log_t(io.a(j)) - ref);
        }
        return;
    }
    if (op == NFM_SIMPLEX_SOFTMAX_BWD) {
        if constexpr (BWD) {
            // a = softmax output.  A class dropped from the output of an explicit input is 1 - sum of the rest.
            const bool synth = p.miss_a && !p.miss_o;
            T pidx = T(0);
            if (synth) {
                T sp = T(0);
                NFM_SX_ALL(j) if (j != idx) sp = sp + io.a(j);
                pidx = T(1) - sp;
            }
            T dot = T(0);
            NFM_SX_ALL(j)
            {
                const T pj = (synth && j == idx) ? pidx : io.a(j);
                const T t = io.g(j) * pj;
                dot = dot + t;
            }
            NFM_SX_OUT(j)
            {
                const T pj = (synth && j == idx) ? pidx : io.a(j);
                io.put(j, pj * (io.g(j) - dot));
            }
        }
        return;
    }
    // everything else starts from the (clamped) max and the sum of exponentials of the logits `a`
    T m = io.a(0);
    NFM_SX_ALL(j)
    {
        const T x = io.a(j);
        m = (x > m || x != x) ? x : m; // NaN wins, like torch.max
    }
    T s = T(0);
    NFM_SX_ALL(j)
    {
        const T e = exp_t(io.a(j) - m);
        io.stash(j, e);
        s = s + e;
    }
    if constexpr (!BWD) {
        if (op == NFM_SIMPLEX_SOFTMAX) {
            NFM_SX_OUT(j) io.put(j, io.ex(j, m) / s);
            if (p.l) io.put_lse(m + log_t(s));
        } else {
            const T l = m + log_t(s);
            if (op == NFM_SIMPLEX_LOG_SOFTMAX) {
                NFM_SX_OUT(j) io.put(j, io.a(j) - l);
            } else {
                io.put_lse(l);
            }
        }
    } else {
        if (op == NFM_SIMPLEX_LOGSUMEXP_BWD) { // softmax(a) * g, g one value per voxel
            const T gg = io.g(0);
            NFM_SX_OUT(j)
            {
                const T q = io.ex(j, m) / s;
                io.put(j, q * gg);
            }
        } else { // NFM_SIMPLEX_LOG_SOFTMAX_BWD: g - softmax(a) * sum(g)
            T sg = T(0);
            NFM_SX_ALL(j) sg = sg + io.g(j);
            NFM_SX_OUT(j)
            {
                const T q = io.ex(j, m) / s;
                const T t = q * sg;
                io.put(j, io.g(j) - t);
            }
        }
    }
#undef NFM_SX_ALL
#undef NFM_SX_OUT
}

// ---------------------------------------------------------------- class-last tiles through LDS
// `nt` lanes move the n (<= nt * C) contiguous elements of nt records of C classes between global
// memory and an LDS image with an ODD row pitch: global accesses are 16 bytes per lane where the
// tile is whole, and a lane's walk along its own row is bank-conflict-free.
template <typename T>
__device__ __forceinline__ void tile_in(T *lds, const T *__restrict__ g, int C, int pitch, int n, int nt)
{
    using V = typename VecOf<T>::type;
    using VG = typename VecOf<T>::gtype;
    constexpr int kVec = VecOf<T>::N;
    const int step = nt * kVec, dr = step / C, dc = step - dr * C;
    int e = threadIdx.x * kVec;
    int r = e / C, c = e - r * C;
    for (; e < n; e += step) {
        int rr = r, cc = c;
        if (e + kVec <= n) {
            const V v = NFM_LDG(reinterpret_cast<const VG *>(g + e));
#pragma unroll
            for (int k = 0; k < kVec; ++k) {
                lds[rr * pitch + cc] = v[k];
                if (++cc == C) { cc = 0; ++rr; }
            }
        } else {
#pragma unroll
            for (int k = 0; k < kVec; ++k) {
                if (e + k < n) lds[rr * pitch + cc] = g[e + k];
                if (++cc == C) { cc = 0; ++rr; }
            }
        }
        r += dr;
        c += dc;
        if (c >= C) { c -= C; ++r; }
    }
}

template <typename T>
__device__ __forceinline__ void tile_out(const T *lds, T *__restrict__ g, int C, int pitch, int n, int nt)
{
    using V = typename VecOf<T>::type;
    using VG = typename VecOf<T>::gtype;
    constexpr int kVec = VecOf<T>::N;
    const int step = nt * kVec, dr = step / C, dc = step - dr * C;
    int e = threadIdx.x * kVec;
    int r = e / C, c = e - r * C;
    for (; e < n; e += step) {
        int rr = r, cc = c;
        if (e + kVec <= n) {
            V v;
#pragma unroll
            for (int k = 0; k < kVec; ++k) {
                v[k] = lds[rr * pitch + cc];
                if (++cc == C) { cc = 0; ++rr; }
            }
            NFM_STG(static_cast<VG>(v), reinterpret_cast<VG *>(g + e));
        } else {
#pragma unroll
            for (int k = 0; k < kVec; ++k) {
                if (e + k < n) g[e + k] = lds[rr * pitch + cc];
                if (++cc == C) { cc = 0; ++rr; }
            }
        }
        r += dr;
        c += dc;
        if (c >= C) { c -= C; ++r; }
    }
}

} // namespace simplex
} // namespace nfm
