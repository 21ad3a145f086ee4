// nfm_cholgrad.hip -- backward kernels of the Cholesky factor of compact symmetric positive definite matrices (the
// gradients of sym_chol and sym_chol_apply; an extension of `sym`, no counterpart in the reference).  One record per
// lane through rec_kernel, as nfm_symchol.hip: read the K = N (N + 1) / 2 compact values, the cotangent (and the N of
// the vector), factor (or adopt the factor) in registers, run the two triangular sweeps of nfm_cholgrad_ops.hpp, write
// the packed gradient.  The op and the `factored` flag are run-time members of Params (wave-uniform): the
// instantiations are (dtype, N, Op struct) x the layout kinds of rec_launch.  Compiled without implicit contraction
// (csrc/Makefile), so that every layout kind of an Op, and the CPU entry, give the same bits.
#include "nfm_record_kernel.hpp"
#include "nfm_cholgrad_ops.hpp"

// This file is compiled 17 times (-DNFM_CHOLGRAD_PART=0..16).  Part 0: the entry points, the caps and the CPU routine.
// Parts 1..16: the kernels of one (dtype, class, pair of orders): part = 1 + dtype * 8 + class * 4 + pair, class =
// NFM_CHOL_CLASS_FACTOR or NFM_CHOL_CLASS_APPLY, pair p = orders 2p + 1 and 2p + 2.
#ifndef NFM_CHOLGRAD_PART
#error "compile with -DNFM_CHOLGRAD_PART=0..16"
#endif

namespace nfm {

using symchol::CholParams;

// The compiled caps: the largest order of each (dtype, class) whose kernels have no private segment in any layout form
// (profiles/cholgrad_table.md lists the registers).  Orders above take the caller's own route.
constexpr int kCholGradCap[2][2] = {{8, 8}, {8, 8}}; // [dtype][NFM_CHOL_CLASS_FACTOR | NFM_CHOL_CLASS_APPLY]
constexpr bool cholgrad_fits(bool f64, int cls, int N) { return N >= 1 && N <= kCholGradCap[f64 ? 1 : 0][cls]; }

// Both Ops write a record at least as large as the matrix: every order is staged through the LDS tile, the rule
// nfm_symchol.hip measured for its own gradients.
template <typename T, int N>
struct CholFactorGradOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>; // compact A, or its factor
    using RB = Rec<1, K>; // cotangent of the factor
    using RC = NoRec;
    using RO = Rec<1, K>; // compact gradient
    using Params = CholParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RO::C) * (int)sizeof(T) + 48);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&g)[RB::Cs], const T (&)[1],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        cholgrad::rec_factor_grad<T, N>(a, g, o, q);
    }
};

template <typename T, int N>
struct CholApplyGradOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>;     // compact A, or its factor
    using RB = Rec<1, N>;     // the vector
    using RC = Rec<1, N>;     // cotangent of the applied vector
    using RO = Rec<1, K + N>; // packed gradient [K | N]
    using Params = CholParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RC::C + RO::C) * (int)sizeof(T) + 64);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&v)[RB::Cs], const T (&g)[RC::Cs],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        cholgrad::rec_apply_grad<T, N>(a, v, g, o, q);
    }
};

#define NFM_CHOLGRAD_ARGS                                                                                              \
    int M, const nfm_operand *a, const nfm_operand *v, const nfm_operand *g, const nfm_operand *o, int64_t no,          \
        int64_t ni, const CholParams &q, void *stream
template <int PART>
int cholgrad_part(NFM_CHOLGRAD_ARGS);

#if NFM_CHOLGRAD_PART >= 1
template <>
int cholgrad_part<NFM_CHOLGRAD_PART>(NFM_CHOLGRAD_ARGS)
{
    constexpr int part = NFM_CHOLGRAD_PART - 1;
    constexpr bool F64 = part / 8 != 0;
    constexpr int CLS = (part / 4) % 2;
    constexpr int N0 = 2 * (part % 4) + 1;
    using T = std::conditional_t<F64, double, float>;
    auto run = [&](auto n) -> int {
        constexpr int N = decltype(n)::value;
        if constexpr (cholgrad_fits(F64, CLS, N)) {
            if constexpr (CLS == NFM_CHOL_CLASS_FACTOR)
                return rec_launch<T, CholFactorGradOp<T, N>>(a, g, nullptr, o, no, ni, q, stream);
            else
                return rec_launch<T, CholApplyGradOp<T, N>>(a, v, g, o, no, ni, q, stream);
        } else {
            return NFM_ESIZE;
        }
    };
    if (M == N0) return run(std::integral_constant<int, N0>{});
    if (M == N0 + 1) return run(std::integral_constant<int, N0 + 1>{});
    return NFM_ESIZE;
}
#endif

} // namespace nfm

#if NFM_CHOLGRAD_PART == 0
using namespace nfm;

// n contiguous host records through the record routines of nfm_cholgrad_ops.hpp
template <typename T, int N>
static void cholgrad_host_n(int op, int64_t n, const T *mat, const T *vec, const T *gout, T *out)
{
    constexpr int K = sym_k(N);
    const CholParams q{op & ~NFM_CHOL_FACTORED, (op & NFM_CHOL_FACTORED) ? 1 : 0};
    for (int64_t b = 0; b < n; ++b) {
        T a[K];
        for (int k = 0; k < K; ++k) a[k] = mat[b * K + k];
        if (q.op == NFM_CHOL_FACTOR) {
            T g[K], o[K];
            for (int k = 0; k < K; ++k) g[k] = gout[b * K + k];
            cholgrad::rec_factor_grad<T, N>(a, g, o, q);
            for (int k = 0; k < K; ++k) out[b * K + k] = o[k];
        } else {
            T v[N], g[N], o[K + N];
            for (int i = 0; i < N; ++i) v[i] = vec[b * N + i];
            for (int i = 0; i < N; ++i) g[i] = gout[b * N + i];
            cholgrad::rec_apply_grad<T, N>(a, v, g, o, q);
            for (int k = 0; k < K + N; ++k) out[b * (K + N) + k] = o[k];
        }
    }
}

template <typename T>
static int cholgrad_host_t(int M, int op, int64_t n, const void *mat, const void *vec, const void *gout, void *out)
{
    return switch_order<8>(M, NFM_ESIZE, [&](auto nn) {
        constexpr int NN = nn;
        cholgrad_host_n<T, NN>(op, n, static_cast<const T *>(mat), static_cast<const T *>(vec),
                               static_cast<const T *>(gout), static_cast<T *>(out));
        return (int)NFM_OK;
    });
}

extern "C" {

int nfm_sym_chol_grad(int dtype, int M, int op, int64_t n_outer, int64_t n_inner, const nfm_operand *mat,
                      const nfm_operand *vec, const nfm_operand *gout, const nfm_operand *gpacked, void *stream)
{
    // the checks of nfm_sym_chol in its order: the batch, the op code, the cap, then the operands
    int rc = check_batch(dtype, n_outer, n_inner, {M});
    if (rc) return rc;
    if (op < 0) return NFM_EINVAL;
    const int code = op & ~NFM_CHOL_FACTORED;
    if (!cholgrad::op_has_grad(code)) return NFM_EINVAL;
    const int cls = symchol::op_class(code);
    if (!cholgrad_fits(dtype == NFM_F64, cls, M)) return NFM_ESIZE;
    const bool has_vec = symchol::op_is_apply(code);
    if ((rc = check_operands(dtype, n_outer, n_inner, {mat, {vec, has_vec}, gout, gpacked}))) return rc;
    const int part = (dtype == NFM_F64 ? 8 : 0) + cls * 4 + (M - 1) / 2;
    const CholParams q{code, (op & NFM_CHOL_FACTORED) ? 1 : 0};
    return switch_order<16>(part + 1, NFM_ESIZE, [&](auto p) {
        constexpr int P = p;
        return cholgrad_part<P>(M, mat, has_vec ? vec : nullptr, gout, gpacked, n_outer, n_inner, q, stream);
    });
}

int nfm_sym_chol_grad_max_order(int dtype, int op_class)
{
    if ((dtype != NFM_F32 && dtype != NFM_F64) || (op_class != NFM_CHOL_CLASS_FACTOR && op_class != NFM_CHOL_CLASS_APPLY))
        return 0;
    return kCholGradCap[dtype == NFM_F64 ? 1 : 0][op_class];
}

int nfm_sym_chol_grad_host(int dtype, int M, int op, int64_t n, const void *mat, const void *vec, const void *gout,
                           void *out)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (n < 0 || op < 0) return NFM_EINVAL;
    const int code = op & ~NFM_CHOL_FACTORED;
    if (!cholgrad::op_has_grad(code)) return NFM_EINVAL;
    if (M < 1 || M > 8) return NFM_ESIZE;
    if (n > 0 && (mat == nullptr || gout == nullptr || out == nullptr || (symchol::op_is_apply(code) && vec == nullptr)))
        return NFM_EINVAL;
    return dtype == NFM_F32 ? cholgrad_host_t<float>(M, op, n, mat, vec, gout, out)
                            : cholgrad_host_t<double>(M, op, n, mat, vec, gout, out);
}

} // extern "C"
#endif
