// nfm_symchol.hip -- Cholesky kernels of compact symmetric positive definite matrices (sym_chol, sym_chol_apply,
// sym_logdet, sym_mahalanobis, sym_gauss_logpdf and the gradient of the three scalars; an extension of `sym`, no
// counterpart in the reference).  One record per lane through rec_kernel, as nfm_symeig.hip: read the
// K = N (N + 1) / 2 compact values (and the N of the vector), factor in registers, write the result.  The record
// routines, the bad-record rule and the arithmetic are those of nfm_symchol_ops.hpp, shared with the CPU entry.
// The op of a class is a run-time member of Params (wave-uniform): the instantiations are
// (dtype, N, Op struct) x the layout kinds of rec_launch.  Compiled without implicit contraction (csrc/Makefile), so
// that every layout kind of an Op gives the same bits.
#include "nfm_record_kernel.hpp"
#include "nfm_symchol_ops.hpp"

// This file is compiled 33 times (-DNFM_SYMCHOL_PART=0..32).  Part 0: the entry points, the caps and the CPU routine.
// Parts 1..32: the kernels of one (dtype, class, pair of orders): part = 1 + dtype * 16 + class * 4 + pair, class =
// NFM_CHOL_CLASS_*, pair p = orders 2p + 1 and 2p + 2.  Each of them defines its own specialisation of
// symchol_part<PART>; part 0 reaches them through switch_order<32>.
#ifndef NFM_SYMCHOL_PART
#error "compile with -DNFM_SYMCHOL_PART=0..32"
#endif

namespace nfm {

using symchol::CholParams;

// The compiled caps: the largest order of each (dtype, class) whose kernels have no private segment in any layout form
// (profiles/symchol_table.md lists the registers).  Orders above take the caller's own route.
constexpr int kSymCholCap[2][4] = {{8, 8, 8, 8}, {8, 8, 8, 8}}; // [dtype][NFM_CHOL_CLASS_*]
constexpr bool symchol_fits(bool f64, int cls, int N) { return N >= 1 && N <= kSymCholCap[f64 ? 1 : 0][cls]; }

// TILE and kNoTile: the rule of SymEigOp / SymFunOp (from these orders on a lane fetches its record itself) for the Ops
// whose result is a vector or a scalar.  The Ops that WRITE a record as large as the matrix (the factor, the
// gradients) stage every order through the LDS tile: measured against the other rule in one process, same bits, the
// factor takes 0.58-0.79 and the log-density gradient 0.70-0.86 of the time at N >= 5 (float64: N >= 4), where the
// per-lane stores of a K-value record bound the kernel; the vector and scalar Ops are mixed, 0.90-1.24
// (profiles/symchol_tile_ab.md).
// Kernel experiment: -DNFM_SYMCHOL_TILE=0 builds every Op under the spectral kernels' rule, =1 every Op tiled at every
// order (make symchol-exp SYMCHOL_DEFS=...; scripts/bench_symchol_builds.py compares two such builds in one process).
template <typename T, int N>
constexpr bool symchol_no_tile(bool wide_result)
{
#ifdef NFM_SYMCHOL_TILE
    wide_result = NFM_SYMCHOL_TILE != 0;
#endif
    return !wide_result && (N >= 5 || (N == 4 && sizeof(T) == 8));
}

template <typename T, int N>
struct CholFactorOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>;
    using RB = NoRec;
    using RC = NoRec;
    using RO = Rec<1, K>;
    using Params = CholParams;
    static constexpr int TILE = pick_tile((RA::C + RO::C) * (int)sizeof(T) + 32);
    static constexpr bool kNoTile = symchol_no_tile<T, N>(true);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&)[1], const T (&)[1], T (&o)[RO::Cs],
                                                 const Params &)
    {
        symchol::rec_factor<T, N>(a, o);
    }
};

// L v, L^T v, L^-1 v, L^-T v; the matrix operand is A or, with q.factored, L
template <typename T, int N>
struct CholApplyOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>;
    using RB = Rec<1, N>;
    using RC = NoRec;
    using RO = Rec<1, N>;
    using Params = CholParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RO::C) * (int)sizeof(T) + 48);
    static constexpr bool kNoTile = symchol_no_tile<T, N>(false);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&v)[RB::Cs], const T (&)[1],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        symchol::rec_apply<T, N>(a, v, o, q);
    }
};

template <typename T, int N>
struct CholLogdetOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>;
    using RB = NoRec;
    using RC = NoRec;
    using RO = Rec<1, 1>;
    using Params = CholParams;
    static constexpr int TILE = pick_tile((RA::C + RO::C) * (int)sizeof(T) + 32);
    static constexpr bool kNoTile = symchol_no_tile<T, N>(false);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&)[1], const T (&)[1], T (&o)[RO::Cs],
                                                 const Params &)
    {
        o[0] = symchol::rec_logdet<T, N>(a);
    }
};

// squared Mahalanobis distance, its root, Gaussian log-density: K + N values read, one written
template <typename T, int N>
struct CholQuadOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>;
    using RB = Rec<1, N>;
    using RC = NoRec;
    using RO = Rec<1, 1>;
    using Params = CholParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RO::C) * (int)sizeof(T) + 48);
    static constexpr bool kNoTile = symchol_no_tile<T, N>(false);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&v)[RB::Cs], const T (&)[1],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        o[0] = symchol::rec_quad<T, N>(a, v, q);
    }
};

template <typename T, int N>
struct CholLogdetBwdOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>; // compact A
    using RB = Rec<1, 1>; // cotangent of the value
    using RC = NoRec;
    using RO = Rec<1, K>; // compact gradient
    using Params = CholParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RO::C) * (int)sizeof(T) + 48);
    static constexpr bool kNoTile = symchol_no_tile<T, N>(true);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&g)[RB::Cs], const T (&)[1],
                                                 T (&o)[RO::Cs], const Params &)
    {
        symchol::rec_logdet_bwd<T, N>(a, g[0], o);
    }
};

template <typename T, int N, bool WITH_INV>
struct CholQuadBwdOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>;     // compact A
    using RB = Rec<1, N>;     // the vector
    using RC = Rec<1, 1>;     // cotangent of the value
    using RO = Rec<1, K + N>; // packed gradient [K | N]
    using Params = CholParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RC::C + RO::C) * (int)sizeof(T) + 64);
    static constexpr bool kNoTile = symchol_no_tile<T, N>(true);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&v)[RB::Cs], const T (&g)[RC::Cs],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        symchol::rec_quad_bwd<T, N, WITH_INV>(a, v, g[0], o, q);
    }
};

// one launcher per part: (M, backward, mat, vec or NULL, gout or NULL, out)
#define NFM_SYMCHOL_ARGS                                                                                               \
    int M, bool backward, const nfm_operand *a, const nfm_operand *v, const nfm_operand *g, const nfm_operand *o,      \
        int64_t no, int64_t ni, const CholParams &q, void *stream
template <int PART>
int symchol_part(NFM_SYMCHOL_ARGS);

#if NFM_SYMCHOL_PART >= 1
template <>
int symchol_part<NFM_SYMCHOL_PART>(NFM_SYMCHOL_ARGS)
{
    constexpr int part = NFM_SYMCHOL_PART - 1;
    constexpr bool F64 = part / 16 != 0;
    constexpr int CLS = (part / 4) % 4;
    constexpr int N0 = 2 * (part % 4) + 1;
    using T = std::conditional_t<F64, double, float>;
    auto run = [&](auto n) -> int {
        constexpr int N = decltype(n)::value;
        if constexpr (symchol_fits(F64, CLS, N)) {
            if constexpr (CLS == NFM_CHOL_CLASS_FACTOR)
                return rec_launch<T, CholFactorOp<T, N>>(a, nullptr, nullptr, o, no, ni, q, stream);
            else if constexpr (CLS == NFM_CHOL_CLASS_APPLY)
                return rec_launch<T, CholApplyOp<T, N>>(a, v, nullptr, o, no, ni, q, stream);
            else if constexpr (CLS == NFM_CHOL_CLASS_SCALAR) {
                if (q.op == NFM_CHOL_LOGDET)
                    return rec_launch<T, CholLogdetOp<T, N>>(a, nullptr, nullptr, o, no, ni, q, stream);
                return rec_launch<T, CholQuadOp<T, N>>(a, v, nullptr, o, no, ni, q, stream);
            } else {
                if (q.op == NFM_CHOL_LOGDET)
                    return rec_launch<T, CholLogdetBwdOp<T, N>>(a, g, nullptr, o, no, ni, q, stream);
                if (q.op == NFM_CHOL_LOGPDF)
                    return rec_launch<T, CholQuadBwdOp<T, N, true>>(a, v, g, o, no, ni, q, stream);
                return rec_launch<T, CholQuadBwdOp<T, N, false>>(a, v, g, o, no, ni, q, stream);
            }
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

#if NFM_SYMCHOL_PART == 0
using namespace nfm;

// the checks of nfm_sym_funm in its order: the batch, the op code, the cap (then the operands)
static int symchol_check(int dtype, int M, int op, bool backward, int64_t n_outer, int64_t n_inner)
{
    const int rc = check_batch(dtype, n_outer, n_inner, {M});
    if (rc) return rc;
    if (op < 0) return NFM_EINVAL;
    const int code = op & ~NFM_CHOL_FACTORED;
    if (symchol::op_class(code) < 0) return NFM_EINVAL;
    if ((op & NFM_CHOL_FACTORED) && !symchol::op_is_apply(code)) return NFM_EINVAL;
    if (backward && !symchol::op_is_scalar(code)) return NFM_EINVAL;
    const int cls = backward ? NFM_CHOL_CLASS_BACKWARD : symchol::op_class(code);
    if (!symchol_fits(dtype == NFM_F64, cls, M)) return NFM_ESIZE;
    return NFM_OK;
}

static int symchol_dispatch(int dtype, int M, int cls, bool backward, const nfm_operand *a, const nfm_operand *v,
                            const nfm_operand *g, const nfm_operand *o, int64_t no, int64_t ni, const CholParams &q,
                            void *stream)
{
    const int part = (dtype == NFM_F64 ? 16 : 0) + cls * 4 + (M - 1) / 2;
    return switch_order<32>(part + 1, NFM_ESIZE, [&](auto p) {
        constexpr int P = p;
        return symchol_part<P>(M, backward, a, v, g, o, no, ni, q, stream);
    });
}

// n contiguous host records through the record routines of nfm_symchol_ops.hpp
template <typename T, int N>
static void symchol_host_n(int op, int64_t n, const T *mat, const T *vec, const T *gout, T *out)
{
    constexpr int K = sym_k(N);
    const CholParams q{op & ~NFM_CHOL_FACTORED, (op & NFM_CHOL_FACTORED) ? 1 : 0};
    for (int64_t b = 0; b < n; ++b) {
        T a[K], v[N];
        for (int k = 0; k < K; ++k) a[k] = mat[b * K + k];
        for (int i = 0; i < N; ++i) v[i] = symchol::op_has_vec(q.op) ? vec[b * N + i] : T(0);
        if (gout) {
            if (q.op == NFM_CHOL_LOGDET) {
                T o[K];
                symchol::rec_logdet_bwd<T, N>(a, gout[b], o);
                for (int k = 0; k < K; ++k) out[b * K + k] = o[k];
            } else {
                T o[K + N];
                if (q.op == NFM_CHOL_LOGPDF) symchol::rec_quad_bwd<T, N, true>(a, v, gout[b], o, q);
                else symchol::rec_quad_bwd<T, N, false>(a, v, gout[b], o, q);
                for (int k = 0; k < K + N; ++k) out[b * (K + N) + k] = o[k];
            }
        } else if (q.op == NFM_CHOL_FACTOR) {
            T o[K];
            symchol::rec_factor<T, N>(a, o);
            for (int k = 0; k < K; ++k) out[b * K + k] = o[k];
        } else if (symchol::op_is_apply(q.op)) {
            T o[N];
            symchol::rec_apply<T, N>(a, v, o, q);
            for (int i = 0; i < N; ++i) out[b * N + i] = o[i];
        } else if (q.op == NFM_CHOL_LOGDET) {
            out[b] = symchol::rec_logdet<T, N>(a);
        } else {
            out[b] = symchol::rec_quad<T, N>(a, v, q);
        }
    }
}

template <typename T>
static int symchol_host_t(int M, int op, int64_t n, const void *mat, const void *vec, const void *gout, void *out)
{
    return switch_order<8>(M, NFM_ESIZE, [&](auto nn) {
        constexpr int NN = nn;
        symchol_host_n<T, NN>(op, n, static_cast<const T *>(mat), static_cast<const T *>(vec),
                              static_cast<const T *>(gout), static_cast<T *>(out));
        return (int)NFM_OK;
    });
}

extern "C" {

int nfm_sym_chol(int dtype, int M, int op, int64_t n_outer, int64_t n_inner, const nfm_operand *mat,
                 const nfm_operand *vec, const nfm_operand *out, void *stream)
{
    int rc = symchol_check(dtype, M, op, false, n_outer, n_inner);
    if (rc) return rc;
    const int code = op & ~NFM_CHOL_FACTORED;
    const bool has_vec = symchol::op_has_vec(code);
    if ((rc = check_operands(dtype, n_outer, n_inner, {mat, {vec, has_vec}, out}))) return rc;
    return symchol_dispatch(dtype, M, symchol::op_class(code), false, mat, has_vec ? vec : nullptr, nullptr, out, n_outer,
                            n_inner, CholParams{code, (op & NFM_CHOL_FACTORED) ? 1 : 0}, stream);
}

int nfm_sym_chol_backward(int dtype, int M, int op, int64_t n_outer, int64_t n_inner, const nfm_operand *mat,
                          const nfm_operand *vec, const nfm_operand *gout, const nfm_operand *gpacked, void *stream)
{
    int rc = symchol_check(dtype, M, op, true, n_outer, n_inner);
    if (rc) return rc;
    const bool has_vec = symchol::op_has_vec(op);
    if ((rc = check_operands(dtype, n_outer, n_inner, {mat, {vec, has_vec}, gout, gpacked}))) return rc;
    return symchol_dispatch(dtype, M, NFM_CHOL_CLASS_BACKWARD, true, mat, has_vec ? vec : nullptr, gout, gpacked,
                            n_outer, n_inner, CholParams{op, 0}, stream);
}

int nfm_sym_chol_max_order(int dtype, int op_class)
{
    if ((dtype != NFM_F32 && dtype != NFM_F64) || op_class < 0 || op_class > 3) return 0;
    return kSymCholCap[dtype == NFM_F64 ? 1 : 0][op_class];
}

int nfm_sym_chol_host(int dtype, int M, int op, int64_t n, const void *mat, const void *vec, const void *gout,
                      void *out)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (n < 0 || op < 0) return NFM_EINVAL;
    const int code = op & ~NFM_CHOL_FACTORED;
    if (symchol::op_class(code) < 0 || ((op & NFM_CHOL_FACTORED) && !symchol::op_is_apply(code))) return NFM_EINVAL;
    if (gout && !symchol::op_is_scalar(code)) return NFM_EINVAL;
    if (M < 1 || M > 8) return NFM_ESIZE;
    if (n > 0 && (mat == nullptr || out == nullptr || (symchol::op_has_vec(code) && vec == nullptr))) return NFM_EINVAL;
    return dtype == NFM_F32 ? symchol_host_t<float>(M, op, n, mat, vec, gout, out)
                            : symchol_host_t<double>(M, op, n, mat, vec, gout, out);
}

} // extern "C"
#endif
