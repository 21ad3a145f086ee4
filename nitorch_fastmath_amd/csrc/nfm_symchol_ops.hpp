// nfm_symchol_ops.hpp -- the record routines of the Cholesky kernels of `sym` (sym_chol, sym_chol_apply, sym_logdet,
// sym_mahalanobis, sym_gauss_logpdf and the gradient of the three scalars).  Everything is __host__ __device__: the
// kernels of nfm_symchol.hip and the CPU entry nfm_sym_chol_host run the same source, so the host tests hold the
// arithmetic the GPU runs to its bounds on a machine without one.
//
// Storage: compact throughout.  A = L L^T, L lower; L_ij (i >= j) lives at sym_idx(N, i, j).  Inside a routine the
// factor is held as K values with the RECIPROCAL diagonal (l[j] = 1 / L_jj, as chol_solve of nfm_sugar_ops.hpp):
// every substitution multiplies.  The diagonal itself (sd) and the pivots (piv) are returned beside it.
//
// Arithmetic: every sum is an explicit chain of fused multiply-adds in a fixed order and the translation unit is
// compiled without implicit contraction, so the kernels of every layout kind of an Op -- and the host routine, as far
// as sqrt and the division are correctly rounded on both sides -- evaluate the same expression.  Nothing is scaled: no
// intermediate of the factorisation leaves the range of A and sqrt(A), and chol(s^2 A) = s chol(A) bit for bit for a
// power of two s while nothing is subnormal (sqrt, the reciprocal and every product commute with the scaling).
//
// THE BAD-RECORD RULE: a record with an entry (of the matrix or of the vector) that is not finite, or with a pivot
// d_j = a_jj - sum_k l_jk^2 that is not > 0 (NaN, zero and negative alike), is NaN in every value of its result and of
// its gradient.  The routines compute on whatever the record holds and select NaN at the end: no branch, no trap.
#pragma once
#include "nfm_common.hpp"
#include "nfm_symfun_ops.hpp"

namespace nfm {
namespace symchol {

using symfun::finite_t;
using symfun::log_t;
using symfun::nan_t;
using symfun::sqrt_t;

NFM_HD float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
NFM_HD double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// op codes as in include/nfm_hip.h (NFM_CHOL_*); wave-uniform in a kernel
struct CholParams {
    int op;       // NFM_CHOL_* without the flag
    int factored; // the matrix operand already is the factor (apply ops)
};

constexpr bool op_is_apply(int op) { return op >= NFM_CHOL_APPLY_L && op <= NFM_CHOL_APPLY_LTINV; }
constexpr bool op_is_quad(int op) { return op == NFM_CHOL_MAHA || op == NFM_CHOL_MAHA_SQRT || op == NFM_CHOL_LOGPDF; }
constexpr bool op_is_scalar(int op) { return op == NFM_CHOL_LOGDET || op_is_quad(op); }
constexpr bool op_has_vec(int op) { return op_is_apply(op) || op_is_quad(op); }
// the class of an op code (NFM_CHOL_CLASS_*, the second argument of nfm_sym_chol_max_order), -1 for an unknown code
constexpr int op_class(int op)
{
    return op == NFM_CHOL_FACTOR ? NFM_CHOL_CLASS_FACTOR
                                 : (op_is_apply(op) ? NFM_CHOL_CLASS_APPLY : (op_is_scalar(op) ? NFM_CHOL_CLASS_SCALAR : -1));
}
// values per record of the result
constexpr int out_size(int N, int op, bool backward)
{
    if (backward) return sym_k(N) + (op == NFM_CHOL_LOGDET ? 0 : N);
    return op == NFM_CHOL_FACTOR ? sym_k(N) : (op_is_apply(op) ? N : 1);
}

template <typename T, int C>
NFM_HD bool any_not_finite(const T (&x)[C])
{
    bool bad = false;
#pragma unroll
    for (int k = 0; k < C; ++k) bad |= !finite_t(x[k]);
    return bad;
}

// A = L L^T: l = L with the reciprocal diagonal, sd = the diagonal of L, piv = the pivots d_j.  True for a bad record.
template <typename T, int N>
NFM_HD bool factor(const T (&a)[sym_k(N)], T (&l)[sym_k(N)], T (&sd)[N], T (&piv)[N])
{
    bool bad = any_not_finite<T, sym_k(N)>(a);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        T d = a[j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = fma_t(-l[sym_idx(N, j, k)], l[sym_idx(N, j, k)], d);
        bad |= !(d > T(0));
        piv[j] = d;
        sd[j] = sqrt_t(d);
        const T rd = T(1) / sd[j];
        l[j] = rd;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            T s = a[sym_idx(N, i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) s = fma_t(-l[sym_idx(N, i, k)], l[sym_idx(N, j, k)], s);
            l[sym_idx(N, i, j)] = s * rd;
        }
    }
    return bad;
}

// the same three arrays from a factor that is already there (the result of sym_chol): bad unless finite with a
// positive diagonal.  1 / L_jj is the reciprocal `factor` formed, so both routes give the same bits afterwards.
template <typename T, int N>
NFM_HD bool adopt(const T (&f)[sym_k(N)], T (&l)[sym_k(N)], T (&sd)[N])
{
    bool bad = any_not_finite<T, sym_k(N)>(f);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        bad |= !(f[j] > T(0));
        sd[j] = f[j];
        l[j] = T(1) / f[j];
    }
#pragma unroll
    for (int k = N; k < sym_k(N); ++k) l[k] = f[k];
    return bad;
}

// y = L v
template <typename T, int N>
NFM_HD void mul_l(const T (&l)[sym_k(N)], const T (&sd)[N], const T (&v)[N], T (&y)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T s = sd[i] * v[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = fma_t(l[sym_idx(N, i, k)], v[k], s);
        y[i] = s;
    }
}

// y = L^T v
template <typename T, int N>
NFM_HD void mul_lt(const T (&l)[sym_k(N)], const T (&sd)[N], const T (&v)[N], T (&y)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T s = sd[i] * v[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) s = fma_t(l[sym_idx(N, k, i)], v[k], s);
        y[i] = s;
    }
}

// y = L^-1 v (forward substitution; y may be v)
template <typename T, int N>
NFM_HD void solve_l(const T (&l)[sym_k(N)], const T (&v)[N], T (&y)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T s = v[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = fma_t(-l[sym_idx(N, i, k)], y[k], s);
        y[i] = s * l[i];
    }
}

// x = L^-T v (back substitution; x may be v)
template <typename T, int N>
NFM_HD void solve_lt(const T (&l)[sym_k(N)], const T (&v)[N], T (&x)[N])
{
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        T s = v[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) s = fma_t(-l[sym_idx(N, k, i)], x[k], s);
        x[i] = s * l[i];
    }
}

template <typename T, int N>
NFM_HD T sum_squares(const T (&y)[N])
{
    T q = y[0] * y[0];
#pragma unroll
    for (int i = 1; i < N; ++i) q = fma_t(y[i], y[i], q);
    return q;
}

// log det A = sum_j log d_j (= 2 sum_j log L_jj: d_j is the number L_jj was rounded from)
template <typename T, int N>
NFM_HD T log_det(const T (&piv)[N])
{
    T s = log_t(piv[0]);
#pragma unroll
    for (int j = 1; j < N; ++j) s += log_t(piv[j]);
    return s;
}

// the compact inverse (lower triangle, column by column): column j solves L y = e_j from row j on, then L^T x = y
// down to row j.  Each column is a pair of substitutions with the computed factor, so it carries the backward error
// of a solve (|dA| <= 3 gamma |L||L^T|); a product of explicit triangular inverses would not.
template <typename T, int N>
NFM_HD void inverse(const T (&l)[sym_k(N)], T (&x)[sym_k(N)])
{
#pragma unroll
    for (int j = 0; j < N; ++j) {
        x[j] = l[j];
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            T s = -l[sym_idx(N, i, j)] * x[j];
#pragma unroll
            for (int k = j + 1; k < i; ++k) s = fma_t(-l[sym_idx(N, i, k)], x[sym_idx(N, k, j)], s);
            x[sym_idx(N, i, j)] = s * l[i];
        }
#pragma unroll
        for (int i = N - 1; i >= j; --i) {
            T s = x[sym_idx(N, i, j)];
#pragma unroll
            for (int k = i + 1; k < N; ++k) s = fma_t(-l[sym_idx(N, k, i)], x[sym_idx(N, k, j)], s);
            x[sym_idx(N, i, j)] = s * l[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------ the records
template <typename T, int N>
NFM_HD void rec_factor(const T (&a)[sym_k(N)], T (&o)[sym_k(N)])
{
    T l[sym_k(N)], sd[N], piv[N];
    const bool bad = factor<T, N>(a, l, sd, piv);
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = bad ? nan_t<T>() : sd[j];
#pragma unroll
    for (int k = N; k < sym_k(N); ++k) o[k] = bad ? nan_t<T>() : l[k];
}

template <typename T, int N>
NFM_HD void rec_apply(const T (&a)[sym_k(N)], const T (&v)[N], T (&o)[N], const CholParams &q)
{
    T l[sym_k(N)], sd[N], piv[N], y[N];
    bool bad = q.factored ? adopt<T, N>(a, l, sd) : factor<T, N>(a, l, sd, piv);
    bad |= any_not_finite<T, N>(v);
    if (q.op == NFM_CHOL_APPLY_L) mul_l<T, N>(l, sd, v, y);
    else if (q.op == NFM_CHOL_APPLY_LT) mul_lt<T, N>(l, sd, v, y);
    else if (q.op == NFM_CHOL_APPLY_LINV) solve_l<T, N>(l, v, y);
    else solve_lt<T, N>(l, v, y);
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = bad ? nan_t<T>() : y[i];
}

template <typename T, int N>
NFM_HD T rec_logdet(const T (&a)[sym_k(N)])
{
    T l[sym_k(N)], sd[N], piv[N];
    const bool bad = factor<T, N>(a, l, sd, piv);
    return bad ? nan_t<T>() : log_det<T, N>(piv);
}

// N log(2 pi) in the working precision
template <typename T, int N>
NFM_HD T log_two_pi_n()
{
    return T(N * 1.8378770664093454835606594728112353);
}

// v^T A^-1 v = |L^-1 v|^2, its root, or the Gaussian log-density -(N log 2 pi + log det A + v^T A^-1 v) / 2
template <typename T, int N>
NFM_HD T rec_quad(const T (&a)[sym_k(N)], const T (&v)[N], const CholParams &p)
{
    T l[sym_k(N)], sd[N], piv[N], y[N];
    bool bad = factor<T, N>(a, l, sd, piv);
    bad |= any_not_finite<T, N>(v);
    solve_l<T, N>(l, v, y);
    const T q = sum_squares<T, N>(y);
    T r;
    if (p.op == NFM_CHOL_MAHA) r = q;
    else if (p.op == NFM_CHOL_MAHA_SQRT) r = sqrt_t(q);
    else r = T(-0.5) * ((log_det<T, N>(piv) + q) + log_two_pi_n<T, N>());
    return bad ? nan_t<T>() : r;
}

// gradient of log det A for the cotangent g: S = g A^-1, compact (S_ii, 2 S_ij)
template <typename T, int N>
NFM_HD void rec_logdet_bwd(const T (&a)[sym_k(N)], T g, T (&o)[sym_k(N)])
{
    T l[sym_k(N)], sd[N], piv[N], x[sym_k(N)];
    const bool bad = factor<T, N>(a, l, sd, piv);
    inverse<T, N>(l, x);
    const T g2 = T(2) * g;
#pragma unroll
    for (int k = 0; k < sym_k(N); ++k) o[k] = bad ? nan_t<T>() : (k < N ? g : g2) * x[k];
}

// gradient of the three quadratic scalars for the cotangent g, packed [K | N]: with w = A^-1 v
//   squared Mahalanobis   S = -g w w^T,               gv = 2 g w
//   its root d            the same with g / (2 d), exactly zero where d = 0
//   log-density           S = -g (A^-1 - w w^T) / 2,  gv = -g w
// WITH_INV: the log-density (the only one that needs A^-1: its own instantiation, the others stay small)
template <typename T, int N, bool WITH_INV>
NFM_HD void rec_quad_bwd(const T (&a)[sym_k(N)], const T (&v)[N], T g, T (&o)[sym_k(N) + N], const CholParams &p)
{
    constexpr int K = sym_k(N);
    T l[K], sd[N], piv[N], w[N];
    bool bad = factor<T, N>(a, l, sd, piv);
    bad |= any_not_finite<T, N>(v);
    solve_l<T, N>(l, v, w);
    T c = g; // the weight of -w w^T
    if constexpr (!WITH_INV) {
        if (p.op == NFM_CHOL_MAHA_SQRT) {
            const T d = sqrt_t(sum_squares<T, N>(w));
            c = d > T(0) ? g / (T(2) * d) : (d == T(0) ? T(0) : d); // a NaN distance stays a NaN
        }
    } else {
        c = T(0.5) * g;
    }
    solve_lt<T, N>(l, w, w);
    const T cv = WITH_INV ? -g : T(2) * c;
#pragma unroll
    for (int i = 0; i < N; ++i) o[K + i] = bad ? nan_t<T>() : cv * w[i];
    if constexpr (WITH_INV) {
        T x[K];
        inverse<T, N>(l, x);
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                const T s = c * fma_t(w[i], w[j], -x[sym_idx(N, i, j)]);
                o[sym_idx(N, i, j)] = bad ? nan_t<T>() : (i == j ? s : T(2) * s);
            }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                const T s = -c * (w[i] * w[j]);
                o[sym_idx(N, i, j)] = bad ? nan_t<T>() : (i == j ? s : T(2) * s);
            }
    }
}

} // namespace symchol
} // namespace nfm
