// nfm_cholgrad_ops.hpp -- the record routines of the gradient of the Cholesky factor itself (the backward pass of
// sym_chol and of sym_chol_apply).  __host__ __device__ as nfm_symchol_ops.hpp, whose factor, substitutions and
// bad-record rule they use: the kernels of nfm_cholgrad.hip and the CPU entry nfm_sym_chol_grad_host run this source.
//
// The factor.  A = L L^T, G the cotangent of L: compact, one value per stored entry L_ij (i >= j), each counted once.
//     M = Phi(L^T G) + Phi(L^T G)^T      Phi keeps the lower triangle and halves the diagonal, so M is the symmetric
//                                        matrix whose lower triangle, diagonal included, is that of L^T G
//     S = L^-T M L^-1 / 2                returned as (S_ii, 2 S_ij), the convention of nfm_sym_chol_backward
// Both steps run in place on the K values of the working copy of G:
//     pull_lt      M_ij = sum_{k >= i} L_ki G_kj, column by column, row i before row i + 1 (row i reads rows >= i only)
//     congruence   W = L^-T M L^-1 as two sweeps of substitutions with the computed factor.  X = M L^-1 row by row
//                  from the first (a row of N temporaries; its lower part replaces the row of M, which no later row
//                  reads), then W = L^-T X from the last row up, which needs the lower triangle of X only.  Every
//                  row and every column is one substitution, so the result carries the backward error of a solve
//                  on either side (|dL| <= gamma |L| per right-hand side) and nothing else.  (The one-sweep two-sided
//                  form that updates the trailing block by rank-two terms is cheaper by a third and missed the
//                  bounds of tests/_cholgrad_ref.py at cond 1e10 in float64: not used.)
// The live values are l, the working copy and one row: 2K + 2N.
//
// Arithmetic: explicit chains of fused multiply-adds in a fixed order, no implicit contraction, nothing scaled.  For a
// power of two s the gradient at s^2 A is the gradient at A divided by s, bit for bit, while nothing is subnormal:
// every product and every reciprocal commutes with the scaling.
//
// The four apply ops, y the forward result and g its cotangent (N values):
//     'L'      gv = L^T g     G = tril(g v^T)            'LT'      gv = L g      G = tril(v g^T)
//     'Linv'   gv = L^-T g    G = -tril(gv y^T)          'LTinv'   gv = L^-1 g   G = -tril(y gv^T)
// With `factored` the matrix operand is the factor and the result is [G | gv], G plain (one value per stored entry);
// without, G goes through the factor routine in the same lane and the result is [S | gv].
//
// Bad records: those of the forward ops (an entry of the matrix or the vector that is not finite, a pivot that is not
// > 0, with `factored` a diagonal that is not > 0) and a cotangent entry that is not finite.  NaN in every value,
// selected at the end.
#pragma once
#include "nfm_symchol_ops.hpp"

namespace nfm {
namespace cholgrad {

using symchol::adopt;
using symchol::any_not_finite;
using symchol::CholParams;
using symchol::factor;
using symchol::fma_t;
using symchol::mul_l;
using symchol::mul_lt;
using symchol::nan_t;
using symchol::solve_l;
using symchol::solve_lt;

// the op codes nfm_sym_chol_grad accepts (without the flag)
constexpr bool op_has_grad(int op) { return op == NFM_CHOL_FACTOR || symchol::op_is_apply(op); }

// the lower triangle (diagonal included) of L^T G, in place on g
template <typename T, int N>
NFM_HD void pull_lt(const T (&l)[sym_k(N)], const T (&sd)[N], T (&g)[sym_k(N)])
{
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int i = j; i < N; ++i) {
            T s = sd[i] * g[sym_idx(N, i, j)];
#pragma unroll
            for (int k = i + 1; k < N; ++k) s = fma_t(l[sym_idx(N, k, i)], g[sym_idx(N, k, j)], s);
            g[sym_idx(N, i, j)] = s;
        }
}

// W = L^-T M L^-1 in place on the compact symmetric m (l holds the reciprocal diagonal): two sweeps of substitutions
template <typename T, int N>
NFM_HD void congruence(const T (&l)[sym_k(N)], T (&m)[sym_k(N)])
{
    // X = M L^-1 row by row from the first: x L = (row i of M), solved from the last column down.  Row i reads its own
    // lower part and, for the columns past i, the rows below it, which still hold M; the lower part of X replaces it.
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T x[N];
#pragma unroll
        for (int j = N - 1; j >= 0; --j) {
            T s = m[sym_idx(N, i, j)];
#pragma unroll
            for (int p = j + 1; p < N; ++p) s = fma_t(-x[p], l[sym_idx(N, p, j)], s);
            x[j] = s * l[j];
        }
#pragma unroll
        for (int j = 0; j <= i; ++j) m[sym_idx(N, i, j)] = x[j];
    }
    // W = L^-T X from the last row up: the lower triangle of W needs the lower triangle of X only
#pragma unroll
    for (int i = N - 1; i >= 0; --i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            T s = m[sym_idx(N, i, j)];
#pragma unroll
            for (int p = i + 1; p < N; ++p) s = fma_t(-l[sym_idx(N, p, i)], m[sym_idx(N, p, j)], s);
            m[sym_idx(N, i, j)] = s * l[i];
        }
}

// the cotangent of L (in g) -> the gradient with respect to A, compact (S_ii, 2 S_ij), in place
template <typename T, int N>
NFM_HD void factor_pullback(const T (&l)[sym_k(N)], const T (&sd)[N], T (&g)[sym_k(N)])
{
    pull_lt<T, N>(l, sd, g);
    congruence<T, N>(l, g);
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] *= T(0.5);
}

// ------------------------------------------------------------------------------------------------ the records
// gradient of sym_chol: a = A, or with q.factored its factor; gout = the cotangent of the factor
template <typename T, int N>
NFM_HD void rec_factor_grad(const T (&a)[sym_k(N)], const T (&gout)[sym_k(N)], T (&o)[sym_k(N)], const CholParams &q)
{
    constexpr int K = sym_k(N);
    T l[K], sd[N], piv[N], m[K];
    bool bad = q.factored ? adopt<T, N>(a, l, sd) : factor<T, N>(a, l, sd, piv);
    bad |= any_not_finite<T, K>(gout);
#pragma unroll
    for (int k = 0; k < K; ++k) m[k] = gout[k];
    factor_pullback<T, N>(l, sd, m);
#pragma unroll
    for (int k = 0; k < K; ++k) o[k] = bad ? nan_t<T>() : m[k];
}

// gradient of sym_chol_apply, packed [K | N]: with respect to the matrix operand (A, or the factor with q.factored),
// then with respect to the vector
template <typename T, int N>
NFM_HD void rec_apply_grad(const T (&a)[sym_k(N)], const T (&v)[N], const T (&g)[N], T (&o)[sym_k(N) + N],
                           const CholParams &q)
{
    constexpr int K = sym_k(N);
    T l[K], sd[N], piv[N], gv[N], m[K];
    bool bad = q.factored ? adopt<T, N>(a, l, sd) : factor<T, N>(a, l, sd, piv);
    bad |= any_not_finite<T, N>(v);
    bad |= any_not_finite<T, N>(g);
    if (q.op == NFM_CHOL_APPLY_L) {
        mul_lt<T, N>(l, sd, g, gv);
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) m[sym_idx(N, i, j)] = g[i] * v[j];
    } else if (q.op == NFM_CHOL_APPLY_LT) {
        mul_l<T, N>(l, sd, g, gv);
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) m[sym_idx(N, i, j)] = v[i] * g[j];
    } else if (q.op == NFM_CHOL_APPLY_LINV) {
        T y[N];
        solve_l<T, N>(l, v, y);
        solve_lt<T, N>(l, g, gv);
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) m[sym_idx(N, i, j)] = -(gv[i] * y[j]);
    } else {
        T y[N];
        solve_lt<T, N>(l, v, y);
        solve_l<T, N>(l, g, gv);
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) m[sym_idx(N, i, j)] = -(y[i] * gv[j]);
    }
    if (!q.factored) factor_pullback<T, N>(l, sd, m);
#pragma unroll
    for (int k = 0; k < K; ++k) o[k] = bad ? nan_t<T>() : m[k];
#pragma unroll
    for (int i = 0; i < N; ++i) o[K + i] = bad ? nan_t<T>() : gv[i];
}

} // namespace cholgrad
} // namespace nfm
