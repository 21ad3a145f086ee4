// nfm_sympencil_ops.hpp -- the per-record arithmetic of the two-matrix spectral kernels (nfm_sympencil.hip):
// the simultaneous reduction of a pencil (A, B), A symmetric positive definite and B symmetric, both compact.
//
//   1. A = V L V^T (eig_sym1, fast sweeps), W = V L^-1/2 so that W^T A W = I; Y = V L^1/2 = W L = W^-T
//   2. C = W^T B W, symmetric: one column of B W at a time, then the rows above the diagonal
//   3. C = Q M Q^T (eig_sym1 again), X = W Q, Z = Y Q: X^T A X = I, X^T B X = M, Z = X^-T
//
// A's triangle, its reflectors and V die before the second decomposition: only W and L live across it.
// Every function of the pencil is then Z f(M) Z^T = A^1/2 f(A^-1/2 B A^-1/2) A^1/2, its gradient with respect to B
// is X [(Z^T G Z) o F] X^T with the closed-form divided differences of nfm_symfun_ops.hpp, and the squared
// affine-invariant distance is sum_i log^2 mu_i with the gradients X diag(2 log mu / mu) X^T (B) and
// -X diag(2 log mu) X^T (A): no divided difference, exact at A = B.
#pragma once
#include "nfm_spectral.hpp"

namespace nfm {
namespace sympencil {

// what nfm_sym_pencil_eig returns
enum { MODE_EIG = 0, MODE_DIST2 = 1, MODE_DIST = 2 };
struct EigParams {
    int mode;
};

// steps 1 and 2: w = W, lam = L (1 for a bad record), c = C mirrored.  Returns the bad flag: an entry of A or B
// that is not finite, an eigenvalue of A that is not positive, or a C that is not finite (a base whose
// conditioning is beyond the format).  A bad record leaves with C = I, so the second sweeps stay short.
template <typename T, int N>
__device__ __forceinline__ bool whiten(const T (&ra)[sym_k(N)], const T (&rb)[sym_k(N)], T (&w)[N][N], T (&lam)[N],
                                       T (&c)[N][N])
{
    bool bad;
    {
        T a[N][N], up[N][N];
        bad = spectral::expand<T, N>(ra, a);
        qr::eig_sym1<T, N, true, true>(a, w, up, lam, N, spectral::kMaxIter, spectral::kTol);
    } // a and up die here
    bool badb = false;
#pragma unroll
    for (int k = 0; k < sym_k(N); ++k) badb |= !symfun::finite_t(rb[k]);
#pragma unroll
    for (int k = 0; k < N; ++k) bad |= !(symfun::finite_t(lam[k]) && lam[k] > T(0));
#pragma unroll
    for (int k = 0; k < N; ++k) {
        lam[k] = bad ? T(1) : lam[k];
        const T rs = T(1) / symfun::sqrt_t(lam[k]);
#pragma unroll
        for (int i = 0; i < N; ++i) w[i][k] *= rs;
    }
    bad |= badb;
    // column l of B W, then C_kl for k <= l (the congruence of PencilFunBwdOp and SymFunBwdOp without the halving)
    bool badc = false;
#pragma unroll
    for (int l = 0; l < N; ++l) {
        T t[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            T s = rb[i] * w[i][l];
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (j != i) s = qr::fma_t(rb[sym_idx(N, i, j)], w[j][l], s);
            t[i] = s;
        }
#pragma unroll
        for (int k = 0; k <= l; ++k) {
            T s = w[0][k] * t[0];
#pragma unroll
            for (int i = 1; i < N; ++i) s = qr::fma_t(w[i][k], t[i], s);
            badc |= !symfun::finite_t(s);
            c[k][l] = s;
            c[l][k] = s;
        }
    }
    bad |= badc;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) c[i][j] = bad ? T(i == j) : c[i][j];
    return bad;
}

// m <- (m diag(s)) q (SCALE) or m q, in place, a row at a time
template <typename T, int N, bool SCALE>
__device__ __forceinline__ void times_q(T (&m)[N][N], const T (&s)[N], const T (&q)[N][N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T t[N];
#pragma unroll
        for (int k = 0; k < N; ++k) t[k] = SCALE ? m[i][k] * s[k] : m[i][k];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            T y = t[0] * q[0][j];
#pragma unroll
            for (int k = 1; k < N; ++k) y = qr::fma_t(t[k], q[k][j], y);
            m[i][j] = y;
        }
    }
}

// ascending order by compare-exchange (an odd-even transposition network: N rounds)
template <typename T, int N>
__device__ __forceinline__ void sort_up(T (&v)[N])
{
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int i = r & 1; i + 1 < N; i += 2) {
            const T lo = v[i] < v[i + 1] ? v[i] : v[i + 1];
            const T hi = v[i] < v[i + 1] ? v[i + 1] : v[i];
            v[i] = lo;
            v[i + 1] = hi;
        }
}

// is a positive and finite, b finite?  (the scalar pencil)
template <typename T>
__device__ __forceinline__ bool scalar_ok(T a, T b)
{
    return symfun::finite_t(a) && a > T(0) && symfun::finite_t(b);
}

} // namespace sympencil
} // namespace nfm
