// nfm_lstsq_ops.hpp -- per-lane least-squares solves X = A^+ B of one TALL M x N matrix (N <= 8, M up to
// NFM_LSTSQ_MAX_ROWS) and K right-hand sides, by a streaming QR: A^+ B = R^+ (Q^T B) for A = Q R.  The lane holds
// the N x N triangle R and C = Q^T B (N x K) in registers, the M rows of [A | B] pass it once, each eliminated
// against R by N Givens rotations, and the Jacobi routine of nfm_svd_ops.hpp finishes on the N x N system R X = C:
// R has the singular values of A, so the result is the reference's `pinv(a, rcond) @ b` (minimum norm, singular
// values cut at rcond sigma_max).  The per-record routines are __host__ __device__: nfm_lstsq_solve_host runs the
// same arithmetic on the CPU.
//
// Range.  A record is scaled by an exact power of two so that no square leaves the range of T, as svd_solve_rec
// does for a whole record -- but the maximum of a streamed record is not known in advance: the scale is the one
// of the largest |a| of the row blocks seen so far, and when a block raises it R is multiplied by the exact ratio
// of the two powers.  C is not scaled; X is scaled back at the end.  Supported: every finite record.  Entries
// below 2^-63 (float32) / 2^-511 (float64) of the largest entry seen so far have squares that underflow and count
// as zero: they lie below rcond sigma_max for every rcond >= 1e-15 (2^-50), the smallest a caller passes in
// practice, so no singular value that is kept depends on them.  A NaN or an inf
// anywhere in A or B makes the record's X NaN (0 * inf and 0 * NaN in the rotations), and only that record's.
#pragma once
#include "nfm_svd_ops.hpp"

namespace nfm {

constexpr int kLstsqMaxRows = NFM_LSTSQ_MAX_ROWS;
constexpr int kLstsqMaxN = 8;
// rows of [A | B] that are fetched, scanned for their largest |a| and rotated in together.  The same in every
// movement mode and on the host: the scale changes at the same rows everywhere, so every layout of the same
// values gives the same bits.
constexpr int kLstsqRB = 4;

// Largest number of right-hand sides one launch takes at N columns.  The one table of the column caps (kernels
// above a cap are not compiled, nfm_lstsq_solve answers NFM_ESIZE there, the facade reads it through
// nfm_lstsq_max_cols and splits B into blocks of columns).  Every entry is the largest K at which both kernels
// have no private segment (tests/test_lstsq_host.py holds the table to the code objects); the finishing
// svd_solve_rec<T, N, N, K> bounds it by svd_max_k(f64, N, N).
__host__ __device__ constexpr int lstsq_max_k(bool f64, int N)
{
    // float64: R, C, X, one row block in registers and the next one staged -- the LDS-staged kernel spills from
    // K = 7 at N = 6 (124 bytes) and from K = 5 at N = 7 (68 bytes) and N = 8 (192 bytes)
    return !f64 ? 8 : (N <= 5 ? 8 : (N == 6 ? 6 : 4));
}
static_assert(lstsq_max_k(true, 8) <= svd_max_k(true, 8, 8) && lstsq_max_k(true, 7) <= svd_max_k(true, 7, 7) &&
                  lstsq_max_k(true, 6) <= svd_max_k(true, 6, 6) && lstsq_max_k(false, 8) <= svd_max_k(false, 8, 8),
              "the finishing routine's own cap");

// R is held and rotated in double for both dtypes.  Every element of R is rewritten once per row, M times in all,
// and in float32 that rounding adds up to a few eps sigma_max in the directions A does not span: a record of exact
// rank N - 1 kept an N-th singular value above an rcond of 1e-6 (8 eps) in one case of 65.  With R in double the
// streamed factor is exact to float32's eye and its one rounding to float32 comes at the end; C (which decides no
// rank) and the finishing routine stay in T.
using LstsqAcc = double;

template <typename T, int N, int K>
struct LstsqState {
    LstsqAcc r[N][N]; // upper triangle; the zeros below the diagonal are never written
    T c[N][K];
    T amax;  // largest |a| seen so far
    T scale; // svd_unit(amax): the power of two the rows of A are multiplied by
};

template <typename T, int N, int K>
__host__ __device__ __forceinline__ void lstsq_init(LstsqState<T, N, K> &st)
{
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int k = 0; k < N; ++k) st.r[j][k] = LstsqAcc(0);
#pragma unroll
        for (int k = 0; k < K; ++k) st.c[j][k] = T(0);
    }
    st.amax = T(0);
    st.scale = T(1);
}

// The fused multiply-adds of a rotation are written out: which of two products the compiler fuses into the sum
// would otherwise be its choice per kernel, and the kernels of the movement modes must give the same bits.
__host__ __device__ __forceinline__ float lstsq_fma(float x, float y, float z) { return __builtin_fmaf(x, y, z); }
__host__ __device__ __forceinline__ double lstsq_fma(double x, double y, double z) { return __builtin_fma(x, y, z); }

// c = f / h, s = g / h for h^2 = f^2 + g^2.  h^2 > 0 is false for two zeros and for NaN: the identity.
// float64 records: 1 / sqrt in double.  float32 records: the float32 reciprocal square root and one Newton step
// in double (relative error 1e-14: far below float32's eps, without double's square root and division); an h^2
// below float32's range counts as zero, like every square that underflows (header comment).
template <typename T>
__host__ __device__ __forceinline__ void lstsq_rot(double f, double g, double h2, double &cs, double &sn)
{
    bool ok;
    double inv;
    if constexpr (sizeof(T) == 8) {
        ok = h2 > 0.0;
        inv = 1.0 / svd_sqrt(h2);
    } else {
        const float h2f = (float)h2;
        ok = h2f > 0.0f;
        const double i0 = (double)(1.0f / svd_sqrt(h2f));
        inv = i0 * lstsq_fma(-0.5 * h2, i0 * i0, 1.5);
    }
    cs = ok ? f * inv : 1.0;
    sn = ok ? g * inv : 0.0;
}

// one row (a, b) of [A | B], a already scaled: rotation j is formed from (R_jj, a_j) and applied to row j of R
// from column j on, to the row, and to row j of C and b.  The identity's 0 * a_j carries a NaN into R.  No branch,
// no loop that an input could prolong.
template <typename T, int N, int K>
__host__ __device__ __forceinline__ void lstsq_row(LstsqState<T, N, K> &st, const T (&a)[N], T (&b)[K])
{
    LstsqAcc ar[N];
#pragma unroll
    for (int j = 0; j < N; ++j) ar[j] = (LstsqAcc)a[j];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const LstsqAcc f = st.r[j][j], g = ar[j];
        const LstsqAcc h2 = lstsq_fma(f, f, g * g);
        LstsqAcc cs, sn;
        lstsq_rot<T>(f, g, h2, cs, sn);
#pragma unroll
        for (int k = j; k < N; ++k) {
            const LstsqAcc u = st.r[j][k], v = ar[k];
            st.r[j][k] = lstsq_fma(cs, u, sn * v);
            ar[k] = lstsq_fma(cs, v, -(sn * u));
        }
        const T ct = (T)cs, st_ = (T)sn;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T u = st.c[j][k], v = b[k];
            st.c[j][k] = lstsq_fma(ct, u, st_ * v);
            b[k] = lstsq_fma(ct, v, -(st_ * u));
        }
    }
}

// `rows` (1..kLstsqRB, the same for every lane) rows of [A | B]: raise the running scale, then rotate them in
template <typename T, int N, int K>
__host__ __device__ __forceinline__ void lstsq_block(LstsqState<T, N, K> &st, T (&a)[kLstsqRB][N],
                                                     T (&b)[kLstsqRB][K], int rows)
{
    T amax = st.amax;
#pragma unroll
    for (int i = 0; i < kLstsqRB; ++i)
        if (i < rows) {
#pragma unroll
            for (int j = 0; j < N; ++j) amax = svd_max(amax, svd_abs(a[i][j]));
        }
    const T scale = svd_unit(amax, SvdEps<T>::emax);
    const T ratio = scale / st.scale; // a power of two <= 1 (0 when the two are further apart than T's range)
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int k = j; k < N; ++k) st.r[j][k] *= (LstsqAcc)ratio;
    st.amax = amax;
    st.scale = scale;
#pragma unroll
    for (int i = 0; i < kLstsqRB; ++i)
        if (i < rows) {
#pragma unroll
            for (int j = 0; j < N; ++j) a[i][j] *= scale;
            lstsq_row<T, N, K>(st, a[i], b[i]);
        }
}

// X = R^+ C by the Jacobi routine (R as an N x N array with its zeros), scaled back.  Rank deficiency is
// resolved by rcond alone: at M == N the routine has no null-row clause.  Returns its sweep count.
template <typename T, int N, int K>
__host__ __device__ __forceinline__ int lstsq_finish(LstsqState<T, N, K> &st, T (&x)[N][K], T rc2)
{
    T r[N][N];
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int k = 0; k < N; ++k) r[j][k] = (T)st.r[j][k];
    const int sweeps = svd_solve_rec<T, N, N, K>(r, st.c, x, /*pinv=*/true, rc2);
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) x[j][k] *= st.scale;
    return sweeps;
}

} // namespace nfm
