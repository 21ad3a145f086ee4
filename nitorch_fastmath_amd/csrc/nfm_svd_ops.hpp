// nfm_svd_ops.hpp -- per-lane least-squares / minimum-norm solves X = A^+ B of one small M x N matrix and a matrix
// of K right-hand sides by a one-sided (Hestenes) Jacobi SVD (the `Op` structs of nfm_svd.hip: `lmdiv`, `rmdiv`,
// `solvevec`, `inv` of the reference's `sugar.py` with method 'svd' / 'pinv', and every non-square system;
// file:line citations are relative to the reference package).  The per-record routine is __host__ __device__:
// nfm_svd_solve_host runs the same arithmetic on the CPU.
#pragma once
#include "nfm_record_kernel.hpp"

namespace nfm {

constexpr int kSvdMaxDim = NFM_SVD_MAX_DIM;
// The sweep loop is a run-time loop with a compile-time cap: no input keeps the kernel running.  The largest
// count seen over the test inputs is in DESIGN.md section 4.11.
constexpr int kSvdMaxSweeps = NFM_SVD_MAX_SWEEPS;

// Largest number of right-hand sides one launch takes for an M x N record: [A | B] is M (N + K) values per lane,
// the N x K result and the staging registers of the LDS tiles come on top.  The one table of the column caps:
// the kernels above a cap are not compiled, nfm_svd_solve answers NFM_ESIZE there, and the facade (which reads
// the cap through nfm_svd_max_cols) splits B into blocks of columns.  Every entry is the largest K whose
// kernels, all kinds, have no private segment (tests/test_svd_host.py holds the table to the code objects).
__host__ __device__ constexpr int svd_max_k(bool f64, int M, int N)
{
    // float64 beyond 168 values of A, B and X per lane: the run-time-mode kernel spills (8 x 8 from K = 7,
    // 8 x 7 and 7 x 8 at K = 8)
    return !f64 ? 8 : (M + N == 16 ? 6 : (M + N == 15 ? 7 : 8));
}

struct SvdParams {
    int pinv;     // NFM_SVD_PINV: drop the rows with sigma <= rcond sigma_max
    double rcond; // (squared in the record's arithmetic: the routine compares sigma^2)
};

template <typename T>
struct SvdEps;
template <>
struct SvdEps<float> {
    static constexpr float eps = 1.1920929e-07f;
    static constexpr int emax = 120;
};
template <>
struct SvdEps<double> {
    static constexpr double eps = 2.220446049250313e-16;
    static constexpr int emax = 1000;
};

__host__ __device__ __forceinline__ float svd_abs(float x) { return __builtin_fabsf(x); }
__host__ __device__ __forceinline__ double svd_abs(double x) { return __builtin_fabs(x); }
__host__ __device__ __forceinline__ float svd_max(float x, float y) { return __builtin_fmaxf(x, y); }
__host__ __device__ __forceinline__ double svd_max(double x, double y) { return __builtin_fmax(x, y); }
__host__ __device__ __forceinline__ float svd_sqrt(float x) { return __builtin_sqrtf(x); }
__host__ __device__ __forceinline__ double svd_sqrt(double x) { return __builtin_sqrt(x); }
// 2^-e for the e of x = f 2^e, 0.5 <= |f| < 1 (1 for zero, inf and NaN), kept a normal number of T
__host__ __device__ __forceinline__ float svd_unit(float x, int emax)
{
    int e = 0;
    (void)__builtin_frexpf(x, &e);
    if (!(svd_abs(x) <= 3.0e38f) || x == 0.0f) e = 0;
    e = e > emax ? emax : (e < -emax ? -emax : e);
    return __builtin_ldexpf(1.0f, -e);
}
__host__ __device__ __forceinline__ double svd_unit(double x, int emax)
{
    int e = 0;
    (void)__builtin_frexp(x, &e);
    if (!(svd_abs(x) <= 1.0e308) || x == 0.0) e = 0;
    e = e > emax ? emax : (e < -emax ? -emax : e);
    return __builtin_ldexp(1.0, -e);
}

// did any lane of the wavefront rotate?  (the host runs one record at a time)
__host__ __device__ __forceinline__ bool svd_any(bool rotated)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __any(rotated) != 0;
#else
    return rotated;
#endif
}

// X = A^+ B.  Rows p < q of [A | C] (C starts as B) are rotated until the rows of A are mutually orthogonal: then
// |a_i| = sigma_i, C = U^T B, and X = sum_i a_i^T C_i / sigma_i^2 (V Sigma^-1 U^T B; neither U nor V is stored).
//  * Every record is first scaled by a power of two to max |a| in [0.5, 1) (exact; the result is scaled back), so
//    that no square of a row norm leaves the range of T.
//  * A pair is rotated when gamma^2 > tol^2 alpha beta (alpha, beta the squared norms, gamma the inner product),
//    tol = 2 sqrt(N) eps, and neither row is numerically null: squared norm <= (max(M, N) eps)^2 |A|_F^2.  Without
//    the guard the M - N (or N - rank) null rows of a record rotate rounding noise until the cap.  Every
//    comparison that enables a rotation is false for NaN: such a record leaves the loop after one sweep.
//  * The sweep loop leaves when no lane of the wavefront rotated, or at kSvdMaxSweeps.  A record that has
//    converged is not touched by the sweeps its neighbours still need: its result does not depend on them.
//  * pinv == false ('svd'): every row counts; a zero sigma gives inf / NaN for this record (the reference divides
//    by s the same way).  pinv == true: rows with sigma^2 <= rcond^2 sigma_max^2 are dropped, and for M > N the
//    null rows are (the reference's factorisation has only N singular values there).
// Returns the number of sweeps made (the last one finds nothing to rotate, unless the cap is hit).
template <typename T, int M, int N, int K>
__host__ __device__ __forceinline__ int svd_solve_rec(T (&a)[M][N], T (&c)[M][K], T (&x)[N][K], bool pinv, T rc2)
{
    constexpr T eps = SvdEps<T>::eps;
    constexpr T tol2 = T(4 * N) * eps * eps;
    constexpr int MX = M > N ? M : N;
    constexpr T null_rel = T(MX * MX) * eps * eps;
    T amax = T(0);
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) amax = svd_max(amax, svd_abs(a[i][j]));
    const T scale = svd_unit(amax, SvdEps<T>::emax);
    T fro = T(0);
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            a[i][j] *= scale;
            fro += a[i][j] * a[i][j];
        }
    const T null2 = null_rel * fro;

    int sweeps = 0;
    if constexpr (M > 1) {
        for (; sweeps < kSvdMaxSweeps;) {
            bool rotated = false;
#pragma unroll
            for (int p = 0; p < M - 1; ++p) {
#pragma unroll
                for (int q = p + 1; q < M; ++q) {
                    T alpha = T(0), beta = T(0), gamma = T(0);
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        alpha += a[p][j] * a[p][j];
                        beta += a[q][j] * a[q][j];
                        gamma += a[p][j] * a[q][j];
                    }
                    const bool go = gamma * gamma > tol2 * alpha * beta && alpha > null2 && beta > null2;
                    if (go) {
                        const T zeta = (beta - alpha) / (T(2) * gamma);
                        T t = T(1) / (svd_abs(zeta) + svd_sqrt(T(1) + zeta * zeta));
                        t = zeta < T(0) ? -t : t;
                        const T cs = T(1) / svd_sqrt(T(1) + t * t);
                        const T sn = cs * t;
#pragma unroll
                        for (int j = 0; j < N; ++j) {
                            const T u = a[p][j], v = a[q][j];
                            a[p][j] = cs * u - sn * v;
                            a[q][j] = sn * u + cs * v;
                        }
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const T u = c[p][k], v = c[q][k];
                            c[p][k] = cs * u - sn * v;
                            c[q][k] = sn * u + cs * v;
                        }
                        rotated = true;
                    }
                }
            }
            ++sweeps;
            if (!svd_any(rotated)) break;
        }
    }

    T s2[M];
    T s2max = T(0);
#pragma unroll
    for (int i = 0; i < M; ++i) {
        T alpha = T(0);
#pragma unroll
        for (int j = 0; j < N; ++j) alpha += a[i][j] * a[i][j];
        s2[i] = alpha;
        s2max = svd_max(s2max, alpha);
    }
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) x[j][k] = T(0);
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const bool drop = pinv && (s2[i] <= rc2 * s2max || (M > N && s2[i] <= null2));
        const T w = T(1) / s2[i];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T ck = drop ? T(0) : w * c[i][k];
#pragma unroll
            for (int j = 0; j < N; ++j) x[j][k] += a[i][j] * ck;
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) x[j][k] *= scale;
    return sweeps;
}

// the records as the kernel frame and the host loop hand them over: row-major A (M x N), B (M x K) or the M x M
// identity (IDENT), X (N x K)
template <typename T, int M, int N, int K, bool IDENT>
__host__ __device__ __forceinline__ int svd_solve_flat(const T *a, const T *b, T *r, const SvdParams &prm)
{
    T f[M][N], c[M][K], x[N][K];
#pragma unroll
    for (int i = 0; i < M; ++i) {
#pragma unroll
        for (int j = 0; j < N; ++j) f[i][j] = a[i * N + j];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if constexpr (IDENT) c[i][k] = i == k ? T(1) : T(0);
            else c[i][k] = b[i * K + k];
        }
    }
    const int sweeps = svd_solve_rec<T, M, N, K>(f, c, x, prm.pinv != 0, T(prm.rcond * prm.rcond));
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) r[j * K + k] = x[j][k];
    return sweeps;
}

template <typename T, int M, int N, int K>
struct SvdSolveOp {
    using RA = Rec<M, N>;
    using RB = Rec<M, K>;
    using RC = NoRec;
    using RO = Rec<N, K>;
    using Params = SvdParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RO::C) * (int)sizeof(T) + 48);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&b)[RB::Cs], const T (&)[1],
                                                 T (&r)[RO::Cs], const Params &prm)
    {
        svd_solve_flat<T, M, N, K, false>(a, b, r, prm);
    }
};

// the same against the M x M identity, generated in registers (`inv`, sugar.py:240-256): no B operand, N x M result
template <typename T, int M, int N>
struct SvdInvOp {
    using RA = Rec<M, N>;
    using RB = NoRec;
    using RC = NoRec;
    using RO = Rec<N, M>;
    using Params = SvdParams;
    static constexpr int TILE = pick_tile((RA::C + RO::C) * (int)sizeof(T) + 32);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&)[1], const T (&)[1],
                                                 T (&r)[RO::Cs], const Params &prm)
    {
        svd_solve_flat<T, M, N, M, true>(a, nullptr, r, prm);
    }
};

} // namespace nfm
