// nfm_sugar_ops.hpp -- per-lane solves of A X = B for a general or a positive definite N x N matrix and a matrix
// of K right-hand sides (the `Op` structs of nfm_sugar.hip: `lmdiv`, `rmdiv`, `solvevec`, `inv` of the reference's
// `sugar.py`; file:line citations are relative to the reference package).
#pragma once
#include "nfm_record_kernel.hpp"
#include "nfm_smallmat.hpp"

namespace nfm {

constexpr int kSugarMaxDim = 8;

// Largest number of right-hand sides one launch takes at order N: [A | B] is N (N + K) values per lane, and the
// staging registers of the LDS tiles come on top.  The one table of the column caps: the kernels above a cap are
// not compiled, nfm_sugar_solve answers NFM_ESIZE there, and the facade (which reads the cap through
// nfm_sugar_max_cols) splits B into blocks of columns.  Every entry is the largest K whose kernels, all kinds,
// have no private segment (tests/test_sugar_host.py holds the table to the code objects).
__host__ __device__ constexpr int sugar_max_k(bool f64, int N)
{
    return (f64 && N == 8) ? 6 : 8; // 8 x 8 float64: the run-time-mode LU kernel spills from K = 7
}

struct SugarParams {
    int unused;
};

__device__ __forceinline__ float sqrt_s(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double sqrt_s(double x) { return __builtin_sqrt(x); }

// X = A^-1 B by Gaussian elimination with partial pivoting on [A | B] (ge_solve: getrf / getrs, what
// `torch.linalg.solve` of `lmdiv(method='lu')` runs, sugar.py:125-126).  A singular record gives inf / NaN.
template <typename T, int N, int K>
struct SolveLuOp {
    using RA = Rec<N, N>;
    using RB = Rec<N, K>;
    using RC = NoRec;
    using RO = Rec<N, K>;
    using Params = SugarParams;
    static constexpr int TILE = pick_tile((RA::C + 2 * RB::C) * (int)sizeof(T) + 48);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&b)[RB::Cs], const T (&)[1],
                                                 T (&r)[RO::Cs], const Params &)
    {
        if constexpr (N == 1) {
#pragma unroll
            for (int c = 0; c < K; ++c) r[c] = b[c] / a[0];
        } else {
            T f[N][N], x[N][K];
#pragma unroll
            for (int i = 0; i < N; ++i) {
#pragma unroll
                for (int j = 0; j < N; ++j) f[i][j] = a[i * N + j];
#pragma unroll
                for (int c = 0; c < K; ++c) x[i][c] = b[i * K + c];
            }
            ge_solve<T, N, K>(f, x);
#pragma unroll
            for (int i = 0; i < N; ++i)
#pragma unroll
                for (int c = 0; c < K; ++c) r[i * K + c] = x[i][c];
        }
    }
};

// A = L L^T without pivoting from the LOWER triangle of the record (the upper one is never read, like
// `torch.linalg.cholesky(a, upper=False)`, sugar.py:128), then L y = b and L^T x = y for the K columns of x in
// place.  N (N + 1) / 2 live matrix values; the diagonal of L is kept as its reciprocal.  A pivot that is not
// positive (NaN included) makes every entry of the record's result NaN: the reference raises for the whole batch.
template <typename T, int N, int K>
__device__ __forceinline__ void chol_solve(const T (&a)[N * N], T (&x)[N][K])
{
    T l[N][N]; // j <= i only
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        T d = a[j * N + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= l[j][k] * l[j][k];
        ok = ok && (d > T(0));
        const T rd = T(1) / sqrt_s(d);
        l[j][j] = rd;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            T s = a[i * N + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= l[i][k] * l[j][k];
            l[i][j] = s * rd;
        }
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            T s = x[i][c];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= l[i][k] * x[k][c];
            x[i][c] = s * l[i][i];
        }
#pragma unroll
        for (int i = N - 1; i >= 0; --i) {
            T s = x[i][c];
#pragma unroll
            for (int k = i + 1; k < N; ++k) s -= l[k][i] * x[k][c];
            x[i][c] = s * l[i][i];
        }
    }
    if (!ok) {
        const T nan = __builtin_nanf("");
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int c = 0; c < K; ++c) x[i][c] = nan;
    }
}

template <typename T, int N, int K>
struct SolveCholOp {
    using RA = Rec<N, N>;
    using RB = Rec<N, K>;
    using RC = NoRec;
    using RO = Rec<N, K>;
    using Params = SugarParams;
    static constexpr int TILE = pick_tile((RA::C + 2 * RB::C) * (int)sizeof(T) + 48);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&b)[RB::Cs], const T (&)[1],
                                                 T (&r)[RO::Cs], const Params &)
    {
        T x[N][K];
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int c = 0; c < K; ++c) x[i][c] = b[i * K + c];
        chol_solve<T, N, K>(a, x);
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int c = 0; c < K; ++c) r[i * K + c] = x[i][c];
    }
};

// the same against the identity, generated in registers (`inv(method='chol')`, sugar.py:244-250): no B operand
template <typename T, int N>
struct CholInvOp {
    using RA = Rec<N, N>;
    using RB = NoRec;
    using RC = NoRec;
    using RO = Rec<N, N>;
    using Params = SugarParams;
    static constexpr int TILE = pick_tile(2 * RA::C * (int)sizeof(T) + 32);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&)[1], const T (&)[1],
                                                 T (&r)[RO::Cs], const Params &)
    {
        T x[N][N];
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int c = 0; c < N; ++c) x[i][c] = i == c ? T(1) : T(0);
        chol_solve<T, N, N>(a, x);
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int c = 0; c < N; ++c) r[i * N + c] = x[i][c];
    }
};

} // namespace nfm
