// nfm_polar_ops.hpp -- per-lane singular value decomposition A = U diag(S) Vh and polar decomposition A = R P of one
// small square matrix (the `Op` structs of nfm_polar.hip: `batchsvdvals`, `batchsvd`, `batchpolar` and the gradient of
// `batchpolar`; an extension of `batched`, no counterpart in the reference).  The sweeps are those of svd_solve_rec
// (nfm_svd_ops.hpp: one-sided Jacobi on the rows, power-of-two prescale, relative rotation test, null guard, bounded
// sweep loop), run on the rows of [A | I]: at convergence the rows of A are sigma_i v_i^T and the accumulated block
// is U^T.  The record routines are __host__ __device__: nfm_polar_host runs the same source on the CPU.
// The translation units that include this file are compiled with -ffp-contract=off: the kernels of the layout kinds
// inline the same routine and must give the same bits, so every fused multiply-add is written out here.
#pragma once
#include "nfm_svd_ops.hpp"

namespace nfm {
namespace polar {

// which gradients nfm_batch_polar_backward was given (an absent one counts as zeros; its operand is then a second
// view of A, which the kernel does not look at)
struct BwdParams {
    int has_gr, has_gp;
};
struct NoParams {
    int unused;
};

__host__ __device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__host__ __device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <typename T>
__host__ __device__ __forceinline__ T nan_t()
{
    return T(__builtin_nanf(""));
}

// The sweeps of svd_solve_rec on the rows of [A | W] (W: N x K, K == N accumulates U^T from the identity, K == 0
// for the values alone).  On return A is scaled by `scale` (a power of two), its rows are mutually orthogonal,
// null2 is the squared norm at or below which a row counts as numerically null, and `bad` says that the record had
// an entry that is not finite: it was then replaced by the identity (no sweep runs on it) and the caller writes NaN.
template <typename T, int N, int K>
__host__ __device__ __forceinline__ int jacobi_rows(T (&a)[N][N], T (&w)[N][K > 0 ? K : 1], T &scale, T &null2,
                                                    bool &bad)
{
    constexpr T eps = SvdEps<T>::eps;
    constexpr T tol2 = T(4 * N) * eps * eps;
    constexpr T null_rel = T(N * N) * eps * eps;
    T amax = T(0), chk = T(0);
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            amax = svd_max(amax, svd_abs(a[i][j]));
            chk = fma_t(a[i][j], T(0), chk); // NaN for inf and NaN
        }
    bad = !(chk == T(0));
    amax = bad ? T(1) : amax;
    scale = svd_unit(amax, SvdEps<T>::emax);
    T fro = T(0);
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            a[i][j] = bad ? T(i == j) : a[i][j] * scale;
            fro = fma_t(a[i][j], a[i][j], fro);
        }
    null2 = null_rel * fro;

    int sweeps = 0;
    if constexpr (N > 1) {
        for (; sweeps < kSvdMaxSweeps;) {
            bool rotated = false;
#pragma unroll
            for (int p = 0; p < N - 1; ++p) {
#pragma unroll
                for (int q = p + 1; q < N; ++q) {
                    T alpha = T(0), beta = T(0), gamma = T(0);
#pragma unroll
                    for (int j = 0; j < N; ++j) {
                        alpha = fma_t(a[p][j], a[p][j], alpha);
                        beta = fma_t(a[q][j], a[q][j], beta);
                        gamma = fma_t(a[p][j], a[q][j], gamma);
                    }
                    const bool go = gamma * gamma > tol2 * alpha * beta && alpha > null2 && beta > null2;
                    if (go) {
                        const T zeta = (beta - alpha) / (T(2) * gamma);
                        T t = T(1) / (svd_abs(zeta) + svd_sqrt(fma_t(zeta, zeta, T(1))));
                        t = zeta < T(0) ? -t : t;
                        const T cs = T(1) / svd_sqrt(fma_t(t, t, T(1)));
                        const T sn = cs * t;
#pragma unroll
                        for (int j = 0; j < N; ++j) {
                            const T u = a[p][j], v = a[q][j];
                            a[p][j] = fma_t(cs, u, -(sn * v));
                            a[q][j] = fma_t(sn, u, cs * v);
                        }
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const T u = w[p][k], v = w[q][k];
                            w[p][k] = fma_t(cs, u, -(sn * v));
                            w[q][k] = fma_t(sn, u, cs * v);
                        }
                        rotated = true;
                    }
                }
            }
            ++sweeps;
            if (!svd_any(rotated)) break;
        }
    }
    return sweeps;
}

template <typename T>
__host__ __device__ __forceinline__ void cswap(bool sw, T &x, T &y)
{
    const T u = x, v = y;
    x = sw ? v : u;
    y = sw ? u : v;
}

// squared row norms, then a compare-exchange network (bubble order, N (N - 1) / 2 exchanges) that puts them in
// descending order; whole rows of A and W move with them under the same predicate (no run-time register index)
template <typename T, int N, int K>
__host__ __device__ __forceinline__ void sort_rows(T (&a)[N][N], T (&w)[N][K > 0 ? K : 1], T (&s2)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T alpha = T(0);
#pragma unroll
        for (int j = 0; j < N; ++j) alpha = fma_t(a[i][j], a[i][j], alpha);
        s2[i] = alpha;
    }
#pragma unroll
    for (int r = 0; r < N - 1; ++r) {
#pragma unroll
        for (int i = 0; i < N - 1 - r; ++i) {
            const bool sw = s2[i] < s2[i + 1];
            cswap(sw, s2[i], s2[i + 1]);
            if constexpr (K > 0) {
#pragma unroll
                for (int j = 0; j < N; ++j) cswap(sw, a[i][j], a[i + 1][j]);
#pragma unroll
                for (int k = 0; k < K; ++k) cswap(sw, w[i][k], w[i + 1][k]);
            }
        }
    }
}

// The decomposition of one record: on return the rows of `a` are the v_i^T (Vh), the rows of `w` the u_i^T (U^T),
// sig[i] the singular values of the SCALED record in descending order (sigma_i = sig[i] / scale), nul[i] says that
// row i was numerically null.  The rows the guard classes as null carry rounding noise, not a singular vector: they
// are replaced by an orthonormal completion of the rows before them -- the coordinate vector with the largest
// residual, orthogonalised twice (modified Gram-Schmidt) and normalised; the residual is at least 1 / N, so the
// normalisation is safe.  After the sort a null row has only null rows after it, so row i is completed against the
// rows 0..i-1.  Only lanes with a null row take the branch.  W is a product of rotations: orthogonal for every record.
template <typename T, int N>
__host__ __device__ __forceinline__ int decompose(T (&a)[N][N], T (&w)[N][N], T (&sig)[N], bool (&nul)[N], T &scale,
                                                  bool &bad)
{
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) w[i][j] = T(i == j);
    T null2;
    const int sweeps = jacobi_rows<T, N, N>(a, w, scale, null2, bad);
    T s2[N];
    sort_rows<T, N, N>(a, w, s2);
    bool any_null = false;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        nul[i] = !(s2[i] > null2);
        any_null |= nul[i];
        sig[i] = svd_sqrt(s2[i]);
        const T rinv = nul[i] ? T(0) : T(1) / sig[i];
#pragma unroll
        for (int j = 0; j < N; ++j) a[i][j] *= rinv;
    }
    if (any_null) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (nul[i]) {
                T e[N];
                T best = T(-1);
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    T r = T(1);
#pragma unroll
                    for (int j = 0; j < i; ++j) r = fma_t(-a[j][k], a[j][k], r);
                    e[k] = r;
                    best = svd_max(best, r);
                }
                bool taken = false;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const bool hit = !taken && e[k] == best;
                    e[k] = hit ? T(1) : T(0);
                    taken |= hit;
                }
#pragma unroll
                for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
                    for (int j = 0; j < i; ++j) {
                        T d = T(0);
#pragma unroll
                        for (int k = 0; k < N; ++k) d = fma_t(e[k], a[j][k], d);
#pragma unroll
                        for (int k = 0; k < N; ++k) e[k] = fma_t(-d, a[j][k], e[k]);
                    }
                }
                T nn = T(0);
#pragma unroll
                for (int k = 0; k < N; ++k) nn = fma_t(e[k], e[k], nn);
                const T rn = T(1) / svd_sqrt(nn);
#pragma unroll
                for (int k = 0; k < N; ++k) a[i][k] = e[k] * rn;
            }
        }
    }
    return sweeps;
}

// ---- the records as the kernel frame and the host loop hand them over (row-major)

// S (N), descending
template <typename T, int N>
__host__ __device__ __forceinline__ int vals_flat(const T *ar, T *r)
{
    T a[N][N], w[N][1], s2[N], scale, null2;
    bool bad;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) a[i][j] = ar[i * N + j];
    const int sweeps = jacobi_rows<T, N, 0>(a, w, scale, null2, bad);
    sort_rows<T, N, 0>(a, w, s2);
    const T inv = T(1) / scale;
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = bad ? nan_t<T>() : svd_sqrt(s2[i]) * inv;
    return sweeps;
}

// [S (N) | U (N x N) | Vh (N x N)]
template <typename T, int N>
__host__ __device__ __forceinline__ int full_flat(const T *ar, T *r)
{
    T a[N][N], w[N][N], sig[N], scale;
    bool nul[N], bad;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) a[i][j] = ar[i * N + j];
    const int sweeps = decompose<T, N>(a, w, sig, nul, scale, bad);
    const T inv = T(1) / scale;
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = bad ? nan_t<T>() : sig[i] * inv;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            r[N + i * N + j] = bad ? nan_t<T>() : w[j][i];
            r[N + N * N + i * N + j] = bad ? nan_t<T>() : a[i][j];
        }
    return sweeps;
}

// [R (N x N) | P (N x N)]: R = sum_i u_i v_i^T, P = sum_i sigma_i v_i v_i^T (upper triangle, mirrored)
template <typename T, int N>
__host__ __device__ __forceinline__ int polar_flat(const T *ar, T *r)
{
    T a[N][N], w[N][N], sig[N], scale;
    bool nul[N], bad;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) a[i][j] = ar[i * N + j];
    const int sweeps = decompose<T, N>(a, w, sig, nul, scale, bad);
    const T inv = T(1) / scale;
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int k = 0; k < N; ++k) {
            T s = w[0][j] * a[0][k];
#pragma unroll
            for (int i = 1; i < N; ++i) s = fma_t(w[i][j], a[i][k], s);
            r[j * N + k] = bad ? nan_t<T>() : s;
        }
#pragma unroll
    for (int i = 0; i < N; ++i) sig[i] *= inv;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        T t[N];
#pragma unroll
        for (int i = 0; i < N; ++i) t[i] = sig[i] * a[i][j];
#pragma unroll
        for (int k = j; k < N; ++k) {
            T s = t[0] * a[0][k];
#pragma unroll
            for (int i = 1; i < N; ++i) s = fma_t(t[i], a[i][k], s);
            s = bad ? nan_t<T>() : s;
            r[N * N + j * N + k] = s;
            r[N * N + k * N + j] = s;
        }
    }
    return sweeps;
}

// gradient of (R, P) = polar(A) given the cotangents gr of R and gp of P:  with B = U^T gr V and
// C = V^T sym(gp) V,  X_ij = ((B - B^T)_ij + 2 sigma_i C_ij) / (sigma_i + sigma_j)  and the result is U X V^T.
// The denominators are sums: regular at repeated and clustered singular values.  Two null rows i != j (rank <= N - 2,
// where R is not differentiable): 2 sigma_i / (sigma_i + sigma_j) is taken as 1, and the record is NaN when any entry
// of gr is not zero.
template <typename T, int N>
__host__ __device__ __forceinline__ int polar_bwd_flat(const T *ar, const T *gr, const T *gp, T *r, const BwdParams &q)
{
    const bool has_gr = q.has_gr != 0, has_gp = q.has_gp != 0;
    // what has to wait for the decomposition: gr (N^2 values, B is later built in their place) and the upper
    // triangle of sym(gp)
    T x[N][N], sg[N * (N + 1) / 2];
    bool gr_nonzero = false;
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int l = 0; l < N; ++l) {
            x[k][l] = has_gr ? gr[k * N + l] : T(0);
            gr_nonzero |= !(x[k][l] == T(0));
            if (l >= k) sg[k * N - k * (k - 1) / 2 + l - k] = has_gp ? T(0.5) * (gp[k * N + l] + gp[l * N + k]) : T(0);
        }
    T a[N][N], w[N][N], sig[N], scale;
    bool nul[N], bad;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) a[i][j] = ar[i * N + j];
    const int sweeps = decompose<T, N>(a, w, sig, nul, scale, bad);
    int nnull = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) nnull += nul[i] ? 1 : 0;
    bad |= nnull >= 2 && gr_nonzero;
    // C = V^T sym(gp) V (rows of a are the v_i): Z = sym(gp) V row by row, then C = Vh Z column by column in place
    T c[N][N];
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            T s = T(0);
#pragma unroll
            for (int l = 0; l < N; ++l) {
                const int lo = k < l ? k : l, hi = k < l ? l : k;
                s = fma_t(sg[lo * N - lo * (lo - 1) / 2 + hi - lo], a[j][l], s);
            }
            c[k][j] = s;
        }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        T t[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            T s = T(0);
#pragma unroll
            for (int k = 0; k < N; ++k) s = fma_t(a[i][k], c[k][j], s);
            t[i] = s;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) c[i][j] = t[i];
    }
    // B = U^T gr V in the place of gr: Y = gr V row by row, then B = W Y column by column
#pragma unroll
    for (int k = 0; k < N; ++k) {
        T t[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            T s = T(0);
#pragma unroll
            for (int l = 0; l < N; ++l) s = fma_t(x[k][l], a[j][l], s);
            t[j] = s;
        }
#pragma unroll
        for (int j = 0; j < N; ++j) x[k][j] = t[j];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        T t[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            T s = T(0);
#pragma unroll
            for (int k = 0; k < N; ++k) s = fma_t(w[i][k], x[k][j], s);
            t[i] = s;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) x[i][j] = t[i];
    }
    // X (scaled singular values: 1 / (sigma_i + sigma_j) = scale / (sig_i + sig_j), the ratios are scale-free)
#pragma unroll
    for (int i = 0; i < N; ++i) {
        x[i][i] = c[i][i];
#pragma unroll
        for (int j = i + 1; j < N; ++j) {
            const bool both = nul[i] && nul[j];
            const T den = both ? T(0) : T(1) / (sig[i] + sig[j]);
            const T sk = (x[i][j] - x[j][i]) * (scale * den);
            const T fi = both ? T(1) : T(2) * sig[i] * den, fj = both ? T(1) : T(2) * sig[j] * den;
            x[i][j] = fma_t(fi, c[i][j], sk);
            x[j][i] = fma_t(fj, c[j][i], -sk);
        }
    }
    // U X Vh in place: T = X Vh row by row, then W^T T column by column
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T t[N];
#pragma unroll
        for (int l = 0; l < N; ++l) {
            T s = T(0);
#pragma unroll
            for (int j = 0; j < N; ++j) s = fma_t(x[i][j], a[j][l], s);
            t[l] = s;
        }
#pragma unroll
        for (int l = 0; l < N; ++l) x[i][l] = t[l];
    }
#pragma unroll
    for (int l = 0; l < N; ++l)
#pragma unroll
        for (int k = 0; k < N; ++k) {
            T s = T(0);
#pragma unroll
            for (int i = 0; i < N; ++i) s = fma_t(w[i][k], x[i][l], s);
            r[k * N + l] = bad ? nan_t<T>() : s;
        }
    return sweeps;
}

} // namespace polar

// from these orders on the kernels are bound by their dependent arithmetic: no LDS image of the records (as EigSymOp)
template <typename T, int N>
constexpr bool polar_no_tile = N >= 5 || (N == 4 && sizeof(T) == 8);

template <typename T, int N>
struct SvdValsOp {
    using RA = Rec<N, N>;
    using RB = NoRec;
    using RC = NoRec;
    using RO = Rec<1, N>;
    using Params = polar::NoParams;
    static constexpr int TILE = pick_tile((RA::C + RO::C) * (int)sizeof(T) + 32);
    static constexpr bool kNoTile = polar_no_tile<T, N>;
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&)[1], const T (&)[1], T (&r)[RO::Cs],
                                                 const Params &)
    {
        polar::vals_flat<T, N>(a, r);
    }
};

template <typename T, int N>
struct SvdFullOp {
    using RA = Rec<N, N>;
    using RB = NoRec;
    using RC = NoRec;
    using RO = Rec<1, N + 2 * N * N>;
    using Params = polar::NoParams;
    static constexpr int TILE = pick_tile((RA::C + RO::C) * (int)sizeof(T) + 32);
    static constexpr bool kNoTile = polar_no_tile<T, N>;
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&)[1], const T (&)[1], T (&r)[RO::Cs],
                                                 const Params &)
    {
        polar::full_flat<T, N>(a, r);
    }
};

template <typename T, int N>
struct PolarOp {
    using RA = Rec<N, N>;
    using RB = NoRec;
    using RC = NoRec;
    using RO = Rec<1, 2 * N * N>;
    using Params = polar::NoParams;
    static constexpr int TILE = pick_tile((RA::C + RO::C) * (int)sizeof(T) + 32);
    static constexpr bool kNoTile = polar_no_tile<T, N>;
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&)[1], const T (&)[1], T (&r)[RO::Cs],
                                                 const Params &)
    {
        polar::polar_flat<T, N>(a, r);
    }
};

template <typename T, int N>
struct PolarBwdOp {
    using RA = Rec<N, N>; // A
    using RB = Rec<N, N>; // cotangent of R
    using RC = Rec<N, N>; // cotangent of P
    using RO = Rec<N, N>;
    using Params = polar::BwdParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RC::C + RO::C) * (int)sizeof(T) + 64);
    static constexpr bool kNoTile = polar_no_tile<T, N>;
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&gr)[RB::Cs], const T (&gp)[RC::Cs],
                                                 T (&r)[RO::Cs], const Params &q)
    {
        polar::polar_bwd_flat<T, N>(a, gr, gp, r, q);
    }
};

} // namespace nfm
