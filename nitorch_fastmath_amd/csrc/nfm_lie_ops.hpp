// nfm_lie_ops.hpp -- per-lane matrix exponential and its first / second Frechet derivatives
// (the `Op` structs plugged into rec_kernel; used by nfm_lie.hip).
//
// Scaling and squaring around the reference's Taylor series (`_impl/expm.py:139-190`), per matrix
// (DESIGN.md section 2, quirks Q17 / Q18):
//   s  = min(max(e, 0), kLieMaxSquarings) with ||X||_1 = f 2^e, f in [0.5, 1)  ->  ||X||_1 / 2^s <= 1
//   Y  = X / 2^s (exact)
//   m  = the first n >= 2 with (||Y||_F^n / n!)^2 <= D^2 tol, or max_order: since ||T_n||_F <= ||Y||_F^n / n!
//        for the reference's terms T_n = T_{n-1} Y / n, its own stop test (sum(T_n^2) <= D^2 tol) holds at n = m
//   E  = sum_{n <= m} Y^n / n!, evaluated by Horner: P <- I + Y P / k, k = m .. 1
//   then E <- E E, s times.  A matrix with a non-finite entry gives NaN everywhere.
// Horner multiplies by Y from the left, so column j of the next P needs column j of this one only:
// every step runs column by column in place (2 D^2 + D live values; the term-by-term recurrence needs
// 3 D^2 and did not fit float32 8x8 without scratch).  The derivatives differentiate the same steps:
//   P^A <- (A' P + Y P^A) / k,   H <- (A' P^B + B' P^A + Y H) / k        A' = A / 2^s, B' = B / 2^s
// and the squarings:  L <- L E + E L,  H <- H E + L^A L^B + L^B L^A + E H.
// The derivatives run to degree min(m + DEPTH, max_order): their terms lag the exponential's by DEPTH powers of Y.
#pragma once
#include "nfm_record_kernel.hpp"

namespace nfm {

struct LieParams {
    int max_order;
    int unused;
    double tol;
};

// ||X||_1 / 2^s <= theta with theta = 1; s never exceeds this bound, so inf-free huge
// input still ends after at most 64 squarings (its result overflows, as it would anyway).
constexpr int kLieMaxSquarings = 64;

template <typename T, int D>
__device__ __forceinline__ void lie_mm(const T (&a)[D * D], const T (&b)[D * D], T (&c)[D * D])
{
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            T s = a[i * D] * b[j];
#pragma unroll
            for (int k = 1; k < D; ++k) s = fma(a[i * D + k], b[k * D + j], s);
            c[i * D + j] = s;
        }
}

// c = a b + d e
template <typename T, int D>
__device__ __forceinline__ void lie_mm2(const T (&a)[D * D], const T (&b)[D * D], const T (&d)[D * D],
                                        const T (&e)[D * D], T (&c)[D * D])
{
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            T s = a[i * D] * b[j];
#pragma unroll
            for (int k = 1; k < D; ++k) s = fma(a[i * D + k], b[k * D + j], s);
#pragma unroll
            for (int k = 0; k < D; ++k) s = fma(d[i * D + k], e[k * D + j], s);
            c[i * D + j] = s;
        }
}

// keeps the scheduler from interleaving the columns of a Horner step (their partial sums would be
// live together)
__device__ __forceinline__ void lie_fence() { __builtin_amdgcn_sched_barrier(0); }

// column j of a b, accumulated onto acc (acc += a b[:, j])
template <typename T, int D>
__device__ __forceinline__ void lie_col(const T (&a)[D * D], const T (&b)[D * D], int j, T (&acc)[D])
{
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int k = 0; k < D; ++k) acc[i] = fma(a[i * D + k], b[k * D + j], acc[i]);
}

// Scale X by 2^-s (s from the exponent of ||X||_1, Q17) into y; a non-finite entry makes y all NaN and s 0 (Q18).
template <typename T, int D>
__device__ __forceinline__ int lie_scale(const T (&x)[D * D], T (&y)[D * D])
{
    bool finite = true;
    T nrm = T(0);
#pragma unroll
    for (int j = 0; j < D; ++j) {
        T c = T(0);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            c += fabs(x[i * D + j]);
            finite = finite && __builtin_isfinite(x[i * D + j]);
        }
        nrm = c > nrm ? c : nrm;
    }
    int e = 0;
    (void)frexp(nrm, &e); // nrm = f 2^e, f in [0.5, 1)  ->  nrm <= 2^e
    int s = e > 0 ? e : 0;
    s = s < kLieMaxSquarings ? s : kLieMaxSquarings;
    if (!__builtin_isfinite(nrm)) s = kLieMaxSquarings; // finite entries whose column sum overflows
    s = finite ? s : 0;
    const T f = ldexp(T(1), -s);
    const T nan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < D * D; ++k) y[k] = finite ? x[k] * f : nan;
    return s;
}

// Degree m of the series (Q17): the first n >= 2 whose term bound (||Y||_F^n / n!)^2 is <= D^2 tol, at most
// max_order; a bound that overflows (only after the clamp of s, the result overflows too) or is NaN ends it.
template <typename T, int D>
__device__ __forceinline__ int lie_degree(const T (&y)[D * D], const LieParams &p)
{
    T ss = T(0);
#pragma unroll
    for (int k = 0; k < D * D; ++k) ss = fma(y[k], y[k], ss);
    const double b = sqrt(double(ss)), lim = double(D * D) * p.tol;
    double term = b;
    int m = 1;
#pragma unroll 1
    for (int n = 2; n <= p.max_order; ++n) {
        term = term * b / n;
        m = n;
        if (!(term * term > lim) || !(term < __builtin_huge_val())) break;
    }
    return m;
}

template <typename T, int D>
struct ExpmOp {
    using RA = Rec<D, D>;
    using RB = NoRec;
    using RC = NoRec;
    using RO = Rec<D, D>;
    using Params = LieParams;
    static constexpr int TILE = pick_tile(RA::C * (int)sizeof(T) + 16);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&)[1], const T (&)[1],
                                                 T (&r)[RO::Cs], const Params &p)
    {
        if constexpr (D == 1) {
            r[0] = __builtin_isfinite(a[0]) ? T(exp(a[0])) : T(__builtin_nan(""));
        } else {
            T y[D * D];
            const int s = lie_scale<T, D>(a, y);
            const int m = lie_degree<T, D>(y, p);
            T e[D * D];
#pragma unroll
            for (int k = 0; k < D * D; ++k) e[k] = (k % (D + 1) == 0) ? T(1) : T(0);
#pragma unroll 1
            for (int k = m; k >= 1; --k) {
                const T rk = T(1) / T(k);
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    T u[D] = {};
                    lie_col<T, D>(y, e, j, u);
#pragma unroll
                    for (int i = 0; i < D; ++i) e[i * D + j] = fma(u[i], rk, T(i == j ? 1 : 0));
                    lie_fence();
                }
            }
#pragma unroll 1
            for (int q = 0; q < s; ++q) {
                T u[D * D];
                lie_mm<T, D>(e, e, u);
#pragma unroll
                for (int k = 0; k < D * D; ++k) e[k] = u[k];
            }
#pragma unroll
            for (int k = 0; k < D * D; ++k) r[k] = e[k];
        }
    }
};

// DEPTH 1: L(X, A) (inputs X, A);  DEPTH 2: L2(X, A, B) (inputs X, A, B), symmetric in A and B.
// A non-finite entry in X, A or B gives NaN everywhere.
template <typename T, int D, int DEPTH>
struct ExpmFrechetOp {
    using RA = Rec<D, D>;
    using RB = Rec<D, D>;
    using RC = typename std::conditional<DEPTH == 2, Rec<D, D>, NoRec>::type;
    using RO = Rec<D, D>;
    using Params = LieParams;
    static constexpr int TILE = pick_tile((DEPTH + 1) * RA::C * (int)sizeof(T) + 16);
    static __device__ __forceinline__ void apply(const T (&x)[RA::Cs], const T (&a)[RB::Cs], const T (&b)[RC::Cs],
                                                 T (&r)[RO::Cs], const Params &p)
    {
        if constexpr (D == 1) {
            // d exp(x) = exp(x) a,  d2 exp(x) = exp(x) a b
            bool fin = __builtin_isfinite(x[0]) && __builtin_isfinite(a[0]);
            if constexpr (DEPTH == 2) fin = fin && __builtin_isfinite(b[0]);
            const T ex = fin ? T(exp(x[0])) : T(__builtin_nan(""));
            if constexpr (DEPTH == 1) r[0] = ex * a[0];
            else r[0] = ex * a[0] * b[0];
        } else {
            T y[D * D], ap[D * D];
            const int s = lie_scale<T, D>(x, y);
            // a non-finite entry in a direction gives NaN everywhere too, like one in X (Q18): an inf would
            // otherwise survive as inf in some entries and as NaN in others
            bool dfin = true;
#pragma unroll
            for (int k = 0; k < D * D; ++k) {
                dfin = dfin && __builtin_isfinite(a[k]);
                if constexpr (DEPTH == 2) dfin = dfin && __builtin_isfinite(b[k]);
            }
#pragma unroll
            for (int k = 0; k < D * D; ++k) y[k] = dfin ? y[k] : T(__builtin_nan(""));
            // Term n of the derivative's series is n!/(n - DEPTH)! products of n - DEPTH factors Y over n!: of size
            // ||Y||^(n - DEPTH) / (n - DEPTH)! per unit direction.  It passes the stop test DEPTH degrees after the
            // exponential's own term does (at ||X||_1 = 1e-3 the float64 L2 was 1e-13 off without this).
            int m = lie_degree<T, D>(y, p);
            const long long md = (long long)m + DEPTH;
            m = md <= (long long)p.max_order ? (int)md : (p.max_order > m ? p.max_order : m);
            const T f = ldexp(T(1), -s);
            T e[D * D], la[D * D];
#pragma unroll
            for (int k = 0; k < D * D; ++k) {
                ap[k] = a[k] * f;
                e[k] = (k % (D + 1) == 0) ? T(1) : T(0);
                la[k] = T(0);
            }
            [[maybe_unused]] T bp[D * D], lb[D * D], h[D * D];
            if constexpr (DEPTH == 2) {
#pragma unroll
                for (int k = 0; k < D * D; ++k) {
                    bp[k] = b[k] * f;
                    lb[k] = T(0);
                    h[k] = T(0);
                }
            }
#pragma unroll 1
            for (int k = m; k >= 1; --k) {
                const T rk = T(1) / T(k);
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    T ue[D] = {}, ua[D] = {};
                    lie_col<T, D>(ap, e, j, ua);
                    lie_col<T, D>(y, la, j, ua);
                    [[maybe_unused]] T ub[D] = {}, uh[D] = {};
                    if constexpr (DEPTH == 2) {
                        lie_col<T, D>(ap, lb, j, uh);
                        lie_col<T, D>(bp, la, j, uh);
                        lie_col<T, D>(y, h, j, uh);
                        lie_col<T, D>(bp, e, j, ub);
                        lie_col<T, D>(y, lb, j, ub);
                    }
                    lie_col<T, D>(y, e, j, ue);
#pragma unroll
                    for (int i = 0; i < D; ++i) {
                        const int q = i * D + j;
                        if constexpr (DEPTH == 2) {
                            h[q] = uh[i] * rk;
                            lb[q] = ub[i] * rk;
                        }
                        la[q] = ua[i] * rk;
                        e[q] = fma(ue[i], rk, T(i == j ? 1 : 0));
                    }
                    lie_fence();
                }
            }
#pragma unroll 1
            for (int q = 0; q < s; ++q) {
                T u[D * D];
                if constexpr (DEPTH == 2) {
                    T v[D * D];
                    lie_mm2<T, D>(h, e, la, lb, u);
                    lie_mm2<T, D>(lb, la, e, h, v);
#pragma unroll
                    for (int k = 0; k < D * D; ++k) h[k] = u[k] + v[k];
                    lie_mm2<T, D>(lb, e, e, lb, u);
#pragma unroll
                    for (int k = 0; k < D * D; ++k) lb[k] = u[k];
                }
                lie_mm2<T, D>(la, e, e, la, u);
#pragma unroll
                for (int k = 0; k < D * D; ++k) la[k] = u[k];
                lie_mm<T, D>(e, e, u);
#pragma unroll
                for (int k = 0; k < D * D; ++k) e[k] = u[k];
            }
#pragma unroll
            for (int k = 0; k < D * D; ++k) r[k] = DEPTH == 2 ? h[k] : la[k];
        }
    }
};

} // namespace nfm
