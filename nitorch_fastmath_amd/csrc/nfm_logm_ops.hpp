// nfm_logm_ops.hpp -- per-lane principal matrix logarithm and its Frechet derivative
// (the `Op` structs plugged into rec_kernel; used by nfm_logm.hip).
//
// Full-matrix inverse scaling and squaring (Cheng, Higham, Kenney and Laub 2001), no Schur form
// (DESIGN.md section 2, quirks Q20 / Q22):
//   s = 0
//   while ||A - I||_1 > kLogmTheta:                       square roots, per matrix
//       M = Y = A                                         product-form Denman-Beavers iteration
//       repeat:  Mi = inv(M);  Y <- Y (I + Mi) / 2;  M <- (I + (M + Mi) / 2) / 2
//       until ||M - I||_1 <= 4 D eps, or the M before the step had ||M - I||_1 <= sqrt(eps)
//             (the step squares that residual: e -> e^2 / 4, so the second form cannot stagnate on rounding)
//       A = Y;  s += 1
//   Z = (A - I) inv(A + I)                                log A = 2 atanh(Z)
//   m = the first k with ||Z||_1^(2k+1) / (2k+1) <= eps / 8
//   log = 2^(s+1) Z sum_{k <= m} (Z^2)^k / (2k+1)         Horner, column by column in place
// A matrix with a non-finite entry, a singular one, or one whose square-root iteration does not pass its
// stop test in kLogmMaxIter steps (eigenvalues on the closed negative real axis) gives NaN everywhere.
//
// The two loops are flattened into one per-lane loop of Denman-Beavers steps: a lane whose iteration has
// converged restarts it on its own Y in the same pass (selects, no branch around the inverse), so a wave
// runs the largest TOTAL step count of its lanes, not the sum of the per-root maxima.
//
// LogmCore<T, D, true> carries the derivative of every value along (A', M', Y', Z', ...): the same steps
// differentiated, with inv' = -Mi M' Mi.
// Its roots end on another test: at the second step in a row whose M before the step had
// ||M - I||_1 <= sqrt(eps).  M' lags M by a step, and where M - I is nilpotent (a unipotent A: a translation) M
// reaches I exactly while M' is of order one.
#pragma once
#include "nfm_record_kernel.hpp"
#include "nfm_smallmat.hpp"
#include "nfm_lie_ops.hpp"

namespace nfm {

// Every multiply-add below is an explicit fma and nothing else may fuse: the variants of rec_kernel inline the
// same body next to different load / store code, and a contraction left to the compiler (or to the packed
// float32 instructions its vectoriser picks) would make the result depend on the layout of the operands.
// The pragma opens every function body here (as det_closed in nfm_smallmat.hpp does), so that including this
// header changes nothing for the code after it.
#define NFM_LOGM_NO_CONTRACT _Pragma("clang fp contract(off)")

// In-place Gauss-Jordan inverse with partial pivoting (gj_inverse of nfm_smallmat.hpp, with explicit fma):
// row exchanges during the elimination, the matching column exchanges undone at the end.  Singular -> inf / NaN.
template <typename T, int N>
__device__ __forceinline__ void logm_inverse(T (&a)[N][N])
{
    NFM_LOGM_NO_CONTRACT
    int piv[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int p = k;
        T best = fabs_(a[k][k]);
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const T x = fabs_(a[i][k]);
            const bool g = x > best;
            best = g ? x : best;
            p = g ? i : p;
        }
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const bool sw = p == i;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const T t = a[k][j];
                a[k][j] = sw ? a[i][j] : t;
                a[i][j] = sw ? t : a[i][j];
            }
        }
        piv[k] = p;
        const T rp = T(1) / a[k][k];
        a[k][k] = T(1);
#pragma unroll
        for (int j = 0; j < N; ++j) a[k][j] *= rp;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (i != k) {
                const T f = -a[i][k];
                a[i][k] = T(0);
#pragma unroll
                for (int j = 0; j < N; ++j) a[i][j] = fma_(f, a[k][j], a[i][j]);
            }
        }
    }
#pragma unroll
    for (int k = N - 2; k >= 0; --k) {
#pragma unroll
        for (int c = k + 1; c < N; ++c) {
            const bool sw = piv[k] == c;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const T t = a[i][k];
                a[i][k] = sw ? a[i][c] : t;
                a[i][c] = sw ? t : a[i][c];
            }
        }
    }
}

// b <- a^-1 b by Gaussian elimination with partial pivoting on [a | b] (ge_solve of nfm_smallmat.hpp, with
// explicit fma)
template <typename T, int N>
__device__ __forceinline__ void logm_solve(T (&a)[N][N], T (&b)[N][N])
{
    NFM_LOGM_NO_CONTRACT
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int p = k;
        T best = fabs_(a[k][k]);
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const T x = fabs_(a[i][k]);
            const bool g = x > best;
            best = g ? x : best;
            p = g ? i : p;
        }
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const bool sw = p == i;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                if (j >= k) {
                    const T t = a[k][j];
                    a[k][j] = sw ? a[i][j] : t;
                    a[i][j] = sw ? t : a[i][j];
                }
                const T u = b[k][j];
                b[k][j] = sw ? b[i][j] : u;
                b[i][j] = sw ? u : b[i][j];
            }
        }
        const T rp = T(1) / a[k][k];
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const T l = -(a[i][k] * rp);
#pragma unroll
            for (int j = k + 1; j < N; ++j) a[i][j] = fma_(l, a[k][j], a[i][j]);
#pragma unroll
            for (int j = 0; j < N; ++j) b[i][j] = fma_(l, b[k][j], b[i][j]);
        }
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        const T rd = T(1) / a[i][i];
#pragma unroll
        for (int r = 0; r < N; ++r) {
            T s = b[i][r];
#pragma unroll
            for (int j = i + 1; j < N; ++j) s = fma_(-a[i][j], b[j][r], s);
            b[i][r] = s * rd;
        }
    }
}

struct LogmParams {}; // the ops take no run-time parameter

constexpr int kLogmMaxIter = 40;  // Denman-Beavers steps per square root (a root of norm 2^60 takes about 35)
constexpr int kLogmMaxRoots = 64; // square roots per matrix

template <typename T>
struct LogmEps;
template <>
struct LogmEps<float> {
    static constexpr float eps = 1.1920928955078125e-07f, sqrt_eps = 3.4526698300124393e-04f;
};
template <>
struct LogmEps<double> {
    static constexpr double eps = 2.220446049250313e-16, sqrt_eps = 1.4901161193847656e-08;
};

// ||a - I||_1
template <typename T, int D>
__device__ __forceinline__ T logm_dist1(const T (&a)[D][D])
{
    NFM_LOGM_NO_CONTRACT
    T nrm = T(0);
#pragma unroll
    for (int j = 0; j < D; ++j) {
        T c = T(0);
#pragma unroll
        for (int i = 0; i < D; ++i) c += fabs_(a[i][j] - T(i == j ? 1 : 0));
        nrm = fmax_(nrm, c); // (a NaN column is dropped here; the callers test finiteness on their own)
    }
    return nrm;
}

template <typename T, int D>
__device__ __forceinline__ bool logm_finite(const T (&a)[D][D])
{
    bool f = true;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) f = f && __builtin_isfinite(a[i][j]);
    return f;
}

// b <- a b, column by column in place
template <typename T, int D>
__device__ __forceinline__ void logm_lmul(const T (&a)[D][D], T (&b)[D][D])
{
    NFM_LOGM_NO_CONTRACT
#pragma unroll
    for (int j = 0; j < D; ++j) {
        T u[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            T s = a[i][0] * b[0][j];
#pragma unroll
            for (int k = 1; k < D; ++k) s = fma_(a[i][k], b[k][j], s);
            u[i] = s;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) b[i][j] = u[i];
        lie_fence();
    }
}

// a <- a b, row by row in place
template <typename T, int D>
__device__ __forceinline__ void logm_rmul(T (&a)[D][D], const T (&b)[D][D])
{
    NFM_LOGM_NO_CONTRACT
#pragma unroll
    for (int i = 0; i < D; ++i) {
        T u[D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            T s = a[i][0] * b[0][j];
#pragma unroll
            for (int k = 1; k < D; ++k) s = fma_(a[i][k], b[k][j], s);
            u[j] = s;
        }
#pragma unroll
        for (int j = 0; j < D; ++j) a[i][j] = u[j];
        lie_fence();
    }
}

// The whole algorithm on y (and its derivative yd when DUAL): y <- log y, yd <- L_log(y, yd).
template <typename T, int D, bool DUAL>
struct LogmCore {
    using Mat = T[D][D];
    static constexpr int DD = DUAL ? D : 1; // extent of the derivative matrices (unused ones collapse)
    using Dual = T[DD][DD];

    static __device__ __forceinline__ void run(Mat &y, Dual &yd)
    {
        NFM_LOGM_NO_CONTRACT
        using E = LogmEps<T>;
        [[maybe_unused]] const T tol_m = T(4 * D) * E::eps;
        const T theta = T(0.25);
        bool bad = !logm_finite<T, D>(y);
        if constexpr (DUAL) bad = bad || !logm_finite<T, D>(yd);
        bool done = bad || logm_dist1<T, D>(y) <= theta;
        int s = 0, it = 0;
        [[maybe_unused]] bool was_near = false; // the step before started within sqrt(eps) (this root)
        Mat m;
        [[maybe_unused]] Dual md;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                m[i][j] = y[i][j];
                if constexpr (DUAL) md[i][j] = yd[i][j];
            }
        // ---- square roots: one Denman-Beavers step per pass
#pragma unroll 1
        while (!done) {
            const T e_prev = logm_dist1<T, D>(m);
            Mat mi;
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) mi[i][j] = m[i][j];
            logm_inverse<T, D>(mi);
            lie_fence();
            if constexpr (DUAL) {
                // mid = -mi md mi, built in place on t = md mi
                Mat t;
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        T a = md[i][0] * mi[0][j];
#pragma unroll
                        for (int k = 1; k < D; ++k) a = fma_(md[i][k], mi[k][j], a);
                        t[i][j] = -a;
                    }
                logm_lmul<T, D>(mi, t);
                // yd <- (yd + yd mi + y mid) / 2 row by row (the old row of y), md <- (md + mid) / 4
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    T u[D];
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        T a = yd[i][j];
#pragma unroll
                        for (int k = 0; k < D; ++k) a = fma_(yd[i][k], mi[k][j], a);
#pragma unroll
                        for (int k = 0; k < D; ++k) a = fma_(y[i][k], t[k][j], a);
                        u[j] = T(0.5) * a;
                    }
#pragma unroll
                    for (int j = 0; j < D; ++j) yd[i][j] = u[j];
                    lie_fence();
                }
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) md[i][j] = T(0.25) * (md[i][j] + t[i][j]);
            }
            // y <- (y + y mi) / 2 row by row, m <- (I + (m + mi) / 2) / 2
#pragma unroll
            for (int i = 0; i < D; ++i) {
                T u[D];
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    T a = y[i][j];
#pragma unroll
                    for (int k = 0; k < D; ++k) a = fma_(y[i][k], mi[k][j], a);
                    u[j] = T(0.5) * a;
                }
#pragma unroll
                for (int j = 0; j < D; ++j) y[i][j] = u[j];
                lie_fence();
            }
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j)
                    m[i][j] = T(0.5) * (T(i == j ? 1 : 0) + T(0.5) * (m[i][j] + mi[i][j]));
            ++it;
            // With the derivative carried along, the root ends at the second step in a row that started within
            // sqrt(eps): m can reach I, even exactly, while md is still of order one (a unipotent matrix:
            // m - I is nilpotent and vanishes after a few steps), and y' needs the steps that consume that md.
            // A step from ||m - I|| = e leaves md of order e md: the first of the two makes e rounding-sized,
            // the second md.
            const bool near = e_prev <= E::sqrt_eps;
            const bool conv = DUAL ? near && was_near : logm_dist1<T, D>(m) <= tol_m || near;
            was_near = near;
            if (conv) {
                // this root is done: count it and start the next one on y (or leave)
                ++s;
                it = 0;
                was_near = false;
                done = logm_dist1<T, D>(y) <= theta || s >= kLogmMaxRoots;
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        m[i][j] = y[i][j];
                        if constexpr (DUAL) md[i][j] = yd[i][j];
                    }
            } else if (it >= kLogmMaxIter || !logm_finite<T, D>(m)) { // (singular: no need to wait)
                bad = true;
                done = true;
            }
        }
        bad = bad || !logm_finite<T, D>(y) || !(logm_dist1<T, D>(y) <= theta);
        // ---- z = (y - I) inv(y + I), into y; m holds inv(y + I)
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                m[i][j] = bad ? T(i == j ? 2 : 0) : y[i][j] + T(i == j ? 1 : 0);
                y[i][j] = bad ? T(0) : y[i][j] - T(i == j ? 1 : 0);
            }
        logm_inverse<T, D>(m);
        lie_fence();
        logm_rmul<T, D>(y, m);
        if constexpr (DUAL) {
            // z' = (I - z) y' inv(y + I)
            logm_rmul<T, D>(yd, m);
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) m[i][j] = T(i == j ? 1 : 0) - y[i][j];
            logm_lmul<T, D>(m, yd);
        }
        // ---- degree of the series (per lane)
        T zn = T(0);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            T c = T(0);
#pragma unroll
            for (int i = 0; i < D; ++i) c += fabs_(y[i][j]);
            zn = fmax_(zn, c);
        }
        int deg = 0;
        {
            const T zn2 = zn * zn;
            T pw = zn;
#pragma unroll 1
            while (deg < 16 && pw > E::eps * T(0.125) * T(2 * deg + 1)) {
                pw *= zn2;
                ++deg;
            }
        }
        // ---- w = z z (into m), p = sum_k w^k / (2k+1) by Horner
        Mat p;
        [[maybe_unused]] Dual wd, pd;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                T a = y[i][0] * y[0][j];
#pragma unroll
                for (int k = 1; k < D; ++k) a = fma_(y[i][k], y[k][j], a);
                m[i][j] = a;
                p[i][j] = i == j ? T(1) / T(2 * deg + 1) : T(0);
                if constexpr (DUAL) {
                    T b = T(0);
#pragma unroll
                    for (int k = 0; k < D; ++k) b = fma_(yd[i][k], y[k][j], b);
#pragma unroll
                    for (int k = 0; k < D; ++k) b = fma_(y[i][k], yd[k][j], b);
                    wd[i][j] = b;
                    pd[i][j] = T(0);
                }
            }
#pragma unroll 1
        for (int k = deg - 1; k >= 0; --k) {
            const T ck = T(1) / T(2 * k + 1);
#pragma unroll
            for (int j = 0; j < D; ++j) {
                T u[D];
                [[maybe_unused]] T ud[DD];
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    T a = i == j ? ck : T(0);
#pragma unroll
                    for (int q = 0; q < D; ++q) a = fma_(m[i][q], p[q][j], a);
                    u[i] = a;
                    if constexpr (DUAL) {
                        T b = T(0);
#pragma unroll
                        for (int q = 0; q < D; ++q) b = fma_(wd[i][q], p[q][j], b);
#pragma unroll
                        for (int q = 0; q < D; ++q) b = fma_(m[i][q], pd[q][j], b);
                        ud[i] = b;
                    }
                }
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    p[i][j] = u[i];
                    if constexpr (DUAL) pd[i][j] = ud[i];
                }
                lie_fence();
            }
        }
        // ---- log = 2^(s+1) z p,  log' = 2^(s+1) (z' p + z p')
        const T f = ldexp(T(1), s + 1);
        const T nan = __builtin_nan("");
        if constexpr (DUAL) {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                T u[D];
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    T b = T(0);
#pragma unroll
                    for (int k = 0; k < D; ++k) b = fma_(yd[i][k], p[k][j], b);
#pragma unroll
                    for (int k = 0; k < D; ++k) b = fma_(y[i][k], pd[k][j], b);
                    u[j] = b;
                }
#pragma unroll
                for (int j = 0; j < D; ++j) yd[i][j] = bad ? nan : f * u[j];
                lie_fence();
            }
        }
        logm_rmul<T, D>(y, p);
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) y[i][j] = bad ? nan : f * y[i][j];
    }
};

template <typename T>
__device__ __forceinline__ T logm_scalar(T x)
{
    return (__builtin_isfinite(x) && x > T(0)) ? T(log(x)) : T(__builtin_nan(""));
}

template <typename T, int D>
struct LogmOp {
    using RA = Rec<D, D>;
    using RB = NoRec;
    using RC = NoRec;
    using RO = Rec<D, D>;
    using Params = LogmParams;
    static constexpr int TILE = pick_tile(RA::C * (int)sizeof(T) + 16);
    static __device__ __forceinline__ void apply(const T (&a)[RA::Cs], const T (&)[1], const T (&)[1],
                                                 T (&r)[RO::Cs], const Params &)
    {
        NFM_LOGM_NO_CONTRACT
        if constexpr (D == 1) {
            r[0] = logm_scalar(a[0]);
        } else {
            T y[D][D], none[1][1];
#pragma unroll
            for (int k = 0; k < D * D; ++k) y[k / D][k % D] = a[k];
            LogmCore<T, D, false>::run(y, none);
#pragma unroll
            for (int k = 0; k < D * D; ++k) r[k] = y[k / D][k % D];
        }
    }
};

// inputs M, A: log(M^-1 A), one pivoted elimination on [M | A] in front of the same body
template <typename T, int D>
struct LogmSolveOp {
    using RA = Rec<D, D>;
    using RB = Rec<D, D>;
    using RC = NoRec;
    using RO = Rec<D, D>;
    using Params = LogmParams;
    static constexpr int TILE = pick_tile(2 * RA::C * (int)sizeof(T) + 16);
    static __device__ __forceinline__ void apply(const T (&mm)[RA::Cs], const T (&a)[RB::Cs], const T (&)[1],
                                                 T (&r)[RO::Cs], const Params &)
    {
        NFM_LOGM_NO_CONTRACT
        if constexpr (D == 1) {
            r[0] = logm_scalar(a[0] / mm[0]);
        } else {
            T y[D][D], none[1][1];
            {
                T lhs[D][D];
#pragma unroll
                for (int k = 0; k < D * D; ++k) {
                    lhs[k / D][k % D] = mm[k];
                    y[k / D][k % D] = a[k];
                }
                logm_solve<T, D>(lhs, y);
            }
            lie_fence();
            LogmCore<T, D, false>::run(y, none);
#pragma unroll
            for (int k = 0; k < D * D; ++k) r[k] = y[k / D][k % D];
        }
    }
};

// inputs X, G: L_log(X, G) = d/dt log(X + t G) at t = 0
template <typename T, int D>
struct LogmFrechetOp {
    using RA = Rec<D, D>;
    using RB = Rec<D, D>;
    using RC = NoRec;
    using RO = Rec<D, D>;
    using Params = LogmParams;
    static constexpr int TILE = pick_tile(2 * RA::C * (int)sizeof(T) + 16);
    static __device__ __forceinline__ void apply(const T (&x)[RA::Cs], const T (&g)[RB::Cs], const T (&)[1],
                                                 T (&r)[RO::Cs], const Params &)
    {
        NFM_LOGM_NO_CONTRACT
        if constexpr (D == 1) {
            r[0] = (__builtin_isfinite(x[0]) && x[0] > T(0)) ? g[0] / x[0] : T(__builtin_nan(""));
        } else {
            T y[D][D], yd[D][D];
#pragma unroll
            for (int k = 0; k < D * D; ++k) {
                y[k / D][k % D] = x[k];
                yd[k / D][k % D] = g[k];
            }
            LogmCore<T, D, true>::run(y, yd);
#pragma unroll
            for (int k = 0; k < D * D; ++k) r[k] = yd[k / D][k % D];
        }
    }
};

} // namespace nfm
