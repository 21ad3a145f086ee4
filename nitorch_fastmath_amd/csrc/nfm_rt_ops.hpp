// nfm_rt_ops.hpp -- arithmetic of the real transforms (reference `realtransforms.py`): DCT / DST of types
// I, II, III along ONE line of N elements, as a direct sum against a table of cosines / sines.
//
// Every transform is   y = diag(post) B diag(pre) x   with B a matrix of pure 2 cos / 2 sin entries:
//     DCT-II  B[k][n] = 2 cos(pi k (2n+1) / 2N)        DST-II  B[k][n] = 2 sin(pi (k+1) (2n+1) / 2N)
//     DCT-III B[k][n] = 2 cos(pi (2k+1) n / 2N)        DST-III B[k][n] = 2 sin(pi (2k+1) (n+1) / 2N)
//     DCT-I   B[k][n] = 2 cos(pi k n / (N-1))          DST-I   B[k][n] = 2 sin(pi (k+1) (n+1) / (N+1))
// `pre` differs from one only at the first / last input term and `post` is one factor for all outputs but the
// first / last: the halved end terms of types I and III, the global factor of `forward` / `ortho` and the
// end-term corrections of `ortho` / `ortho_scipy` all live there (make_plan).  B of type III is the transpose
// of B of type II and B of type I is symmetric, so the transposed operator is the other B with pre and post
// swapped.
//
// The entry B[k][n] is table[(a_k + n s_k) mod P] with the table 2 cos / 2 sin(pi m / D), m = 0..P-1, P = 2 D:
// the index advances by a constant per term, and the angle is reduced in integers to the first octant
// (unit_cos), so that every entry carries the relative error of one cospi / sinpi and the zeros of the
// matrix are exact zeros.  The same routine (`lines`) serves the kernels (table and line in LDS) and the
// host entry point.
#pragma once
#include <math.h>
#include "nfm_common.hpp"

namespace nfm {
namespace rt {

struct Plan {
    int sine;           // 0: cosines, 1: sines
    int N;              // line length
    int D, P;           // table: angle unit pi / D, period P = 2 D
    int a1, a0, s1, s0; // output k starts at index a1 k + a0 and advances by s1 k + s0 per input term
    double pre_first, pre_last;              // factors of the first / last input term
    double post_first, post_mid, post_last;  // factors of the first / inner / last output term
};

// the checks of (kind, type, norm, N) are the entry point's; transpose != 0: the transposed operator
inline Plan make_plan(int kind, int type, int norm, int transpose, int N)
{
    Plan p;
    p.sine = kind;
    p.N = N;
    const int L = type == 1 ? (kind ? N + 1 : N - 1) : N; // the "logical" half-period
    double pre0 = 1, pre1 = 1, post0 = 1, post1 = 1;
    // the end terms that enter with half the weight of the others
    if (type == 3) (kind ? pre1 : pre0) = 0.5;
    if (type == 1 && !kind) pre0 = pre1 = 0.5;
    double f = 1;
    if (norm == NFM_RT_FORWARD) f = 1.0 / (2.0 * L);
    if (norm == NFM_RT_ORTHO || norm == NFM_RT_ORTHO_SCIPY) {
        f = 1.0 / sqrt(2.0 * L);
        const double r2 = sqrt(2.0), h2 = sqrt(0.5);
        const bool first = !kind || (norm == NFM_RT_ORTHO_SCIPY && type != 1); // which end term is corrected
        if (type == 2) (first ? post0 : post1) *= h2;
        if (type == 3) (first ? pre0 : pre1) *= r2;
        if (type == 1 && !kind) {
            pre0 *= r2, pre1 *= r2;
            post0 *= h2, post1 *= h2;
        }
    }
    int bt = type;
    if (transpose) {
        bt = type == 1 ? 1 : 5 - type;
        double t = pre0;
        pre0 = post0, post0 = t;
        t = pre1, pre1 = post1, post1 = t;
    }
    if (N == 1) { // the first term is the last one
        pre0 *= pre1, pre1 = 1;
        post0 *= post1, post1 = 1;
    }
    p.pre_first = pre0, p.pre_last = pre1;
    p.post_first = f * post0, p.post_mid = f, p.post_last = f * post1;
    p.D = bt == 1 ? L : 2 * N;
    p.P = 2 * p.D;
    const int c = kind ? 1 : 0;
    if (bt == 2) p.a1 = 1, p.a0 = c, p.s1 = 2, p.s0 = 2 * c;
    else if (bt == 3) p.a1 = 2 * c, p.a0 = c, p.s1 = 2, p.s0 = 1;
    else p.a1 = c, p.a0 = c, p.s1 = 1, p.s0 = c;
    return p;
}

__host__ __device__ inline float fma_t(float a, float b, float c) { return fmaf(a, b, c); }
__host__ __device__ inline double fma_t(double a, double b, double c) { return fma(a, b, c); }

// cos(pi x) and sin(pi x) for 0 <= x <= 1/4
__host__ __device__ inline float cospi_t(float x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return cospif(x);
#else
    return (float)cos(M_PI * (double)x);
#endif
}
__host__ __device__ inline double cospi_t(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return cospi(x);
#else
    return cos(M_PI * x);
#endif
}
__host__ __device__ inline float sinpi_t(float x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return sinpif(x);
#else
    return (float)sin(M_PI * (double)x);
#endif
}
__host__ __device__ inline double sinpi_t(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return sinpi(x);
#else
    return sin(M_PI * x);
#endif
}

// cos(pi q / D) for 0 <= q < 2 D: folded in integers into [0, pi/4] (no floating fmod, exact zeros)
template <typename T>
__host__ __device__ inline T unit_cos(int q, int D)
{
    if (q > D) q = 2 * D - q;
    bool neg = false;
    if (2 * q > D) {
        q = D - q;
        neg = true;
    }
    const T v = 4 * q <= D ? cospi_t(T(q) / T(D)) : sinpi_t(T(D - 2 * q) / T(2 * D));
    return neg ? -v : v;
}

// entry m of the table: 2 cos(pi m / D) or 2 sin(pi m / D) = 2 cos(pi (D - 2m) / 2D)
template <typename T>
__host__ __device__ inline T table_entry(const Plan &p, int m)
{
    if (!p.sine) return T(2) * unit_cos<T>(m, p.D);
    int r = p.D - 2 * m; // in (-3D, D]
    if (r < 0) r += 4 * p.D;
    return T(2) * unit_cos<T>(r, 2 * p.D);
}

// The transform of VEC lines at once: xs.get(n, v) -- term n of the lines, already scaled by `pre`;
// ys.put(k, v) -- output k.  KB outputs share one pass over the input terms.
template <typename T, int VEC, int KB, class XS, class YS>
__host__ __device__ __forceinline__ void lines(const Plan &p, const T *tab, const XS &xs, YS &ys)
{
    const int N = p.N, P = p.P;
    const T post_first = (T)p.post_first, post_mid = (T)p.post_mid, post_last = (T)p.post_last;
    for (int k0 = 0; k0 < N; k0 += KB) {
        int idx[KB], step[KB];
        T acc[KB][VEC];
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            const int k = k0 + j < N ? k0 + j : N - 1; // (outputs past the end repeat the last one, unwritten)
            idx[j] = p.a1 * k + p.a0;
            step[j] = p.s1 * k + p.s0;
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[j][v] = T(0);
        }
        for (int n = 0; n < N; ++n) {
            T x[VEC];
            xs.get(n, x);
#pragma unroll
            for (int j = 0; j < KB; ++j) {
                const T c = tab[idx[j]];
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[j][v] = fma_t(c, x[v], acc[j][v]);
                idx[j] += step[j];
                if (idx[j] >= P) idx[j] -= P;
            }
        }
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            const int k = k0 + j;
            if (k < N) {
                const T s = k == 0 ? post_first : (k == N - 1 ? post_last : post_mid);
                T y[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) y[v] = acc[j][v] * s;
                ys.put(k, y);
            }
        }
    }
}

} // namespace rt
} // namespace nfm
