// nfm_symfun_ops.hpp -- the scalar pieces of sym_funm (spectral functions of compact symmetric matrices):
// the clamp, the domain test, f and its first divided difference f[a, b] in closed form, for ONE eigenvalue (pair).
// Everything is __host__ __device__: the kernels of nfm_symfun.hip and the CPU entry nfm_sym_funm_host_eval run the
// same source, so the host tests check the formulas the GPU evaluates.
//
// Why closed forms: the gradient of f(A) is V [(V^T G V) o F] V^T with F_kl = f[l_k, l_l] (Daleckii-Krein), and the
// quotient (f(a) - f(b)) / (a - b) loses every digit as a -> b -- which is where isotropic and clustered spectra
// live.  Each form below keeps a relative error of a few eps for every pair of its domain:
//   exp    exp((a + b) / 2) sinh(h) / h, h = (a - b) / 2           (series of sinh(h) / h for |h| < 2^-6)
//   log    log1p(t) / (t b), t = (a - b) / b, b the smaller one    (t >= 0: 1 + t never cancels)
//   sqrt   1 / (sqrt a + sqrt b)
//   rsqrt  -1 / (sqrt a sqrt b (sqrt a + sqrt b))
//   pow    b^(p-1) expm1(p log1p(t)) / t while |p log1p(t)| <= 1, the quotient beyond (no cancellation there)
//   a == b gives f'(a).
// With a lower clamp the function is g = f o max(., min) and g[a, b] = f[ac, bc] (ac - bc) / (a - b), ac and bc the
// clamped values; for a == b the second factor is 1 (a >= min, torch's convention for clamp at the kink) or 0.
#pragma once
#include "nfm_common.hpp"
#include <cmath>

namespace nfm {
namespace symfun {

#ifndef NFM_HD
#define NFM_HD __host__ __device__ __forceinline__
#endif

// run-time description of the function: wave-uniform in a kernel (the kernels are NOT templated on fn)
struct FunParams {
    int fn;      // NFM_FUN_*
    int has_min; // clamp the eigenvalues from below first
    double p;    // exponent of NFM_FUN_POW
    double vmin; // the clamp
};

// The argument check of a function code at an entry point, in the documented order: the code, then the cap (`fits`),
// then the values.  `clamp`: the entry takes a lower clamp (has_min, vmin) and NFM_FUN_CLAMP; a pencil takes neither
// and passes vmin = 0.
inline int check_fun(bool clamp, int fn, double p, int has_min, double vmin, bool fits)
{
    if (fn < NFM_FUN_EXP || fn > (clamp ? NFM_FUN_CLAMP : NFM_FUN_POW) || (has_min && !clamp)) return NFM_EINVAL;
    if (!fits) return NFM_ESIZE;
    if (!std::isfinite(p) || !std::isfinite(vmin)) return NFM_EINVAL;
    if (fn == NFM_FUN_CLAMP && !has_min) return NFM_EINVAL;
    return NFM_OK;
}

NFM_HD float exp_t(float x) { return expf(x); }
NFM_HD double exp_t(double x) { return exp(x); }
NFM_HD float log_t(float x) { return logf(x); }
NFM_HD double log_t(double x) { return log(x); }
NFM_HD float log1p_t(float x) { return log1pf(x); }
NFM_HD double log1p_t(double x) { return log1p(x); }
NFM_HD float expm1_t(float x) { return expm1f(x); }
NFM_HD double expm1_t(double x) { return expm1(x); }
NFM_HD float sinh_t(float x) { return sinhf(x); }
NFM_HD double sinh_t(double x) { return sinh(x); }
NFM_HD float pow_t(float x, float p) { return powf(x, p); }
NFM_HD double pow_t(double x, double p) { return pow(x, p); }
NFM_HD float sqrt_t(float x) { return sqrtf(x); }
NFM_HD double sqrt_t(double x) { return sqrt(x); }
NFM_HD float abs_t(float x) { return fabsf(x); }
NFM_HD double abs_t(double x) { return fabs(x); }
template <typename T>
NFM_HD T nan_t()
{
    return T(__builtin_nanf(""));
}
template <typename T>
NFM_HD bool finite_t(T x)
{
    return abs_t(x) < T(__builtin_huge_valf()); // false for inf and for NaN
}

// max(x, min) where a clamp is set; a NaN stays a NaN
template <typename T>
NFM_HD T clamp_min(const FunParams &q, T x)
{
    const T m = T(q.vmin);
    return (q.has_min && x < m) ? m : x;
}

// is the (clamped) eigenvalue x in the domain of f?  A NaN or an inf is in no domain.
template <typename T>
NFM_HD bool in_domain(const FunParams &q, T x)
{
    if (!finite_t(x)) return false;
    switch (q.fn) {
    case NFM_FUN_LOG:
    case NFM_FUN_RSQRT: return x > T(0);
    case NFM_FUN_SQRT: return x >= T(0);
    case NFM_FUN_POW: return q.p < 0.0 ? x > T(0) : x >= T(0);
    default: return true; // exp, clamp
    }
}

// f at a clamped eigenvalue of its domain
template <typename T>
NFM_HD T fval(const FunParams &q, T x)
{
    switch (q.fn) {
    case NFM_FUN_EXP: return exp_t(x);
    case NFM_FUN_LOG: return log_t(x);
    case NFM_FUN_SQRT: return sqrt_t(x);
    case NFM_FUN_RSQRT: return T(1) / sqrt_t(x);
    case NFM_FUN_POW: return pow_t(x, T(q.p));
    default: return x; // clamp
    }
}

// f'(a)
template <typename T>
NFM_HD T fprime(const FunParams &q, T a)
{
    switch (q.fn) {
    case NFM_FUN_EXP: return exp_t(a);
    case NFM_FUN_LOG: return T(1) / a;
    case NFM_FUN_SQRT: return T(0.5) / sqrt_t(a);
    case NFM_FUN_RSQRT: return T(-0.5) / (a * sqrt_t(a));
    case NFM_FUN_POW: {
        const T p = T(q.p);
        return p == T(0) ? T(0) : p * pow_t(a, p - T(1));
    }
    default: return T(1);
    }
}

// sinh(h) / h
template <typename T>
NFM_HD T sinhc(T h)
{
    const T h2 = h * h;
    if (h2 < T(0x1p-12)) // |h| < 2^-6: the next term is h^8 / 9! < 2^-66
        return T(1) + h2 * (T(1.0 / 6.0) + h2 * (T(1.0 / 120.0) + h2 * T(1.0 / 5040.0)));
    return sinh_t(h) / h;
}

// f[a, b] for two eigenvalues of the domain (no clamp here)
template <typename T>
NFM_HD T divdiff0(const FunParams &q, T a, T b)
{
    if (a == b) return fprime(q, a);
    switch (q.fn) {
    case NFM_FUN_EXP: return exp_t(T(0.5) * a + T(0.5) * b) * sinhc(T(0.5) * a - T(0.5) * b);
    case NFM_FUN_LOG: {
        const T lo = a < b ? a : b, hi = a < b ? b : a;
        const T t = (hi - lo) / lo;
        return log1p_t(t) / (t * lo);
    }
    case NFM_FUN_SQRT: return T(1) / (sqrt_t(a) + sqrt_t(b));
    case NFM_FUN_RSQRT: {
        const T sa = sqrt_t(a), sb = sqrt_t(b);
        return T(-1) / (sa * sb * (sa + sb));
    }
    case NFM_FUN_POW: {
        const T p = T(q.p);
        if (p == T(0)) return T(0);
        const T lo = a < b ? a : b, hi = a < b ? b : a;
        const T t = (hi - lo) / lo; // +inf for lo == 0: the quotient below
        const T u = p * log1p_t(t);
        if (abs_t(u) <= T(1)) return pow_t(lo, p - T(1)) * (expm1_t(u) / t);
        return (pow_t(hi, p) - pow_t(lo, p)) / (hi - lo);
    }
    default: return T(1);
    }
}

// (f o max(., min))[a, b] for the UNCLAMPED eigenvalues a, b whose clamped values are in the domain
template <typename T>
NFM_HD T divdiff(const FunParams &q, T a, T b)
{
    const T ca = clamp_min(q, a), cb = clamp_min(q, b);
    T fac = T(1);
    if (q.has_min) {
        if (a == b) fac = a >= T(q.vmin) ? T(1) : T(0);
        else if (ca != a || cb != b) fac = (ca - cb) / (a - b);
    }
    if (fac == T(0)) return T(0);
    const T d = divdiff0(q, ca, cb);
    return fac == T(1) ? d : fac * d;
}

} // namespace symfun
} // namespace nfm
