// nfm_special_ops.hpp -- arithmetic of the special functions (reference `special.py`): besseli,
// besseli_ratio, mvdigamma and their derivatives for ONE element.  Everything is __host__ __device__, so the
// same code runs in the kernels of nfm_special.hip and in nfm_special_host_eval (the CPU check of the tests).
//
// besseli, nu in {0, 1}: the reference's two Abramowitz & Stegun 9.8.1-9.8.4 polynomial branches split at
//   z = 15/4, in the value type, one operation per reference op in the reference's order and not contracted.
// besseli, any other nu: the documented function (the reference is wrong there), always
//   in double whatever the value type (why: DESIGN.md 4.9): log I_nu(z) from
//     series   sum_m q^m / (m! (nu+1)_m), q = z^2/4, by the term recurrence term *= q * c[m] with the
//              lane-uniform c[m] = 1 / (m (m + nu)) tabulated once per call on the host (no division and no
//              exp per term); stops when a term no longer changes the sum at the value type's precision;
//     uniform  A&S 9.7.7 with u_1..u_8, written in w = sqrt(nu^2 + z^2) and tau = nu^2 / w^2:
//              log I = w + nu log(z / (nu + w)) - log(2 pi w) / 2 + log(1 + sum_k p_k(tau) / w^k)
//              (no division by nu: valid down to nu = 0), used when w is above the value type's switch;
//   'norm' and 'log' never form exp(z).
// besseli_ratio: the reference's Amos (1974) arithmetic, the N + 1 running ratios in registers.
// digamma / trigamma: shift by the recurrence to x >= kShift, then the asymptotic (Bernoulli) series.
#pragma once
#include "nfm_common.hpp"

namespace nfm {
namespace special {

#define NFM_HD __host__ __device__ __forceinline__

constexpr int kMaxTerms = 160;  // series terms tabulated per call (reached only by backward calls near w = 90)
constexpr int kMaxN = 8;        // besseli_ratio: rounds of Amos eq. 20b held in registers
constexpr double kPi = 3.14159265358979323846;

NFM_HD float exp_t(float x) { return expf(x); }
NFM_HD double exp_t(double x) { return exp(x); }
NFM_HD float log_t(float x) { return logf(x); }
NFM_HD double log_t(double x) { return log(x); }
NFM_HD float sqrt_t(float x) { return sqrtf(x); }
NFM_HD double sqrt_t(double x) { return sqrt(x); }
NFM_HD float rint_t(float x) { return rintf(x); }
NFM_HD double rint_t(double x) { return rint(x); }
NFM_HD float tan_t(float x) { return tanf(x); }
NFM_HD double tan_t(double x) { return tan(x); }
NFM_HD float sin_t(float x) { return sinf(x); }
NFM_HD double sin_t(double x) { return sin(x); }
template <typename T>
NFM_HD T inf_t() { return T(__builtin_huge_val()); }
template <typename T>
NFM_HD T nan_t() { return T(__builtin_nan("")); }

// w = sqrt(nu^2 + z^2) at which the forward / backward routines leave the series for the uniform expansion.
// Truncation of the expansion after u_8 is below |p_9| / w^9 with |p_9| <= 25: 1e-8 at w = 11 (float32
// results), 1e-13 at w = 40 (float64); the derivative of a nu in {0, 1} result is held to rounding level
// in float64, hence the later switch of the backward pass (6e-17 at w = 90).
template <typename T>
struct Switch;
template <>
struct Switch<float> {
    static constexpr double fwd = 12.0, bwd = 12.0, tol = 1.0 / (1 << 30);
};
template <>
struct Switch<double> {
    static constexpr double fwd = 40.0, bwd = 90.0, tol = 1.0 / (1ull << 55);
};

// everything that depends on nu alone: filled once per call on the host, read from scalar registers
struct NuTab {
    double nu;
    double lg;            // lgamma(nu + 1)
    double c[kMaxTerms];  // c[m - 1] = 1 / (m (m + nu))
};

// ------------------------------------------------------------------ gamma family (the project's own)
// lgamma(x), x > 0, double: shift to x >= 16, Stirling with B_2 .. B_12 (next term 2e-19 at 16)
NFM_HD double lgamma_pos(double x)
{
    double prod = 1.0;
    while (x < 16.0) {
        prod *= x;
        x += 1.0;
    }
    const double i = 1.0 / x, i2 = i * i;
    const double s = i * (1.0 / 12 + i2 * (-1.0 / 360 + i2 * (1.0 / 1260 + i2 * (-1.0 / 1680 + i2 * (1.0 / 1188 + i2 * (-691.0 / 360360))))));
    return (x - 0.5) * log(x) - x + 0.91893853320467274178 + s - log(prod);
}

template <typename T>
struct Shift;
template <>
struct Shift<float> {
    static constexpr int at = 6, terms = 4;
};
template <>
struct Shift<double> {
    static constexpr int at = 10, terms = 7;
};

// torch.digamma's special values: 0 -> -inf (+0) / +inf (-0), negative integers -> NaN, reflection below 0
template <typename T>
NFM_HD T digamma(T x)
{
    if (x == T(0)) return (T(1) / x < T(0)) ? inf_t<T>() : -inf_t<T>();
    T refl = T(0);
    if (x < T(0)) {
        const T d = x - rint_t(x); // exact, in [-1/2, 1/2]: tan(pi x) = tan(pi d), and a tiny |x| keeps its digits
        if (d == T(0)) return nan_t<T>();
        refl = -T(kPi) / tan_t(T(kPi) * d);
        x = T(1) - x;
    }
    T acc = T(0);
    while (x < T(Shift<T>::at)) {
        acc = acc + T(1) / x;
        x = x + T(1);
    }
    const T i = T(1) / x, i2 = i * i;
    // sum_k B_2k / (2k x^2k)
    constexpr double B[7] = {1.0 / 12, -1.0 / 120, 1.0 / 252, -1.0 / 240, 1.0 / 132, -691.0 / 32760, 1.0 / 12};
    T s = T(0);
#pragma unroll
    for (int k = Shift<T>::terms - 1; k >= 0; --k) s = T(B[k]) + i2 * s;
    return log_t(x) - T(0.5) * i - i2 * s - acc + refl;
}

template <typename T>
NFM_HD T trigamma(T x)
{
    T sign = T(1), refl = T(0);
    if (x < T(0)) { // reflection: psi1(x) = pi^2 / sin^2(pi x) - psi1(1 - x), sin(pi x) = +-sin(pi d)
        const T sn = sin_t(T(kPi) * (x - rint_t(x)));
        refl = T(kPi * kPi) / (sn * sn);
        sign = T(-1);
        x = T(1) - x;
    }
    T acc = T(0);
    while (x < T(Shift<T>::at)) {
        acc = acc + T(1) / (x * x);
        x = x + T(1);
    }
    const T i = T(1) / x, i2 = i * i;
    // 1/x + 1/(2 x^2) + sum_k B_2k / x^(2k+1)
    constexpr double B[7] = {1.0 / 6, -1.0 / 30, 1.0 / 42, -1.0 / 30, 5.0 / 66, -691.0 / 2730, 7.0 / 6};
    T s = T(0);
#pragma unroll
    for (int k = Shift<T>::terms - 1; k >= 0; --k) s = T(B[k]) + i2 * s;
    return refl + sign * (acc + i * (T(1) + T(0.5) * i + i2 * s));
}

template <typename T>
NFM_HD T mvdigamma(T x, int order)
{
    T dg = digamma(x);
    for (int p = 2; p <= order; ++p) dg = dg + digamma(x + T((1 - p) * 0.5));
    return dg;
}

template <typename T>
NFM_HD T mvtrigamma(T x, int order)
{
    T tg = trigamma(x);
    for (int p = 2; p <= order; ++p) tg = tg + trigamma(x + T((1 - p) * 0.5));
    return tg;
}

// ------------------------------------------------------------------ besseli, nu in {0, 1}
// MODE 0: I, 1: I exp(-z), 2: log I.  The constants are A&S 9.8.1-9.8.4 as the reference writes them.
template <typename T, int NU, int MODE>
NFM_HD T besseli01(T z)
{
#pragma clang fp contract(off)
    T f;
    if (z < T(15.0 / 4.0)) {
        T t = z * T(4.0 / 15.0);
        t = t * t;
        if constexpr (NU == 0) {
            t = T(1) + t * (T(3.5156229) + t * (T(3.0899424) + t * (T(1.2067492) + t * (T(0.2659732) + t * (T(0.0360768) + t * T(0.0045813))))));
            f = MODE == 2 ? log_t(t) : (MODE == 1 ? t / exp_t(z) : t);
        } else {
            t = T(0.5) + t * (T(0.87890594) + t * (T(0.51498869) + t * (T(0.15084934) + t * (T(0.02658733) + t * (T(0.00301532) + t * T(0.00032411))))));
            f = MODE == 2 ? log_t(z) + log_t(t) : (MODE == 0 ? z * t : z * t / exp_t(z));
        }
    } else {
        T t = T(15.0 / 4.0) / z;
        if constexpr (NU == 0) {
            t = (T(0.39894228) + t * (T(0.01328592) + t * (T(0.00225319) + t * (T(-0.00157565) + t * (T(0.00916281) + t * (T(-0.02057706) + t * (T(0.02635537) + t * (T(-0.01647633) + t * T(0.0039237)))))))));
            t = t < T(1e-32) ? T(1e-32) : t;
        } else {
            t = T(0.398942281) + t * (T(-0.03988024) + t * (T(-0.00362018) + t * (T(0.00163801) + t * (T(-0.01031555) + t * (T(0.02282967) + t * (T(-0.02895312) + t * (T(0.01787654) - t * T(0.00420059))))))));
        }
        if (MODE == 2)
            f = z - T(0.5) * log_t(z) + log_t(t);
        else if (MODE == 1)
            f = t / sqrt_t(z);
        else
            f = exp_t(z) * t / sqrt_t(z);
        if (z == inf_t<T>()) f = MODE == 1 ? T(0) : z; // the limits (the reference: inf / inf, inf - inf)
    }
    return f;
}

// ------------------------------------------------------------------ besseli, general nu (double)
// p_k(tau), k = 1..8, with u_k(t) = t^k p_k(t^2) of A&S 9.3.9 (from the recurrence 9.3.10 in exact rationals)
NFM_HD double uae_sum(double tau, double iw)
{
    constexpr double P1[] = {0.125, -0.20833333333333334};
    constexpr double P2[] = {0.0703125, -0.4010416666666667, 0.3342013888888889};
    constexpr double P3[] = {0.0732421875, -0.8912109375, 1.8464626736111112, -1.0258125964506173};
    constexpr double P4[] = {0.112152099609375, -2.3640869140625, 8.78912353515625, -11.207002616222994, 4.669584423426247};
    constexpr double P5[] = {0.22710800170898438, -7.368794359479632, 42.53499874538846, -91.81824154324002, 84.63621767460073,
                             -28.212072558200244};
    constexpr double P6[] = {0.5725014209747314, -26.491430486951554, 218.1905117442116, -699.5796273761325, 1059.9904525279999,
                             -765.2524681411817, 212.57013003921713};
    constexpr double P7[] = {1.7277275025844574, -108.09091978839466, 1200.9029132163525, -5305.646978613403, 11655.393336864534,
                             -13586.550006434138, 8061.722181737309, -1919.457662318407};
    constexpr double P8[] = {6.074042001273483, -493.915304773088, 7109.514302489364, -41192.65496889755, 122200.46498301746,
                             -203400.17728041555, 192547.00123253153, -96980.59838863752, 20204.29133096615};
#define NFM_SP_POLY(P, n, out)                        \
    double out = P[n];                                \
    _Pragma("unroll") for (int j = n - 1; j >= 0; --j) out = P[j] + tau * out;
    NFM_SP_POLY(P1, 1, p1)
    NFM_SP_POLY(P2, 2, p2)
    NFM_SP_POLY(P3, 3, p3)
    NFM_SP_POLY(P4, 4, p4)
    NFM_SP_POLY(P5, 5, p5)
    NFM_SP_POLY(P6, 6, p6)
    NFM_SP_POLY(P7, 7, p7)
    NFM_SP_POLY(P8, 8, p8)
#undef NFM_SP_POLY
    return iw * (p1 + iw * (p2 + iw * (p3 + iw * (p4 + iw * (p5 + iw * (p6 + iw * (p7 + iw * p8)))))));
}

// log I_nu(z) by the uniform expansion; `shift` = z for the 'norm' mode: log(I exp(-z)) without w - z cancelling
NFM_HD double logi_uniform(double nu, double z, bool norm)
{
    const double w = sqrt(nu * nu + z * z);
    const double iw = 1.0 / w;
    const double tau = (nu * iw) * (nu * iw);
    const double lead = norm ? (nu * nu) / (w + z) : w;
    return lead + nu * log(z / (nu + w)) - 0.5 * log((2 * kPi) * w) + log1p(uae_sum(tau, iw));
}

// the series sum_m q^m / (m! (nu+1)_m); tol: stop when term < tol * sum
NFM_HD double series(const double *c, double q, double tol)
{
    double term = 1.0, sum = 1.0;
    for (int m = 0; m < kMaxTerms; ++m) {
        term *= q * c[m];
        sum += term;
        if (!(term >= tol * sum)) break;
    }
    return sum;
}

// log I_nu(z) (norm: minus z), z >= 0; NaN for z < 0 or NaN; z = 0 -> -inf (nu > 0) or 0; z = +inf -> +inf
template <typename T>
NFM_HD double logi(const NuTab &tb, double z, bool norm)
{
    const double nu = tb.nu;
    if (!(z >= 0.0)) return nan_t<double>();
    if (z == inf_t<double>()) return norm ? -z : z; // I exp(-z) -> 0
    if (nu * nu + z * z < Switch<T>::fwd * Switch<T>::fwd) {
        const double s = series(tb.c, 0.25 * z * z, Switch<T>::tol);
        double l = log(s) - tb.lg;
        if (nu != 0.0) l += nu * log(0.5 * z);
        return norm ? l - z : l;
    }
    return logi_uniform(nu, z, norm);
}

template <typename T, int MODE>
NFM_HD T besseli_any(const NuTab &tb, T z)
{
    const double l = logi<T>(tb, (double)z, MODE == 1);
    return T(MODE == 2 ? l : exp(l));
}

// r = I_{nu+1}(z) / I_nu(z), z >= 0 (tb1: the table of nu + 1)
template <typename T>
NFM_HD double ratio_any(const NuTab &tb, const NuTab &tb1, double z)
{
    const double nu = tb.nu;
    if (!(z >= 0.0)) return nan_t<double>();
    if (z == inf_t<double>()) return 1.0;
    if (nu * nu + z * z < Switch<T>::bwd * Switch<T>::bwd) {
        const double q = 0.25 * z * z;
        double t0 = 1.0, s0 = 1.0, t1 = 1.0, s1 = 1.0;
        for (int m = 0; m < kMaxTerms; ++m) {
            t0 *= q * tb.c[m];
            t1 *= q * tb1.c[m];
            s0 += t0;
            s1 += t1;
            if (!(t0 >= Switch<T>::tol * s0)) break; // t1 / s1 is the smaller
        }
        return (0.5 * z / (nu + 1.0)) * (s1 / s0);
    }
    // both orders by the uniform expansion, the difference of the logarithms term by term
    const double n1 = nu + 1.0;
    const double w0 = sqrt(nu * nu + z * z), w1 = sqrt(n1 * n1 + z * z);
    const double i0 = 1.0 / w0, i1 = 1.0 / w1;
    const double u0 = uae_sum((nu * i0) * (nu * i0), i0), u1 = uae_sum((n1 * i1) * (n1 * i1), i1);
    const double d = (2.0 * nu + 1.0) / (w0 + w1) + n1 * log(z / (n1 + w1)) - nu * log(z / (nu + w0)) - 0.5 * log(w1 * i0) +
                     log1p((u1 - u0) / (1.0 + u0));
    return exp(d);
}

// grad_z of besseli from z, the saved output and grad_out
template <typename T, int MODE>
NFM_HD T besseli_bwd(const NuTab &tb, const NuTab &tb1, T z, T out, T g)
{
    const double nu = tb.nu;
    const double zd = (double)z;
    if (zd == 0.0) { // the limits: I_nu ~ (z/2)^nu / Gamma(nu + 1), r -> 0
        if (nu == 0.0) return MODE == 1 ? -g : T(0) * g; // I_0 exp(-z) = 1 - z + ...; I_0 and log I_0 are flat
        if (MODE == 2) return g * inf_t<T>();
        // slope 1/2 at nu = 1 (with or without exp(-z)), 0 above, infinite below
        return g * (nu == 1.0 ? T(0.5) : (nu > 1.0 ? T(0) : inf_t<T>()));
    }
    const double r = ratio_any<T>(tb, tb1, zd);
    const double a = nu != 0.0 ? nu / zd : 0.0;
    if (MODE == 2) return T((double)g * (r + a));
    const double d = MODE == 1 ? (r - 1.0) + a : r + a; // d/dz log of the output
    return T((double)g * ((double)out * d));
}

// ------------------------------------------------------------------ besseli_ratio (Amos 1974)
template <typename T, int N>
NFM_HD T besseli_ratio(double nu, int K, T x)
{
#pragma clang fp contract(off)
    const double nu1 = nu + K;
    const T xx = x * x;
    T rk[N + 1];
#pragma unroll
    for (int k = 0; k <= N; ++k) { // eq. 20a
        T tmp = xx + T((nu1 + k + 1.5) * (nu1 + k + 1.5));
        tmp = sqrt_t(tmp);
        tmp = tmp + T(nu1 + k + 0.5);
        rk[k] = x / tmp;
    }
#pragma unroll
    for (int m = N; m > 0; --m) { // eq. 20b
#pragma unroll
        for (int k = 1; k <= m; ++k) {
            T tmp = rk[k] / rk[k - 1];
            tmp = tmp * xx;
            tmp = tmp + T((nu1 + k) * (nu1 + k));
            tmp = sqrt_t(tmp);
            tmp = tmp + T(nu1 + k);
            rk[k - 1] = x / tmp;
        }
    }
    T r = rk[0];
    const T ix = T(1) / x;
    for (int k = K; k > 0; --k) { // backward recurrence (eq. 2)
        r = r + T(2 * (nu + k)) * ix;
        r = T(1) / r;
    }
    // the limits (the reference: 0/0 in eq. 20b at 0, inf/inf in eq. 20a at +inf)
    if (x == T(0)) r = T(0);
    if (x == inf_t<T>()) r = T(1);
    return r;
}

// the Riccati identity r' = 1 - r^2 - (2 nu + 1) r / z on the saved output
template <typename T>
NFM_HD T besseli_ratio_bwd(double nu, T x, T r, T g)
{
    if (x == T(0)) return g * T(1.0 / (2.0 * nu + 2.0));
    if (x == inf_t<T>()) return T(0) * g;
    return g * (T(1) - r * r - T(2.0 * nu + 1.0) * r / x);
}

inline void fill_nutab(NuTab &tb, double nu)
{
    tb.nu = nu;
    tb.lg = lgamma_pos(nu + 1.0);
    for (int m = 1; m <= kMaxTerms; ++m) tb.c[m - 1] = 1.0 / ((double)m * ((double)m + nu));
}

} // namespace special
} // namespace nfm
