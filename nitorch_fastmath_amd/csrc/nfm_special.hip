// nfm_special.hip -- besseli / besseli_ratio / mvdigamma and their backward passes (reference `special.py`)
// over a flat range of n elements.  One kernel shape serves them all: a lane owns 16 bytes (4 float32 or
// 2 float64 elements) of every tensor, reads them with one 16-byte load each, evaluates the functor of
// nfm_special_ops.hpp on each element in registers and writes one 16-byte store; the elements past the
// last whole vector are done one per lane by the lanes of the last workgroup (scalar tail).  The vectors are
// element-aligned (VecOf::gtype), so a base pointer at any element offset takes the same path.  No LDS, no
// scratch; every input vector is in registers before the store, so out may alias an input.
#include "nfm_special_ops.hpp"

namespace nfm {
namespace special {

constexpr int kBlock = 256;

template <typename T, int NIN, class F>
__global__ __launch_bounds__(kBlock) void ew_kernel(const F f, const T *a, const T *b, const T *c, T *o, const int64_t n)
{
    constexpr int VEC = VecOf<T>::N;
    using VG = typename VecOf<T>::gtype;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t nvec = n / VEC;
    if (gid < nvec) {
        const VG va = NFM_LDG(reinterpret_cast<const VG *>(a) + gid);
        VG vb = va, vc = va;
        if constexpr (NIN > 1) vb = NFM_LDG(reinterpret_cast<const VG *>(b) + gid);
        if constexpr (NIN > 2) vc = NFM_LDG(reinterpret_cast<const VG *>(c) + gid);
        VG vo;
#pragma unroll
        for (int k = 0; k < VEC; ++k) vo[k] = f(va[k], vb[k], vc[k]);
        NFM_STG(vo, reinterpret_cast<VG *>(o) + gid);
    } else {
        const int64_t e = nvec * VEC + (gid - nvec); // tail: fewer than VEC elements
        if (e < n) {
            const T xa = a[e];
            const T xb = NIN > 1 ? b[e] : xa;
            const T xc = NIN > 2 ? c[e] : xa;
            o[e] = f(xa, xb, xc);
        }
    }
}

template <typename T, int NIN, class F>
static int launch(const F &f, const void *a, const void *b, const void *c, void *o, int64_t n, void *stream)
{
    constexpr int VEC = VecOf<T>::N;
    const int64_t lanes = n / VEC + n % VEC;
    const int64_t blocks = (lanes + kBlock - 1) / kBlock;
    if (blocks > INT32_MAX) return NFM_ESIZE;
    hipLaunchKernelGGL((ew_kernel<T, NIN, F>), dim3((unsigned)blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), f,
                       static_cast<const T *>(a), static_cast<const T *>(b), static_cast<const T *>(c), static_cast<T *>(o), n);
    return launch_status();
}

template <typename T, class F>
static void host_apply(const F &f, const void *a, const void *b, const void *c, void *o, int64_t n)
{
    const T *pa = static_cast<const T *>(a), *pb = static_cast<const T *>(b), *pc = static_cast<const T *>(c);
    T *po = static_cast<T *>(o);
    for (int64_t e = 0; e < n; ++e) po[e] = f(pa[e], pb ? pb[e] : pa[e], pc ? pc[e] : pa[e]);
}

// ---------------------------------------------------------------- functors (kernel arguments by value)
template <typename T, int NU, int MODE>
struct BesseliF {
    NFM_HD T operator()(T z, T, T) const { return besseli01<T, NU, MODE>(z); }
};
template <typename T, int MODE>
struct BesseliAnyF {
    NuTab tb;
    NFM_HD T operator()(T z, T, T) const { return besseli_any<T, MODE>(tb, z); }
};
template <typename T, int MODE>
struct BesseliBwdF {
    NuTab tb, tb1;
    NFM_HD T operator()(T z, T out, T g) const { return besseli_bwd<T, MODE>(tb, tb1, z, out, g); }
};
template <typename T, int N>
struct RatioF {
    double nu;
    int K;
    NFM_HD T operator()(T x, T, T) const { return besseli_ratio<T, N>(nu, K, x); }
};
template <typename T>
struct RatioBwdF {
    double nu;
    NFM_HD T operator()(T x, T r, T g) const { return besseli_ratio_bwd<T>(nu, x, r, g); }
};
template <typename T>
struct DigammaF {
    int order;
    NFM_HD T operator()(T x, T, T) const { return mvdigamma<T>(x, order); }
};
template <typename T>
struct TrigammaF {
    int order;
    NFM_HD T operator()(T x, T g, T) const { return g * mvtrigamma<T>(x, order); }
};

// one place runs a functor on the device (stream) or on the host (host == true: plain pointers)
template <typename T, int NIN, class F>
static int run(const F &f, bool host, const void *a, const void *b, const void *c, void *o, int64_t n, void *stream)
{
    if (host) {
        host_apply<T, F>(f, a, NIN > 1 ? b : nullptr, NIN > 2 ? c : nullptr, o, n);
        return NFM_OK;
    }
    return launch<T, NIN, F>(f, a, b, c, o, n, stream);
}

template <typename T>
static int besseli_fwd(bool host, int mode, double nu, int64_t n, const void *z, void *out, void *stream)
{
#define NFM_SP_MODE(M)                                                                              \
    case M:                                                                                         \
        if (nu == 0.0) return run<T, 1>(BesseliF<T, 0, M>{}, host, z, nullptr, nullptr, out, n, stream); \
        if (nu == 1.0) return run<T, 1>(BesseliF<T, 1, M>{}, host, z, nullptr, nullptr, out, n, stream); \
        {                                                                                           \
            BesseliAnyF<T, M> f;                                                                    \
            fill_nutab(f.tb, nu);                                                                   \
            return run<T, 1>(f, host, z, nullptr, nullptr, out, n, stream);                         \
        }
    switch (mode) {
        NFM_SP_MODE(0) NFM_SP_MODE(1) NFM_SP_MODE(2)
    default: return NFM_EINVAL;
    }
#undef NFM_SP_MODE
}

template <typename T, int MODE>
static int besseli_bwd_mode(bool host, double nu, int64_t n, const void *z, const void *out, const void *g, void *gz, void *stream)
{
    BesseliBwdF<T, MODE> f;
    fill_nutab(f.tb, nu);
    fill_nutab(f.tb1, nu + 1.0);
    return run<T, 3>(f, host, z, out, g, gz, n, stream);
}

template <typename T>
static int besseli_bwd_any(bool host, int mode, double nu, int64_t n, const void *z, const void *out, const void *g, void *gz,
                           void *stream)
{
    switch (mode) {
    case 0: return besseli_bwd_mode<T, 0>(host, nu, n, z, out, g, gz, stream);
    case 1: return besseli_bwd_mode<T, 1>(host, nu, n, z, out, g, gz, stream);
    case 2: return besseli_bwd_mode<T, 2>(host, nu, n, z, out, g, gz, stream);
    default: return NFM_EINVAL;
    }
}

template <typename T>
static int ratio_fwd(bool host, double nu, int N, int K, int64_t n, const void *x, void *out, void *stream)
{
#define NFM_SP_N(Nv) \
    case Nv: return run<T, 1>(RatioF<T, Nv>{nu, K}, host, x, nullptr, nullptr, out, n, stream);
    switch (N) {
        NFM_SP_N(0) NFM_SP_N(1) NFM_SP_N(2) NFM_SP_N(3) NFM_SP_N(4) NFM_SP_N(5) NFM_SP_N(6) NFM_SP_N(7) NFM_SP_N(8)
    default: return NFM_ESIZE;
    }
#undef NFM_SP_N
    static_assert(kMaxN == 8, "the switch above lists the compiled N");
}

static int check_ptr(const void *ptr, size_t elem, bool needed)
{
    if (ptr == nullptr) return needed ? NFM_EINVAL : NFM_OK;
    return reinterpret_cast<uintptr_t>(ptr) % elem == 0 ? NFM_OK : NFM_EALIGN;
}

static bool bad_nu(double nu) { return !(nu >= 0.0) || nu == __builtin_huge_val(); }

// the checks every entry point shares, in the order of the return codes' documentation
static int check(int dtype, bool bad_arg, bool too_large, int64_t n, const void *const *ptrs, int nptr)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (bad_arg || n < 0) return NFM_EINVAL;
    if (too_large) return NFM_ESIZE;
    const size_t elem = dtype == NFM_F32 ? 4 : 8;
    for (int k = 0; k < nptr; ++k)
        if (int rc = check_ptr(ptrs[k], elem, n > 0)) return rc;
    return NFM_OK;
}

static int besseli_entry(bool host, int dtype, int mode, double nu, int64_t n, const void *z, void *out, void *stream)
{
    const void *ptrs[] = {z, out};
    if (int rc = check(dtype, mode < 0 || mode > 2 || bad_nu(nu), false, n, ptrs, 2)) return rc;
    if (n == 0) return NFM_OK;
    return by_dtype(dtype, [&](auto t) { return besseli_fwd<decltype(t)>(host, mode, nu, n, z, out, stream); });
}

static int besseli_bwd_entry(bool host, int dtype, int mode, double nu, int64_t n, const void *z, const void *out,
                             const void *grad_out, void *grad_z, void *stream)
{
    const void *ptrs[] = {z, out, grad_out, grad_z};
    if (int rc = check(dtype, mode < 0 || mode > 2 || bad_nu(nu), false, n, ptrs, 4)) return rc;
    if (n == 0) return NFM_OK;
    return by_dtype(dtype, [&](auto t) {
        return besseli_bwd_any<decltype(t)>(host, mode, nu, n, z, out, grad_out, grad_z, stream);
    });
}

static int ratio_entry(bool host, int dtype, double nu, int N, int K, int64_t n, const void *x, void *out, void *stream)
{
    const void *ptrs[] = {x, out};
    if (int rc = check(dtype, bad_nu(nu) || N < 0 || K < 0, N > kMaxN, n, ptrs, 2)) return rc;
    if (n == 0) return NFM_OK;
    return by_dtype(dtype, [&](auto t) { return ratio_fwd<decltype(t)>(host, nu, N, K, n, x, out, stream); });
}

static int ratio_bwd_entry(bool host, int dtype, double nu, int64_t n, const void *x, const void *out, const void *grad_out,
                           void *grad_x, void *stream)
{
    const void *ptrs[] = {x, out, grad_out, grad_x};
    if (int rc = check(dtype, bad_nu(nu), false, n, ptrs, 4)) return rc;
    if (n == 0) return NFM_OK;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return run<T, 3>(RatioBwdF<T>{nu}, host, x, out, grad_out, grad_x, n, stream);
    });
}

static int digamma_entry(bool host, int dtype, int order, int64_t n, const void *x, void *out, void *stream)
{
    const void *ptrs[] = {x, out};
    if (int rc = check(dtype, order < 1, false, n, ptrs, 2)) return rc;
    if (n == 0) return NFM_OK;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return run<T, 1>(DigammaF<T>{order}, host, x, nullptr, nullptr, out, n, stream);
    });
}

static int digamma_bwd_entry(bool host, int dtype, int order, int64_t n, const void *x, const void *grad_out, void *grad_x,
                             void *stream)
{
    const void *ptrs[] = {x, grad_out, grad_x};
    if (int rc = check(dtype, order < 1, false, n, ptrs, 3)) return rc;
    if (n == 0) return NFM_OK;
    return by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return run<T, 2>(TrigammaF<T>{order}, host, x, grad_out, nullptr, grad_x, n, stream);
    });
}

} // namespace special
} // namespace nfm

using namespace nfm;

extern "C" {

int nfm_special_besseli(int dtype, int mode, double nu, int64_t n, const void *z, void *out, void *stream)
{
    return special::besseli_entry(false, dtype, mode, nu, n, z, out, stream);
}

int nfm_special_besseli_backward(int dtype, int mode, double nu, int64_t n, const void *z, const void *out, const void *grad_out,
                                 void *grad_z, void *stream)
{
    return special::besseli_bwd_entry(false, dtype, mode, nu, n, z, out, grad_out, grad_z, stream);
}

int nfm_special_besseli_ratio(int dtype, double nu, int N, int K, int64_t n, const void *x, void *out, void *stream)
{
    return special::ratio_entry(false, dtype, nu, N, K, n, x, out, stream);
}

int nfm_special_besseli_ratio_backward(int dtype, double nu, int64_t n, const void *x, const void *out, const void *grad_out,
                                       void *grad_x, void *stream)
{
    return special::ratio_bwd_entry(false, dtype, nu, n, x, out, grad_out, grad_x, stream);
}

int nfm_special_mvdigamma(int dtype, int order, int64_t n, const void *x, void *out, void *stream)
{
    return special::digamma_entry(false, dtype, order, n, x, out, stream);
}

int nfm_special_mvdigamma_backward(int dtype, int order, int64_t n, const void *x, const void *grad_out, void *grad_x,
                                   void *stream)
{
    return special::digamma_bwd_entry(false, dtype, order, n, x, grad_out, grad_x, stream);
}

int nfm_special_host_eval(int func, int dtype, int mode_or_order, double nu, int N, int K, int64_t n, const void *x,
                          const void *saved_out, const void *grad_out, void *result)
{
    switch (func) {
    case NFM_SPECIAL_BESSELI: return special::besseli_entry(true, dtype, mode_or_order, nu, n, x, result, nullptr);
    case NFM_SPECIAL_BESSELI_BWD:
        return special::besseli_bwd_entry(true, dtype, mode_or_order, nu, n, x, saved_out, grad_out, result, nullptr);
    case NFM_SPECIAL_RATIO: return special::ratio_entry(true, dtype, nu, N, K, n, x, result, nullptr);
    case NFM_SPECIAL_RATIO_BWD: return special::ratio_bwd_entry(true, dtype, nu, n, x, saved_out, grad_out, result, nullptr);
    case NFM_SPECIAL_MVDIGAMMA: return special::digamma_entry(true, dtype, mode_or_order, n, x, result, nullptr);
    case NFM_SPECIAL_MVDIGAMMA_BWD: return special::digamma_bwd_entry(true, dtype, mode_or_order, n, x, grad_out, result, nullptr);
    default: return NFM_EINVAL;
    }
}

} // extern "C"
