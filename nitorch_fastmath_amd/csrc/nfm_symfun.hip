// nfm_symfun.hip -- spectral functions of compact symmetric matrices (sym_funm and its gradient; an extension of
// `sym`, no counterpart in the reference).  One record per lane through rec_kernel: read the K = N (N + 1) / 2
// compact values, expand them into the triangle eig_sym1 reads, decompose in registers (FAST sweeps: f(A) depends
// neither on the deflation order nor on the eigenvector signs, and the fast mode is the one held to 16 n eps on
// repeated and clustered spectra), apply f to the eigenvalues, recompose the upper triangle, write K values.  The
// backward recomputes the decomposition from the saved input (saving V would cost N^2 values per record in HBM)
// and evaluates V [(V^T G V) o F] V^T with the closed-form divided differences of nfm_symfun_ops.hpp.  The
// expansion of a record and the sweeps' arguments are those of nfm_spectral.hpp, shared with the pencil kernels.
// fn, p and the clamp are run-time members of Params (a wave-uniform switch): the instantiations are
// (dtype, N, direction) x the layout kinds of rec_launch.
#include "nfm_record_kernel.hpp"
#include "nfm_spectral.hpp"

// This file is compiled seventeen times (-DNFM_SYMFUN_PART=0..16).  Part 0: the entry points, the caps and the CPU
// evaluation of the scalar pieces.  Parts 1..16: the kernels of one (dtype, direction, pair of orders):
// part = 1 + dtype * 8 + backward * 4 + pair, pair p = orders 2p + 1 and 2p + 2.  Each of them defines its own
// specialisation of symfun_part<PART>; part 0 reaches them through switch_order<16>.
#ifndef NFM_SYMFUN_PART
#error "compile with -DNFM_SYMFUN_PART=0..16"
#endif

namespace nfm {

using symfun::FunParams;

// The compiled caps: the largest order of each (dtype, direction) whose kernels have no private segment
// (profiles/symfun_table.md lists the registers of every instantiation).  Orders above take the caller's own route.
// (float64 backward at 8 x 8 holds u, the cotangent and W across the decomposition: its channel-first form needs 112
// bytes of scratch per lane, so the order is left to the caller's route)
constexpr int kSymFunCap[2][2] = {{8, 8}, {8, 7}}; // [dtype][backward]
constexpr bool symfun_fits(bool f64, bool bwd, int N) { return N >= 1 && N <= kSymFunCap[f64 ? 1 : 0][bwd ? 1 : 0]; }

template <typename T, int N>
struct SymFunOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>;
    using RB = NoRec;
    using RC = NoRec;
    using RO = Rec<1, K>;
    using Params = FunParams;
    static constexpr int TILE = pick_tile((RA::C + RO::C) * (int)sizeof(T) + 32);
    // as EigSymOp: from these orders on the kernel is bound by its dependent arithmetic and an LDS image of a
    // wavefront's records would only cost occupancy
    static constexpr bool kNoTile = N >= 5 || (N == 4 && sizeof(T) == 8);
    static __device__ __forceinline__ void apply(const T (&r)[RA::Cs], const T (&)[1], const T (&)[1],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        if constexpr (N == 1) {
            const T x = symfun::clamp_min(q, r[0]);
            o[0] = symfun::in_domain(q, x) ? symfun::fval(q, x) : symfun::nan_t<T>();
        } else {
            T u[N][N], f[N];
            bool bad;
            {
                T a[N][N], up[N][N];
                bad = spectral::expand<T, N>(r, a);
                qr::eig_sym1<T, N, true, true>(a, u, up, f, N, spectral::kMaxIter, spectral::kTol);
            } // a and up die here
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const T x = symfun::clamp_min(q, f[k]);
                bad |= !symfun::in_domain(q, x);
                f[k] = symfun::fval(q, x);
            }
            // Y_ij = sum_k V_ik f_k V_jk, i <= j: spectral::recompose<T, N, 1>, written out.  Built from the shared block
            // the float64 kernels of N = 3 and N = 8 need more registers and lose a wave per SIMD (a block's loops are
            // unrolled before it is inlined; u, indexed by literals only from then on, is promoted to one vector).
#pragma unroll
            for (int i = 0; i < N; ++i) {
                T t[N];
#pragma unroll
                for (int k = 0; k < N; ++k) t[k] = u[i][k] * f[k];
#pragma unroll
                for (int j = i; j < N; ++j) {
                    T y = t[0] * u[j][0];
#pragma unroll
                    for (int k = 1; k < N; ++k) y = qr::fma_t(t[k], u[j][k], y);
                    o[sym_idx(N, i, j)] = bad ? symfun::nan_t<T>() : y;
                }
            }
        }
    }
};

template <typename T, int N>
struct SymFunBwdOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>; // compact A
    using RB = Rec<1, K>; // compact cotangent of f(A)
    using RC = NoRec;
    using RO = Rec<1, K>; // compact gradient
    using Params = FunParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RO::C) * (int)sizeof(T) + 48);
    static constexpr bool kNoTile = SymFunOp<T, N>::kNoTile;
    static __device__ __forceinline__ void apply(const T (&r)[RA::Cs], const T (&g)[RB::Cs], const T (&)[1],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        if constexpr (N == 1) {
            const T x = symfun::clamp_min(q, r[0]);
            o[0] = symfun::in_domain(q, x) ? g[0] * symfun::divdiff(q, r[0], r[0]) : symfun::nan_t<T>();
        } else {
            T u[N][N], lam[N];
            bool bad;
            {
                T a[N][N], up[N][N];
                bad = spectral::expand<T, N>(r, a);
                qr::eig_sym1<T, N, true, true>(a, u, up, lam, N, spectral::kMaxIter, spectral::kTol);
            } // a and up die here
#pragma unroll
            for (int k = 0; k < N; ++k) bad |= !symfun::in_domain(q, symfun::clamp_min(q, lam[k]));
            // (these three steps are written out a second time, with Z and X for V, in PencilFunBwdOp of nfm_sympencil.hip:
            // built from shared blocks, the float32 kernel of N = 8 here needs a private segment)
            // W = V^T G V (symmetric, compact), G_ii = g_ii, G_ij = g_ij / 2: column l of G V, then row k <= l
            T w[K];
#pragma unroll
            for (int l = 0; l < N; ++l) {
                T t[N];
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    T s = g[i] * u[i][l];
#pragma unroll
                    for (int j = 0; j < N; ++j)
                        if (j != i) s = qr::fma_t(T(0.5) * g[sym_idx(N, i, j)], u[j][l], s);
                    t[i] = s;
                }
#pragma unroll
                for (int k = 0; k <= l; ++k) {
                    T s = u[0][k] * t[0];
#pragma unroll
                    for (int i = 1; i < N; ++i) s = qr::fma_t(u[i][k], t[i], s);
                    w[sym_idx(N, k, l)] = s;
                }
            }
            // W o F
#pragma unroll
            for (int k = 0; k < N; ++k)
#pragma unroll
                for (int l = k; l < N; ++l)
                    w[sym_idx(N, k, l)] *= bad ? T(0) : symfun::divdiff(q, lam[k], lam[l]);
            // S = V W V^T, i <= j: column j of W V^T, then row i <= j; compact result S_ii, 2 S_ij
#pragma unroll
            for (int j = 0; j < N; ++j) {
                T t[N];
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    T s = w[sym_idx(N, k, 0)] * u[j][0];
#pragma unroll
                    for (int l = 1; l < N; ++l) s = qr::fma_t(w[sym_idx(N, k, l)], u[j][l], s);
                    t[k] = s;
                }
#pragma unroll
                for (int i = 0; i <= j; ++i) {
                    T s = u[i][0] * t[0];
#pragma unroll
                    for (int k = 1; k < N; ++k) s = qr::fma_t(u[i][k], t[k], s);
                    o[sym_idx(N, i, j)] = bad ? symfun::nan_t<T>() : (i == j ? s : T(2) * s);
                }
            }
        }
    }
};

// one launcher per part: (M, mat, gout or NULL, out)
#define NFM_SYMFUN_ARGS                                                                                                \
    int M, const nfm_operand *a, const nfm_operand *g, const nfm_operand *o, int64_t no, int64_t ni, const FunParams &q, \
        void *stream
template <int PART>
int symfun_part(NFM_SYMFUN_ARGS);

#if NFM_SYMFUN_PART >= 1
template <>
int symfun_part<NFM_SYMFUN_PART>(NFM_SYMFUN_ARGS)
{
    constexpr int part = NFM_SYMFUN_PART - 1;
    constexpr bool F64 = part / 8 != 0, BWD = (part / 4) % 2 != 0;
    constexpr int N0 = 2 * (part % 4) + 1;
    using T = std::conditional_t<F64, double, float>;
    auto run = [&](auto n) -> int {
        constexpr int N = decltype(n)::value;
        if constexpr (symfun_fits(F64, BWD, N)) {
            if constexpr (BWD) return rec_launch<T, SymFunBwdOp<T, N>>(a, g, nullptr, o, no, ni, q, stream);
            else return rec_launch<T, SymFunOp<T, N>>(a, nullptr, nullptr, o, no, ni, q, stream);
        } else {
            return NFM_ESIZE;
        }
    };
    if (M == N0) return run(std::integral_constant<int, N0>{});
    if (M == N0 + 1) return run(std::integral_constant<int, N0 + 1>{});
    return NFM_ESIZE;
}
#endif

} // namespace nfm

#if NFM_SYMFUN_PART == 0
using namespace nfm;

static int symfun_check(int dtype, int M, int fn, double p, int has_min, double vmin, int backward, int64_t n_outer,
                        int64_t n_inner)
{
    const int rc = check_batch(dtype, n_outer, n_inner, {M});
    if (rc) return rc;
    return symfun::check_fun(true, fn, p, has_min, vmin, symfun_fits(dtype == NFM_F64, backward != 0, M));
}

static int symfun_dispatch(int dtype, int M, int backward, const nfm_operand *a, const nfm_operand *g,
                           const nfm_operand *o, int64_t no, int64_t ni, const FunParams &q, void *stream)
{
    const int part = (dtype == NFM_F64 ? 8 : 0) + (backward ? 4 : 0) + (M - 1) / 2;
    return switch_order<16>(part + 1, NFM_ESIZE, [&](auto p) {
        constexpr int P = p;
        return symfun_part<P>(M, a, g, o, no, ni, q, stream);
    });
}

template <typename T>
static void symfun_host_eval_t(const FunParams &q, int n, const T *lam, T *f, T *dd)
{
    for (int i = 0; i < n; ++i) {
        const T x = symfun::clamp_min(q, lam[i]);
        f[i] = symfun::in_domain(q, x) ? symfun::fval(q, x) : symfun::nan_t<T>();
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const bool ok = symfun::in_domain(q, symfun::clamp_min(q, lam[i])) &&
                            symfun::in_domain(q, symfun::clamp_min(q, lam[j]));
            dd[(size_t)i * n + j] = ok ? symfun::divdiff(q, lam[i], lam[j]) : symfun::nan_t<T>();
        }
}

extern "C" {

int nfm_sym_funm(int dtype, int M, int fn, double p, int has_min, double vmin, int64_t n_outer, int64_t n_inner,
                 const nfm_operand *mat, const nfm_operand *out, void *stream)
{
    int rc = symfun_check(dtype, M, fn, p, has_min, vmin, 0, n_outer, n_inner);
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {mat, out}))) return rc;
    const FunParams q{fn, has_min != 0, p, vmin};
    return symfun_dispatch(dtype, M, 0, mat, nullptr, out, n_outer, n_inner, q, stream);
}

int nfm_sym_funm_backward(int dtype, int M, int fn, double p, int has_min, double vmin, int64_t n_outer,
                          int64_t n_inner, const nfm_operand *mat, const nfm_operand *gout, const nfm_operand *gmat,
                          void *stream)
{
    int rc = symfun_check(dtype, M, fn, p, has_min, vmin, 1, n_outer, n_inner);
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {mat, gout, gmat}))) return rc;
    const FunParams q{fn, has_min != 0, p, vmin};
    return symfun_dispatch(dtype, M, 1, mat, gout, gmat, n_outer, n_inner, q, stream);
}

int nfm_sym_funm_max_order(int dtype, int backward)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return 0;
    return kSymFunCap[dtype == NFM_F64 ? 1 : 0][backward ? 1 : 0];
}

int nfm_sym_funm_host_eval(int dtype, int fn, double p, int has_min, double vmin, int n, const void *lam, void *f,
                           void *dd)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (n < 0 || symfun::check_fun(true, fn, p, has_min, vmin, true)) return NFM_EINVAL;
    if (n > 0 && (lam == nullptr || f == nullptr || dd == nullptr)) return NFM_EINVAL;
    const FunParams q{fn, has_min != 0, p, vmin};
    if (dtype == NFM_F32)
        symfun_host_eval_t<float>(q, n, static_cast<const float *>(lam), static_cast<float *>(f), static_cast<float *>(dd));
    else
        symfun_host_eval_t<double>(q, n, static_cast<const double *>(lam), static_cast<double *>(f),
                                   static_cast<double *>(dd));
    return NFM_OK;
}

} // extern "C"
#endif
