// nfm_sympencil.hip -- two-matrix spectral kernels of compact symmetric matrices (an extension of `sym`, the step
// past sym_funm; no counterpart in the reference): functions of a pencil (A, B), A positive definite,
//   G = A^1/2 f(A^-1/2 B A^-1/2) A^1/2   (f = mu^t: the geodesic point A #_t B; log / exp: the Riemannian log / exp map)
// their gradient with respect to B, the generalised eigenvalues of B x = mu A x, the affine-invariant distance
// d = ||log(A^-1/2 B A^-1/2)||_F and its gradients.  One record per lane through rec_kernel: both compact records are
// read once, the two decompositions and the products between them stay in the lane's registers
// (nfm_sympencil_ops.hpp; the blocks shared with sym_funm are in nfm_spectral.hpp), the result is written once.
#include "nfm_record_kernel.hpp"
#include "nfm_sympencil_ops.hpp"

// This file is compiled 33 times (-DNFM_SYMPENCIL_PART=0..32).  Part 0: the entry points and the caps.
// Parts 1..32: the kernels of one (dtype, op, pair of orders): part = 1 + dtype * 16 + op * 4 + pair, pair p = orders
// 2p + 1 and 2p + 2; op: 0 function, 1 its gradient, 2 eigenvalues / distance, 3 gradients of the distance.  Each of
// them defines its own specialisation of sympencil_part<PART>; part 0 reaches them through switch_order<32>.
#ifndef NFM_SYMPENCIL_PART
#error "compile with -DNFM_SYMPENCIL_PART=0..32"
#endif

namespace nfm {

using symfun::FunParams;
using sympencil::EigParams;

// The compiled caps: the largest order of each (dtype, op) whose kernels have no private segment
// (profiles/sympencil_table.md lists the registers of every instantiation).  Orders above take the caller's route.
// Every order up to 8 was compiled; the first one with scratch in some layout kind: float32 gradient 7 (8 bytes),
// float64 function 8 (432), gradient 7 (748), gradients of the distance 8 (160).
constexpr int kSymPencilCap[2][4] = {{8, 6, 8, 8}, {7, 6, 8, 7}}; // [dtype][op]
constexpr bool sympencil_fits(bool f64, int op, int N) { return N >= 1 && N <= kSymPencilCap[f64 ? 1 : 0][op]; }

// G = Z f(M) Z^T
template <typename T, int N>
struct PencilFunOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>; // compact A (the base)
    using RB = Rec<1, K>; // compact B
    using RC = NoRec;
    using RO = Rec<1, K>;
    using Params = FunParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RO::C) * (int)sizeof(T) + 48);
    static constexpr bool kNoTile = N >= 5 || (N == 4 && sizeof(T) == 8); // as SymFunOp
    static __device__ __forceinline__ void apply(const T (&ra)[RA::Cs], const T (&rb)[RB::Cs], const T (&)[1],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        if constexpr (N == 1) {
            const T mu = rb[0] / ra[0];
            const bool ok = sympencil::scalar_ok(ra[0], rb[0]) && symfun::in_domain(q, mu);
            o[0] = ok ? ra[0] * symfun::fval(q, mu) : symfun::nan_t<T>();
        } else {
            T z[N][N], f[N];
            bool bad;
            {
                T lam[N], qq[N][N];
                {
                    T c[N][N], up[N][N];
                    bad = sympencil::whiten<T, N>(ra, rb, z, lam, c);
                    qr::eig_sym1<T, N, true, true>(c, qq, up, f, N, spectral::kMaxIter, spectral::kTol);
                }
                sympencil::times_q<T, N, true>(z, lam, qq); // Z = W L Q
            }
#pragma unroll
            for (int k = 0; k < N; ++k) {
                bad |= !symfun::in_domain(q, f[k]);
                f[k] = symfun::fval(q, f[k]);
            }
            spectral::recompose<T, N, 1>(z, f, bad, o);
        }
    }
};

// gradient of G with respect to B: X [(Z^T Gbar Z) o F] X^T
template <typename T, int N>
struct PencilFunBwdOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>; // compact A
    using RB = Rec<1, K>; // compact B
    using RC = Rec<1, K>; // compact cotangent of G
    using RO = Rec<1, K>; // compact gradient with respect to B
    using Params = FunParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RC::C + RO::C) * (int)sizeof(T) + 64);
    static constexpr bool kNoTile = PencilFunOp<T, N>::kNoTile;
    static __device__ __forceinline__ void apply(const T (&ra)[RA::Cs], const T (&rb)[RB::Cs], const T (&g)[RC::Cs],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        if constexpr (N == 1) {
            const T mu = rb[0] / ra[0];
            const bool ok = sympencil::scalar_ok(ra[0], rb[0]) && symfun::in_domain(q, mu);
            o[0] = ok ? g[0] * symfun::divdiff(q, mu, mu) : symfun::nan_t<T>();
        } else {
            T x[N][N], z[N][N], mu[N];
            bool bad;
            {
                T lam[N], qq[N][N];
                {
                    T c[N][N], up[N][N];
                    bad = sympencil::whiten<T, N>(ra, rb, x, lam, c);
                    qr::eig_sym1<T, N, true, true>(c, qq, up, mu, N, spectral::kMaxIter, spectral::kTol);
                }
#pragma unroll
                for (int i = 0; i < N; ++i)
#pragma unroll
                    for (int k = 0; k < N; ++k) z[i][k] = x[i][k];
                sympencil::times_q<T, N, true>(z, lam, qq);  // Z = W L Q
                sympencil::times_q<T, N, false>(x, lam, qq); // X = W Q
            }
#pragma unroll
            for (int k = 0; k < N; ++k) bad |= !symfun::in_domain(q, mu[k]);
            // (the three steps of SymFunBwdOp, nfm_symfun.hip, with Z and X for V: see there why they are written twice)
            // H = Z^T Gbar Z (symmetric, compact), Gbar_ii = g_ii, Gbar_ij = g_ij / 2: column l of Gbar Z, then rows k <= l
            T h[K];
#pragma unroll
            for (int l = 0; l < N; ++l) {
                T t[N];
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    T s = g[i] * z[i][l];
#pragma unroll
                    for (int j = 0; j < N; ++j)
                        if (j != i) s = qr::fma_t(T(0.5) * g[sym_idx(N, i, j)], z[j][l], s);
                    t[i] = s;
                }
#pragma unroll
                for (int k = 0; k <= l; ++k) {
                    T s = z[0][k] * t[0];
#pragma unroll
                    for (int i = 1; i < N; ++i) s = qr::fma_t(z[i][k], t[i], s);
                    h[sym_idx(N, k, l)] = s;
                }
            }
            // H o F
#pragma unroll
            for (int k = 0; k < N; ++k)
#pragma unroll
                for (int l = k; l < N; ++l) h[sym_idx(N, k, l)] *= bad ? T(0) : symfun::divdiff(q, mu[k], mu[l]);
            // S = X H X^T, i <= j; compact result S_ii, 2 S_ij
#pragma unroll
            for (int j = 0; j < N; ++j) {
                T t[N];
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    T s = h[sym_idx(N, k, 0)] * x[j][0];
#pragma unroll
                    for (int l = 1; l < N; ++l) s = qr::fma_t(h[sym_idx(N, k, l)], x[j][l], s);
                    t[k] = s;
                }
#pragma unroll
                for (int i = 0; i <= j; ++i) {
                    T s = x[i][0] * t[0];
#pragma unroll
                    for (int k = 1; k < N; ++k) s = qr::fma_t(x[i][k], t[k], s);
                    o[sym_idx(N, i, j)] = bad ? symfun::nan_t<T>() : (i == j ? s : T(2) * s);
                }
            }
        }
    }
};

// the generalised eigenvalues, ascending (DIST == false), or the squared distance / the distance (DIST == true)
template <typename T, int N, bool DIST>
struct PencilEigOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>;
    using RB = Rec<1, K>;
    using RC = NoRec;
    using RO = Rec<1, (DIST ? 1 : N)>;
    using Params = EigParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RO::C) * (int)sizeof(T) + 48);
    static constexpr bool kNoTile = PencilFunOp<T, N>::kNoTile;
    static __device__ __forceinline__ void apply(const T (&ra)[RA::Cs], const T (&rb)[RB::Cs], const T (&)[1],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        T mu[N];
        bool bad;
        if constexpr (N == 1) {
            mu[0] = rb[0] / ra[0];
            bad = !sympencil::scalar_ok(ra[0], rb[0]);
        } else {
            T w[N][N], lam[N], c[N][N], up[N][N];
            bad = sympencil::whiten<T, N>(ra, rb, w, lam, c);
            qr::eig_sym1<T, N, false, true>(c, w, up, mu, N, spectral::kMaxIter, spectral::kTol);
        }
        if constexpr (DIST) {
            T d2 = T(0);
#pragma unroll
            for (int k = 0; k < N; ++k) {
                bad |= !(symfun::finite_t(mu[k]) && mu[k] > T(0));
                const T l = symfun::log_t(bad ? T(1) : mu[k]);
                d2 = qr::fma_t(l, l, d2);
            }
            const T r = q.mode == sympencil::MODE_DIST ? symfun::sqrt_t(d2) : d2;
            o[0] = bad ? symfun::nan_t<T>() : r;
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) bad |= !symfun::finite_t(mu[k]);
            sympencil::sort_up<T, N>(mu);
#pragma unroll
            for (int k = 0; k < N; ++k) o[k] = bad ? symfun::nan_t<T>() : mu[k];
        }
    }
};

// both gradients of the squared distance (or of the distance) for its cotangent: one record of 2 K values, with
// respect to A then with respect to B, -c X diag(2 log mu) X^T and c X diag(2 log mu / mu) X^T
template <typename T, int N>
struct PencilDistBwdOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>;
    using RB = Rec<1, K>;
    using RC = Rec<1, 1>; // the cotangent
    using RO = Rec<1, 2 * K>;
    using Params = EigParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RC::C + RO::C) * (int)sizeof(T) + 64);
    static constexpr bool kNoTile = PencilFunOp<T, N>::kNoTile;
    static __device__ __forceinline__ void apply(const T (&ra)[RA::Cs], const T (&rb)[RB::Cs], const T (&g)[RC::Cs],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        T x[N][N], mu[N];
        bool bad;
        if constexpr (N == 1) {
            bad = !sympencil::scalar_ok(ra[0], rb[0]);
            mu[0] = rb[0] / ra[0];
            x[0][0] = T(1) / symfun::sqrt_t(bad ? T(1) : ra[0]);
        } else {
            T lam[N], qq[N][N];
            {
                T c[N][N], up[N][N];
                bad = sympencil::whiten<T, N>(ra, rb, x, lam, c);
                qr::eig_sym1<T, N, true, true>(c, qq, up, mu, N, spectral::kMaxIter, spectral::kTol);
            }
            sympencil::times_q<T, N, false>(x, lam, qq); // X = W Q
        }
        T fa[N], fb[N], d2 = T(0);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            bad |= !(symfun::finite_t(mu[k]) && mu[k] > T(0));
            const T m = bad ? T(1) : mu[k];
            const T l = symfun::log_t(m);
            d2 = qr::fma_t(l, l, d2);
            fa[k] = T(-2) * l;
            fb[k] = T(2) * l / m;
        }
        T coef = g[0];
        if (q.mode == sympencil::MODE_DIST) { // d d / d (d^2) = 1 / (2 d); 0 at d = 0 (a subgradient)
            const T d = symfun::sqrt_t(d2);
            coef = d > T(0) ? g[0] / (T(2) * d) : T(0);
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            fa[k] *= coef;
            fb[k] *= coef;
        }
        bad |= !symfun::finite_t(g[0]);
        spectral::recompose<T, N, 2>(x, fa, bad, &o[0]);
        spectral::recompose<T, N, 2>(x, fb, bad, &o[K]);
    }
};

// one launcher per part: (M, mode, base, mat, cotangent or NULL, out)
struct PencilArgs {
    FunParams fun;
    EigParams eig;
};
#define NFM_SYMPENCIL_ARGS                                                                                             \
    int M, const nfm_operand *a, const nfm_operand *b, const nfm_operand *g, const nfm_operand *o, int64_t no,          \
        int64_t ni, const PencilArgs &q, void *stream
template <int PART>
int sympencil_part(NFM_SYMPENCIL_ARGS);

#if NFM_SYMPENCIL_PART >= 1
template <>
int sympencil_part<NFM_SYMPENCIL_PART>(NFM_SYMPENCIL_ARGS)
{
    constexpr int part = NFM_SYMPENCIL_PART - 1;
    constexpr bool F64 = part / 16 != 0;
    constexpr int OP = (part / 4) % 4;
    constexpr int N0 = 2 * (part % 4) + 1;
    using T = std::conditional_t<F64, double, float>;
    auto run = [&](auto n) -> int {
        constexpr int N = decltype(n)::value;
        if constexpr (sympencil_fits(F64, OP, N)) {
            if constexpr (OP == 0) return rec_launch<T, PencilFunOp<T, N>>(a, b, nullptr, o, no, ni, q.fun, stream);
            else if constexpr (OP == 1) return rec_launch<T, PencilFunBwdOp<T, N>>(a, b, g, o, no, ni, q.fun, stream);
            else if constexpr (OP == 2) {
                if (q.eig.mode == sympencil::MODE_EIG)
                    return rec_launch<T, PencilEigOp<T, N, false>>(a, b, nullptr, o, no, ni, q.eig, stream);
                return rec_launch<T, PencilEigOp<T, N, true>>(a, b, nullptr, o, no, ni, q.eig, stream);
            } else return rec_launch<T, PencilDistBwdOp<T, N>>(a, b, g, o, no, ni, q.eig, stream);
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

#if NFM_SYMPENCIL_PART == 0
using namespace nfm;

static int sympencil_dispatch(int dtype, int M, int op, const nfm_operand *a, const nfm_operand *b, const nfm_operand *g,
                              const nfm_operand *o, int64_t no, int64_t ni, const PencilArgs &q, void *stream)
{
    const int part = (dtype == NFM_F64 ? 16 : 0) + op * 4 + (M - 1) / 2;
    return switch_order<32>(part + 1, NFM_ESIZE, [&](auto p) {
        constexpr int P = p;
        return sympencil_part<P>(M, a, b, g, o, no, ni, q, stream);
    });
}

// the checks of nfm_sym_funm in its order: the batch, the function code, the cap, p finite (then the operands)
static int pencil_fun_check(int dtype, int M, int fn, double p, int has_min, int op, int64_t n_outer, int64_t n_inner)
{
    const int rc = check_batch(dtype, n_outer, n_inner, {M});
    if (rc) return rc;
    return symfun::check_fun(false, fn, p, has_min, 0.0, sympencil_fits(dtype == NFM_F64, op, M)); // no clamp
}

static int pencil_eig_check(int dtype, int M, int mode, bool dist_only, int op, int64_t n_outer, int64_t n_inner)
{
    const int rc = check_batch(dtype, n_outer, n_inner, {M});
    if (rc) return rc;
    if (mode < (dist_only ? sympencil::MODE_DIST2 : sympencil::MODE_EIG) || mode > sympencil::MODE_DIST)
        return NFM_EINVAL;
    if (!sympencil_fits(dtype == NFM_F64, op, M)) return NFM_ESIZE;
    return NFM_OK;
}

extern "C" {

int nfm_sym_pencil_funm(int dtype, int M, int fn, double p, int has_min, double vmin, int64_t n_outer, int64_t n_inner,
                        const nfm_operand *base, const nfm_operand *mat, const nfm_operand *out, void *stream)
{
    int rc = pencil_fun_check(dtype, M, fn, p, has_min, 0, n_outer, n_inner);
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {base, mat, out}))) return rc;
    const PencilArgs q{FunParams{fn, 0, p, 0.0}, EigParams{0}};
    return sympencil_dispatch(dtype, M, 0, base, mat, nullptr, out, n_outer, n_inner, q, stream);
}

int nfm_sym_pencil_funm_backward(int dtype, int M, int fn, double p, int has_min, double vmin, int64_t n_outer,
                                 int64_t n_inner, const nfm_operand *base, const nfm_operand *mat,
                                 const nfm_operand *gout, const nfm_operand *gmat, void *stream)
{
    int rc = pencil_fun_check(dtype, M, fn, p, has_min, 1, n_outer, n_inner);
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {base, mat, gout, gmat}))) return rc;
    const PencilArgs q{FunParams{fn, 0, p, 0.0}, EigParams{0}};
    return sympencil_dispatch(dtype, M, 1, base, mat, gout, gmat, n_outer, n_inner, q, stream);
}

int nfm_sym_pencil_eig(int dtype, int M, int mode, int64_t n_outer, int64_t n_inner, const nfm_operand *base,
                       const nfm_operand *mat, const nfm_operand *out, void *stream)
{
    int rc = pencil_eig_check(dtype, M, mode, false, 2, n_outer, n_inner);
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {base, mat, out}))) return rc;
    const PencilArgs q{FunParams{0, 0, 0.0, 0.0}, EigParams{mode}};
    return sympencil_dispatch(dtype, M, 2, base, mat, nullptr, out, n_outer, n_inner, q, stream);
}

int nfm_sym_pencil_dist_backward(int dtype, int M, int mode, int64_t n_outer, int64_t n_inner, const nfm_operand *base,
                                 const nfm_operand *mat, const nfm_operand *gout, const nfm_operand *grads, void *stream)
{
    int rc = pencil_eig_check(dtype, M, mode, true, 3, n_outer, n_inner);
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {base, mat, gout, grads}))) return rc;
    const PencilArgs q{FunParams{0, 0, 0.0, 0.0}, EigParams{mode}};
    return sympencil_dispatch(dtype, M, 3, base, mat, gout, grads, n_outer, n_inner, q, stream);
}

int nfm_sym_pencil_max_order(int dtype, int op)
{
    if ((dtype != NFM_F32 && dtype != NFM_F64) || op < 0 || op > 3) return 0;
    return kSymPencilCap[dtype == NFM_F64 ? 1 : 0][op];
}

} // extern "C"
#endif
