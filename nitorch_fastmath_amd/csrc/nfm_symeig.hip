// nfm_symeig.hip -- sorted eigendecomposition of compact symmetric matrices (sym_eigvals / sym_eigh and their
// gradient; an extension of `sym`, no counterpart in the reference).  One record per lane through rec_kernel, as
// nfm_symfun.hip: read the K = N (N + 1) / 2 compact values, expand them (spectral::expand: the bad-record rule),
// decompose in registers with the FAST sweeps of eig_sym1 (which scale: every finite record is in range), then sort
// the eigenpairs into the requested order and fix the eigenvectors' signs (nfm_symeig_ops.hpp).  The two backward
// kernels recompute the decomposition from the saved input -- the same code, so the same order and signs -- and
// evaluate S = V W V^T with W_kk = gl_k and W_kl = (B_kl - B_lk) / (2 (l_l - l_k)), B = V^T gV, under the gap rule of
// nfm_symeig_ops.hpp; the result is S_ii and 2 S_ij, the module's compact convention.
// The order is a run-time member of Params (a wave-uniform choice of the key): the instantiations are
// (dtype, N, op) x the layout kinds of rec_launch.
#include "nfm_record_kernel.hpp"
#include "nfm_spectral.hpp"
#include "nfm_symeig_ops.hpp"

// This file is compiled 33 times (-DNFM_SYMEIG_PART=0..32).  Part 0: the entry points, the caps and the CPU routine.
// Parts 1..32: the kernels of one (dtype, op, pair of orders): part = 1 + dtype * 16 + op * 4 + pair, op =
// NFM_EIGH_OP_*, pair p = orders 2p + 1 and 2p + 2.  Each of them defines its own specialisation of
// symeig_part<PART>; part 0 reaches them through switch_order<32>.
#ifndef NFM_SYMEIG_PART
#error "compile with -DNFM_SYMEIG_PART=0..32"
#endif

namespace nfm {

using symeig::OrderParams;

// The compiled caps: the largest order of each (dtype, op) whose kernels have no private segment in any layout form
// (profiles/symeig_table.md lists the registers of every instantiation).  Orders above take the caller's own route.
// (the float64 full backward at 8 x 8 holds u, the 64 values of the vectors' cotangent and W at once: every form of
// it needs 364 bytes of scratch per lane, so the order is left to the caller's route)
constexpr int kSymEigCap[2][4] = {{8, 8, 8, 8}, {8, 8, 8, 7}}; // [dtype][NFM_EIGH_OP_*]
constexpr bool symeig_fits(bool f64, int op, int N) { return N >= 1 && N <= kSymEigCap[f64 ? 1 : 0][op]; }

// the sorted, sign-fixed decomposition of one record; true for a bad record (u, lam: those of the identity)
template <typename T, int N, bool WITH_U>
__device__ __forceinline__ bool symeig_decompose(const T (&r)[sym_k(N)], int order, T (&lam)[N],
                                                 T (&u)[WITH_U ? N : 1][WITH_U ? N : 1])
{
    bool bad;
    if constexpr (WITH_U) {
        T a[N][N], up[N][N];
        bad = spectral::expand<T, N>(r, a);
        qr::eig_sym1<T, N, true, true>(a, u, up, lam, N, spectral::kMaxIter, spectral::kTol);
    } else {
        T a[N][N], w[N][N], up[N][N]; // w and up are never touched without U
        bad = spectral::expand<T, N>(r, a);
        qr::eig_sym1<T, N, false, true>(a, w, up, lam, N, spectral::kMaxIter, spectral::kTol);
    }
    symeig::sort_pairs<T, N, WITH_U>(order, lam, u);
    if constexpr (WITH_U) symeig::fix_signs<T, N>(u);
    return bad;
}

// values (N), or the packed record [values | vectors, row-major] as EigSymOp packs it
template <typename T, int N, bool WITH_U>
struct SymEigOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>;
    using RB = NoRec;
    using RC = NoRec;
    using RO = Rec<1, N + (WITH_U ? N * N : 0)>;
    using Params = OrderParams;
    static constexpr int TILE = pick_tile((RA::C + RO::C) * (int)sizeof(T) + 32);
    // as SymFunOp: from these orders on the kernel is bound by its dependent arithmetic and an LDS image of a
    // wavefront's records would only cost occupancy
    static constexpr bool kNoTile = N >= 5 || (N == 4 && sizeof(T) == 8);
    static __device__ __forceinline__ void apply(const T (&r)[RA::Cs], const T (&)[1], const T (&)[1],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        if constexpr (N == 1) {
            const bool bad = !symfun::finite_t(r[0]);
            o[0] = bad ? symfun::nan_t<T>() : r[0];
            if constexpr (WITH_U) o[1] = bad ? symfun::nan_t<T>() : T(1);
        } else {
            T lam[N], u[WITH_U ? N : 1][WITH_U ? N : 1];
            const bool bad = symeig_decompose<T, N, WITH_U>(r, q.order, lam, u);
#pragma unroll
            for (int k = 0; k < N; ++k) o[k] = bad ? symfun::nan_t<T>() : lam[k];
            if constexpr (WITH_U) {
#pragma unroll
                for (int i = 0; i < N; ++i)
#pragma unroll
                    for (int j = 0; j < N; ++j) o[N + i * N + j] = bad ? symfun::nan_t<T>() : u[i][j];
            }
        }
    }
};

// gradient for a cotangent of the values alone: V diag(gl) V^T
template <typename T, int N>
struct SymEigValBwdOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>; // compact A
    using RB = Rec<1, N>; // cotangent of the values
    using RC = NoRec;
    using RO = Rec<1, K>; // compact gradient
    using Params = OrderParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RO::C) * (int)sizeof(T) + 48);
    static constexpr bool kNoTile = SymEigOp<T, N, true>::kNoTile;
    static __device__ __forceinline__ void apply(const T (&r)[RA::Cs], const T (&g)[RB::Cs], const T (&)[1],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        if constexpr (N == 1) {
            o[0] = symfun::finite_t(r[0]) ? g[0] : symfun::nan_t<T>();
        } else {
            T lam[N], u[N][N];
            const bool bad = symeig_decompose<T, N, true>(r, q.order, lam, u);
            spectral::recompose<T, N, 2>(u, g, bad, &o[0]);
        }
    }
};

// gradient for cotangents of the values and of the vectors
template <typename T, int N>
struct SymEigBwdOp {
    static constexpr int K = sym_k(N);
    using RA = Rec<1, K>;     // compact A
    using RB = Rec<1, N>;     // cotangent of the values (absent: a stride-0 record of zeros)
    using RC = Rec<1, N * N>; // cotangent of the vectors, row-major
    using RO = Rec<1, K>;     // compact gradient
    using Params = OrderParams;
    static constexpr int TILE = pick_tile((RA::C + RB::C + RC::C + RO::C) * (int)sizeof(T) + 64);
    static constexpr bool kNoTile = SymEigOp<T, N, true>::kNoTile;
    static __device__ __forceinline__ void apply(const T (&r)[RA::Cs], const T (&gl)[RB::Cs], const T (&gv)[RC::Cs],
                                                 T (&o)[RO::Cs], const Params &q)
    {
        if constexpr (N == 1) {
            o[0] = symfun::finite_t(r[0]) ? gl[0] : symfun::nan_t<T>(); // a unit vector has no tangent
        } else {
            T lam[N], u[N][N];
            const bool bad = symeig_decompose<T, N, true>(r, q.order, lam, u);
            const T tol = symeig::gap_tol<T, N>(lam);
            // W (symmetric, compact): W_kk = gl_k; W_kl = (B_kl - B_lk) / 2 x the gap weight, B = V^T gV
            T w[K];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                w[k] = gl[k];
#pragma unroll
                for (int l = k + 1; l < N; ++l) {
                    T bkl = u[0][k] * gv[l], blk = u[0][l] * gv[k];
#pragma unroll
                    for (int i = 1; i < N; ++i) {
                        bkl = qr::fma_t(u[i][k], gv[i * N + l], bkl);
                        blk = qr::fma_t(u[i][l], gv[i * N + k], blk);
                    }
                    w[sym_idx(N, k, l)] = T(0.5) * (bkl - blk) * symeig::gap_weight(lam[k], lam[l], tol);
                }
            }
            // S = V W V^T, i <= j: column j of W V^T, then row i <= j; compact result S_ii, 2 S_ij (the third step of
            // SymFunBwdOp in nfm_symfun.hip)
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

// one launcher per part: (M, mat, gval or NULL, gvec or NULL, out)
#define NFM_SYMEIG_ARGS                                                                                                \
    int M, const nfm_operand *a, const nfm_operand *gl, const nfm_operand *gv, const nfm_operand *o, int64_t no,        \
        int64_t ni, const OrderParams &q, void *stream
template <int PART>
int symeig_part(NFM_SYMEIG_ARGS);

#if NFM_SYMEIG_PART >= 1
template <>
int symeig_part<NFM_SYMEIG_PART>(NFM_SYMEIG_ARGS)
{
    constexpr int part = NFM_SYMEIG_PART - 1;
    constexpr bool F64 = part / 16 != 0;
    constexpr int OP = (part / 4) % 4;
    constexpr int N0 = 2 * (part % 4) + 1;
    using T = std::conditional_t<F64, double, float>;
    auto run = [&](auto n) -> int {
        constexpr int N = decltype(n)::value;
        if constexpr (symeig_fits(F64, OP, N)) {
            if constexpr (OP == NFM_EIGH_OP_VALUES)
                return rec_launch<T, SymEigOp<T, N, false>>(a, nullptr, nullptr, o, no, ni, q, stream);
            else if constexpr (OP == NFM_EIGH_OP_VECTORS)
                return rec_launch<T, SymEigOp<T, N, true>>(a, nullptr, nullptr, o, no, ni, q, stream);
            else if constexpr (OP == NFM_EIGH_OP_VALUES_BACKWARD)
                return rec_launch<T, SymEigValBwdOp<T, N>>(a, gl, nullptr, o, no, ni, q, stream);
            else return rec_launch<T, SymEigBwdOp<T, N>>(a, gl, gv, o, no, ni, q, stream);
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

#if NFM_SYMEIG_PART == 0
using namespace nfm;

// the checks of nfm_sym_funm in its order: the batch, the order code, the cap (then the operands)
static int symeig_check(int dtype, int M, int flags, int op, int64_t n_outer, int64_t n_inner)
{
    const int rc = check_batch(dtype, n_outer, n_inner, {M});
    if (rc) return rc;
    if (flags < 0 || (flags & ~(3 | NFM_EIGH_VECTORS)) || !symeig::order_ok(flags & 3)) return NFM_EINVAL;
    if (!symeig_fits(dtype == NFM_F64, op, M)) return NFM_ESIZE;
    return NFM_OK;
}

static int symeig_dispatch(int dtype, int M, int op, const nfm_operand *a, const nfm_operand *gl, const nfm_operand *gv,
                           const nfm_operand *o, int64_t no, int64_t ni, const OrderParams &q, void *stream)
{
    const int part = (dtype == NFM_F64 ? 16 : 0) + op * 4 + (M - 1) / 2;
    return switch_order<32>(part + 1, NFM_ESIZE, [&](auto p) {
        constexpr int P = p;
        return symeig_part<P>(M, a, gl, gv, o, no, ni, q, stream);
    });
}

// one host record: sort, sign rule and gap weights
template <typename T, int N>
static void symeig_host_finish_n(int order, int64_t n, T *lam, T *vec, T *w)
{
    for (int64_t b = 0; b < n; ++b) {
        T l[N], u[N][N];
        for (int k = 0; k < N; ++k) l[k] = lam[b * N + k];
        if (vec) {
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j) u[i][j] = vec[(b * N + i) * N + j];
            symeig::sort_pairs<T, N, true>(order, l, u);
            symeig::fix_signs<T, N>(u);
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j) vec[(b * N + i) * N + j] = u[i][j];
        } else {
            T none[1][1];
            symeig::sort_pairs<T, N, false>(order, l, none);
        }
        for (int k = 0; k < N; ++k) lam[b * N + k] = l[k];
        if (w) {
            const T tol = symeig::gap_tol<T, N>(l);
            for (int k = 0; k < N; ++k)
                for (int j = 0; j < N; ++j) w[(b * N + k) * N + j] = k == j ? T(0) : symeig::gap_weight(l[k], l[j], tol);
        }
    }
}

template <typename T>
static int symeig_host_finish_t(int order, int N, int64_t n, void *lam, void *vec, void *w)
{
    return switch_order<8>(N, NFM_ESIZE, [&](auto nn) {
        constexpr int NN = nn;
        symeig_host_finish_n<T, NN>(order, n, static_cast<T *>(lam), static_cast<T *>(vec), static_cast<T *>(w));
        return (int)NFM_OK;
    });
}

extern "C" {

int nfm_sym_eigh(int dtype, int M, int flags, int64_t n_outer, int64_t n_inner, const nfm_operand *mat,
                 const nfm_operand *out, void *stream)
{
    const int op = (flags >= 0 && (flags & NFM_EIGH_VECTORS)) ? NFM_EIGH_OP_VECTORS : NFM_EIGH_OP_VALUES;
    int rc = symeig_check(dtype, M, flags, op, n_outer, n_inner);
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {mat, out}))) return rc;
    return symeig_dispatch(dtype, M, op, mat, nullptr, nullptr, out, n_outer, n_inner, OrderParams{flags & 3}, stream);
}

int nfm_sym_eigh_backward(int dtype, int M, int flags, int64_t n_outer, int64_t n_inner, const nfm_operand *mat,
                          const nfm_operand *gval, const nfm_operand *gvec, const nfm_operand *gmat, void *stream)
{
    const int op = gvec ? NFM_EIGH_OP_BACKWARD : NFM_EIGH_OP_VALUES_BACKWARD;
    int rc = symeig_check(dtype, M, flags, op, n_outer, n_inner);
    if (rc) return rc;
    if (gvec) rc = check_operands(dtype, n_outer, n_inner, {mat, gval, gvec, gmat});
    else rc = check_operands(dtype, n_outer, n_inner, {mat, gval, gmat});
    if (rc) return rc;
    return symeig_dispatch(dtype, M, op, mat, gval, gvec, gmat, n_outer, n_inner, OrderParams{flags & 3}, stream);
}

int nfm_sym_eigh_max_order(int dtype, int op)
{
    if ((dtype != NFM_F32 && dtype != NFM_F64) || op < 0 || op > 3) return 0;
    return kSymEigCap[dtype == NFM_F64 ? 1 : 0][op];
}

int nfm_sym_eigh_host_finish(int dtype, int order, int N, int64_t n, void *lam, void *vec, void *w)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (n < 0 || !symeig::order_ok(order)) return NFM_EINVAL;
    if (N < 1 || N > 8) return NFM_ESIZE;
    if (n > 0 && lam == nullptr) return NFM_EINVAL;
    return dtype == NFM_F32 ? symeig_host_finish_t<float>(order, N, n, lam, vec, w)
                            : symeig_host_finish_t<double>(order, N, n, lam, vec, w);
}

} // extern "C"
#endif
