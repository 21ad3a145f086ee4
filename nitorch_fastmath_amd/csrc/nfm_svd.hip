// nfm_svd.hip -- X = A^+ B for one small M x N matrix per lane and a matrix of right-hand sides, by a one-sided
// Jacobi SVD (reference `sugar.py`: lmdiv / rmdiv / solvevec / inv with method 'svd' / 'pinv', and every
// non-square system).  Without NFM_SVD_PART: the entry points nfm_svd_solve, nfm_svd_solve_host and
// nfm_svd_max_cols.  With -DNFM_SVD_PART=0..31: one object per (dtype, M, half of the N), so that the (M, N, K)
// grid of fully unrolled sweeps builds in parallel:
// PART = dtype * 16 + (M - 1) * 2 + half; half h holds N = 4h + 1 .. 4h + 4, every K = 1..svd_max_k.
#include "nfm_svd_ops.hpp"
#include "nfm_solve_entry.hpp"

namespace nfm {

// host != 0: the records are in host memory and are solved one after the other on the calling thread (same
// routine, same arithmetic); the return value is then the largest number of sweeps a record took
#define NFM_SVD_ARGS                                                                                               \
    int N, int K, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *b, const nfm_operand *out,      \
        const SvdParams &prm, int host, void *stream
template <int PART>
int svd_part(NFM_SVD_ARGS);

#ifdef NFM_SVD_PART

#if NFM_SVD_PART < 16
using TS = float;
#else
using TS = double;
#endif
constexpr int kM = (NFM_SVD_PART % 16) / 2 + 1;
constexpr int kHalf = NFM_SVD_PART % 2;

template <typename T, int M, int N, int K, bool IDENT>
static int svd_host_loop(int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *b, const nfm_operand *out,
                         const SvdParams &prm)
{
    int most = 0;
    for (int64_t o = 0; o < no; ++o)
        for (int64_t i = 0; i < ni; ++i) {
            T ra[M * N], rb[M * K], ro[N * K];
            host_gather<T>(a, o, i, M, N, ra);
            if constexpr (!IDENT) host_gather<T>(b, o, i, M, K, rb);
            const int sweeps = svd_solve_flat<T, M, N, K, IDENT>(ra, rb, ro, prm);
            most = sweeps > most ? sweeps : most;
            host_scatter<T>(out, o, i, N, K, ro);
        }
    return most;
}

// b == nullptr: the identity (K == M, checked by the entry point)
template <int N>
static int svd_order(int K, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *b,
                     const nfm_operand *out, const SvdParams &prm, int host, void *stream)
{
    if (b == nullptr) {
        if (host) return svd_host_loop<TS, kM, N, kM, true>(no, ni, a, nullptr, out, prm);
        return rec_launch<TS, SvdInvOp<TS, kM, N>>(a, nullptr, nullptr, out, no, ni, prm, stream);
    }
    return switch_order<kSvdMaxDim>(K, NFM_ESIZE, [&](auto k) {
        constexpr int Kc = k;
        if constexpr (Kc > svd_max_k(sizeof(TS) == 8, kM, N)) return (int)NFM_ESIZE;
        else {
            if (host) return svd_host_loop<TS, kM, N, Kc, false>(no, ni, a, b, out, prm);
            return rec_launch<TS, SvdSolveOp<TS, kM, N, Kc>>(a, b, nullptr, out, no, ni, prm, stream);
        }
    });
}

template <>
int svd_part<NFM_SVD_PART>(NFM_SVD_ARGS)
{
    switch (N - 4 * kHalf) {
    case 1: return svd_order<4 * kHalf + 1>(K, no, ni, a, b, out, prm, host, stream);
    case 2: return svd_order<4 * kHalf + 2>(K, no, ni, a, b, out, prm, host, stream);
    case 3: return svd_order<4 * kHalf + 3>(K, no, ni, a, b, out, prm, host, stream);
    default: return svd_order<4 * kHalf + 4>(K, no, ni, a, b, out, prm, host, stream);
    }
}

#endif // NFM_SVD_PART

} // namespace nfm

#ifndef NFM_SVD_PART

using namespace nfm;

static int svd_entry(int dtype, int M, int N, int K, int flags, double rcond, int64_t n_outer, int64_t n_inner,
                     const nfm_operand &oa, const nfm_operand &ob, const nfm_operand &oo, int host, void *stream)
{
    const int rc = check_batch(dtype, n_outer, n_inner, {M, N, K}, kSvdMaxDim);
    if (rc) return rc;
    if (flags != NFM_SVD_PLAIN && flags != NFM_SVD_PINV) return NFM_EINVAL;
    if (!(rcond >= 0.0)) return NFM_EINVAL;
    const SolveRhs rhs = check_rhs(dtype, n_outer, n_inner, K, svd_max_k(dtype == NFM_F64, M, N), M, oa, ob, oo);
    if (!rhs.launch) return rhs.rc;
    const SvdParams prm{flags == NFM_SVD_PINV, rcond};
    const int part = (dtype == NFM_F64 ? 16 : 0) + (M - 1) * 2 + (N > 4);
    return switch_order<32>(part + 1, NFM_ESIZE, [&](auto p) {
        constexpr int P = p;
        return svd_part<P - 1>(N, K, n_outer, n_inner, &oa, rhs.b, &oo, prm, host, stream);
    });
}

extern "C" {

int nfm_svd_max_cols(int dtype, int M, int N)
{
    return max_cols_answer(dtype, {M, N}, kSvdMaxDim, svd_max_k(dtype == NFM_F64, M, N));
}

int nfm_svd_solve(int dtype, int M, int N, int K, int flags, double rcond, int64_t n_outer, int64_t n_inner,
                  const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                  const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                  void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc, void *stream)
{
    return svd_entry(dtype, M, N, K, flags, rcond, n_outer, n_inner, flat_operand(a, a_so, a_si, a_sr, a_sc),
                     flat_operand(b, b_so, b_si, b_sr, b_sc), flat_operand(out, o_so, o_si, o_sr, o_sc), 0, stream);
}

int nfm_svd_solve_host(int dtype, int M, int N, int K, int flags, double rcond, int64_t n_outer, int64_t n_inner,
                       const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                       const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                       void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc)
{
    return svd_entry(dtype, M, N, K, flags, rcond, n_outer, n_inner, flat_operand(a, a_so, a_si, a_sr, a_sc),
                     flat_operand(b, b_so, b_si, b_sr, b_sc), flat_operand(out, o_so, o_si, o_sr, o_sc), 1, nullptr);
}

} // extern "C"

#endif
