// nfm_sugar.hip -- A X = B for one small general or positive definite matrix per lane and a matrix of right-hand
// sides (reference `sugar.py`: lmdiv / rmdiv / solvevec / inv).  Without NFM_SUGAR_PART: the entry point
// nfm_sugar_solve.  With -DNFM_SUGAR_PART=0..15: one object per (dtype, method, pair of orders), so that the
// (N, K) grid of fully unrolled eliminations builds in parallel:
// PART = dtype * 8 + method * 4 + pair; pair q holds the orders 2q + 1 and 2q + 2, every K = 1..sugar_max_k.
#include "nfm_sugar_ops.hpp"
#include "nfm_solve_entry.hpp"

namespace nfm {

#define NFM_SUGAR_ARGS                                                                                             \
    int N, int K, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *b, const nfm_operand *out,      \
        void *stream
template <int PART>
int sugar_part(NFM_SUGAR_ARGS);

#ifdef NFM_SUGAR_PART

#if NFM_SUGAR_PART < 8
using TS = float;
#else
using TS = double;
#endif
constexpr bool kChol = (NFM_SUGAR_PART / 4) % 2 == 1;
constexpr int kPair = NFM_SUGAR_PART % 4;

// b == nullptr: the identity (Cholesky only; the entry point sends the pivoted inverse to nfm_batch_inv)
template <int N>
static int sugar_order(int K, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *b,
                       const nfm_operand *out, void *stream)
{
    SugarParams p{0};
    if constexpr (kChol) {
        if (b == nullptr) return rec_launch<TS, CholInvOp<TS, N>>(a, nullptr, nullptr, out, no, ni, p, stream);
    }
    return switch_order<kSugarMaxDim>(K, NFM_ESIZE, [&](auto k) {
        constexpr int Kc = k;
        if constexpr (Kc > sugar_max_k(sizeof(TS) == 8, N)) return (int)NFM_ESIZE;
        else if constexpr (kChol) return rec_launch<TS, SolveCholOp<TS, N, Kc>>(a, b, nullptr, out, no, ni, p, stream);
        else return rec_launch<TS, SolveLuOp<TS, N, Kc>>(a, b, nullptr, out, no, ni, p, stream);
    });
}

template <>
int sugar_part<NFM_SUGAR_PART>(NFM_SUGAR_ARGS)
{
    if (N == 2 * kPair + 1) return sugar_order<2 * kPair + 1>(K, no, ni, a, b, out, stream);
    return sugar_order<2 * kPair + 2>(K, no, ni, a, b, out, stream);
}

#endif // NFM_SUGAR_PART

} // namespace nfm

#ifndef NFM_SUGAR_PART

using namespace nfm;

extern "C" {

int nfm_sugar_max_cols(int dtype, int N)
{
    return max_cols_answer(dtype, {N}, kSugarMaxDim, sugar_max_k(dtype == NFM_F64, N));
}

int nfm_sugar_solve(int dtype, int N, int K, int flags, int64_t n_outer, int64_t n_inner,
                    const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                    const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                    void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc, void *stream)
{
    const int rc = check_batch(dtype, n_outer, n_inner, {N, K}, kSugarMaxDim);
    if (rc) return rc;
    if (flags != NFM_SOLVE_LU && flags != NFM_SOLVE_CHOL) return NFM_EINVAL;
    const nfm_operand oa = flat_operand(a, a_so, a_si, a_sr, a_sc), ob = flat_operand(b, b_so, b_si, b_sr, b_sc),
                      oo = flat_operand(out, o_so, o_si, o_sr, o_sc);
    const SolveRhs rhs = check_rhs(dtype, n_outer, n_inner, K, sugar_max_k(dtype == NFM_F64, N), N, oa, ob, oo);
    if (!rhs.launch) return rhs.rc;
    if (rhs.b == nullptr && flags == NFM_SOLVE_LU) return nfm_batch_inv(dtype, N, 0, n_outer, n_inner, &oa, &oo, stream);
    const int part = (dtype == NFM_F64 ? 8 : 0) + (flags == NFM_SOLVE_CHOL ? 4 : 0) + ((N - 1) >> 1);
    return switch_order<16>(part + 1, NFM_ESIZE, [&](auto p) {
        constexpr int P = p;
        return sugar_part<P - 1>(N, K, n_outer, n_inner, &oa, rhs.b, &oo, stream);
    });
}

} // extern "C"

#endif
