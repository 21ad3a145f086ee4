// nfm_sugar.hip -- A X = B for one small general or positive definite matrix per lane and a matrix of right-hand
// sides (reference `sugar.py`: lmdiv / rmdiv / solvevec / inv).  Without NFM_SUGAR_PART: the entry point
// nfm_sugar_solve.  With -DNFM_SUGAR_PART=0..15: one object per (dtype, method, pair of orders), so that the
// (N, K) grid of fully unrolled eliminations builds in parallel:
// PART = dtype * 8 + method * 4 + pair; pair q holds the orders 2q + 1 and 2q + 2, every K = 1..sugar_max_k.
#include "nfm_sugar_ops.hpp"

namespace nfm {

#define NFM_SUGAR_ARGS                                                                                             \
    int N, int K, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *b, const nfm_operand *out,      \
        void *stream
#define NFM_SUGAR_DECL(T, M)                                                             \
    int sugar_##T##_##M##_q0(NFM_SUGAR_ARGS); int sugar_##T##_##M##_q1(NFM_SUGAR_ARGS); \
    int sugar_##T##_##M##_q2(NFM_SUGAR_ARGS); int sugar_##T##_##M##_q3(NFM_SUGAR_ARGS);
NFM_SUGAR_DECL(f32, lu) NFM_SUGAR_DECL(f32, chol) NFM_SUGAR_DECL(f64, lu) NFM_SUGAR_DECL(f64, chol)
#undef NFM_SUGAR_DECL

#ifdef NFM_SUGAR_PART

#define NFM_SF64 (NFM_SUGAR_PART / 8)
#define NFM_SCHOL ((NFM_SUGAR_PART / 4) % 2)
#if NFM_SUGAR_PART % 4 == 0
#define NFM_SQ 0
#elif NFM_SUGAR_PART % 4 == 1
#define NFM_SQ 1
#elif NFM_SUGAR_PART % 4 == 2
#define NFM_SQ 2
#else
#define NFM_SQ 3
#endif
#if NFM_SF64 == 0
using TS = float;
#define NFM_ST f32
#else
using TS = double;
#define NFM_ST f64
#endif
#if NFM_SCHOL == 0
#define NFM_SM lu
#else
#define NFM_SM chol
#endif
#define NFM_SNAME3(t, m, q) sugar_##t##_##m##_q##q
#define NFM_SNAME2(t, m, q) NFM_SNAME3(t, m, q)
#define NFM_SNAME NFM_SNAME2(NFM_ST, NFM_SM, NFM_SQ)

// b == nullptr: the identity (Cholesky only; the entry point sends the pivoted inverse to nfm_batch_inv)
template <int N>
static int sugar_order(int K, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *b,
                       const nfm_operand *out, void *stream)
{
    SugarParams p{0};
#if NFM_SCHOL == 1
    if (b == nullptr) return rec_launch<TS, CholInvOp<TS, N>>(a, nullptr, nullptr, out, no, ni, p, stream);
#endif
    return switch_order<kSugarMaxDim>(K, NFM_ESIZE, [&](auto k) {
        constexpr int Kc = k;
        if constexpr (Kc > sugar_max_k(sizeof(TS) == 8, N)) return (int)NFM_ESIZE;
#if NFM_SCHOL == 1
        else return rec_launch<TS, SolveCholOp<TS, N, Kc>>(a, b, nullptr, out, no, ni, p, stream);
#else
        else return rec_launch<TS, SolveLuOp<TS, N, Kc>>(a, b, nullptr, out, no, ni, p, stream);
#endif
    });
}

int NFM_SNAME(NFM_SUGAR_ARGS)
{
    if (N == 2 * NFM_SQ + 1) return sugar_order<2 * NFM_SQ + 1>(K, no, ni, a, b, out, stream);
    return sugar_order<2 * NFM_SQ + 2>(K, no, ni, a, b, out, stream);
}

#endif // NFM_SUGAR_PART

} // namespace nfm

#ifndef NFM_SUGAR_PART

using namespace nfm;

extern "C" {

int nfm_sugar_max_cols(int dtype, int N)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (N < 1 || N > kSugarMaxDim) return NFM_ESIZE;
    return sugar_max_k(dtype == NFM_F64, N);
}

int nfm_sugar_solve(int dtype, int N, int K, int flags, int64_t n_outer, int64_t n_inner,
                    const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                    const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                    void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc, void *stream)
{
    int rc = check_batch(dtype, n_outer, n_inner, {N, K}, kSugarMaxDim);
    if (rc) return rc;
    if (flags != NFM_SOLVE_LU && flags != NFM_SOLVE_CHOL) return NFM_EINVAL;
    const bool empty = n_outer == 0 || n_inner == 0;
    // (an empty batch carries null pointers throughout: B is then taken as present)
    const bool identity = b == nullptr && !empty;
    if (identity && K != N) return NFM_EINVAL;
    if (!identity && K > sugar_max_k(dtype == NFM_F64, N)) return NFM_ESIZE;
    const nfm_operand oa = {const_cast<void *>(a), a_so, a_si, a_sr, a_sc};
    const nfm_operand ob = {const_cast<void *>(b), b_so, b_si, b_sr, b_sc};
    const nfm_operand oo = {out, o_so, o_si, o_sr, o_sc};
    if ((rc = check_operands(dtype, n_outer, n_inner, {&oa, {&ob, !identity}, &oo}))) return rc;
    if (empty) return NFM_OK;
    if (identity && flags == NFM_SOLVE_LU) return nfm_batch_inv(dtype, N, 0, n_outer, n_inner, &oa, &oo, stream);
    const nfm_operand *pb = identity ? nullptr : &ob;
    const int q = (N - 1) >> 1;
#define NFM_SUGAR_CALL(T, M)                                                              \
    switch (q) {                                                                          \
    case 0: return sugar_##T##_##M##_q0(N, K, n_outer, n_inner, &oa, pb, &oo, stream);    \
    case 1: return sugar_##T##_##M##_q1(N, K, n_outer, n_inner, &oa, pb, &oo, stream);    \
    case 2: return sugar_##T##_##M##_q2(N, K, n_outer, n_inner, &oa, pb, &oo, stream);    \
    default: return sugar_##T##_##M##_q3(N, K, n_outer, n_inner, &oa, pb, &oo, stream);   \
    }
    if (dtype == NFM_F32) {
        if (flags == NFM_SOLVE_LU) { NFM_SUGAR_CALL(f32, lu) }
        NFM_SUGAR_CALL(f32, chol)
    }
    if (flags == NFM_SOLVE_LU) { NFM_SUGAR_CALL(f64, lu) }
    NFM_SUGAR_CALL(f64, chol)
#undef NFM_SUGAR_CALL
}

} // extern "C"

#endif
