// nfm_logm.hip -- principal matrix logarithm, logm(M^-1 A) and the Frechet derivative of the
// logarithm, one matrix per lane (reference `_impl/logm.py`, `lie.py:13-93`).  The ops are in
// nfm_logm_ops.hpp; every layout mode of the record kernel comes with rec_launch.
//   logm, logm_solve:  float32 orders 1..NFM_LOGM_MAX_F32, float64 orders 1..NFM_LOGM_MAX_F64
//   logm_frechet:      orders 1..NFM_LOGM_FRECHET_MAX, both dtypes
// Every other order answers NFM_ESIZE: the facade takes its torch route there.
#include "nfm_logm_ops.hpp"

// the largest orders that compile without scratch memory
#define NFM_LOGM_MAX_F32 8
#define NFM_LOGM_MAX_F64 7
#define NFM_LOGM_FRECHET_MAX 5

namespace nfm {

template <typename T>
constexpr int logm_max()
{
    return sizeof(T) == 4 ? NFM_LOGM_MAX_F32 : NFM_LOGM_MAX_F64;
}

template <typename T, int D>
static int logm_one(const nfm_operand *m, const nfm_operand *a, const nfm_operand *out, int64_t no, int64_t ni,
                    void *stream)
{
    const LogmParams p{};
    if constexpr (D <= logm_max<T>()) {
        if (m) return rec_launch<T, LogmSolveOp<T, D>>(m, a, nullptr, out, no, ni, p, stream);
        return rec_launch<T, LogmOp<T, D>>(a, nullptr, nullptr, out, no, ni, p, stream);
    } else {
        return NFM_ESIZE;
    }
}

template <typename T>
static int logm_t(int D, const nfm_operand *m, const nfm_operand *a, const nfm_operand *out, int64_t no,
                  int64_t ni, void *stream)
{
    static_assert(NFM_LOGM_MAX_F32 >= NFM_LOGM_MAX_F64, "the switch runs to the larger of the two limits");
    return switch_order<NFM_LOGM_MAX_F32>(D, NFM_ESIZE, [&](auto d) { return logm_one<T, d()>(m, a, out, no, ni, stream); });
}

template <typename T>
static int logm_frechet_t(int D, const nfm_operand *x, const nfm_operand *g, const nfm_operand *out, int64_t no,
                          int64_t ni, void *stream)
{
    const LogmParams p{};
    return switch_order<NFM_LOGM_FRECHET_MAX>(D, NFM_ESIZE, [&](auto d) {
        return rec_launch<T, LogmFrechetOp<T, d()>>(x, g, nullptr, out, no, ni, p, stream);
    });
}

} // namespace nfm

using namespace nfm;

extern "C" {

int nfm_lie_logm(int dtype, int D, int64_t n_outer, int64_t n_inner, const nfm_operand *x, const nfm_operand *out,
                 void *stream)
{
    int rc = check_batch(dtype, n_outer, n_inner, {D});
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {x, out}))) return rc;
    return by_dtype(dtype, [&](auto t) {
        return logm_t<decltype(t)>(D, nullptr, x, out, n_outer, n_inner, stream);
    });
}

int nfm_lie_logm_solve(int dtype, int D, int64_t n_outer, int64_t n_inner, const nfm_operand *m,
                       const nfm_operand *a, const nfm_operand *out, void *stream)
{
    int rc = check_batch(dtype, n_outer, n_inner, {D});
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {m, a, out}))) return rc;
    return by_dtype(dtype, [&](auto t) {
        return logm_t<decltype(t)>(D, m, a, out, n_outer, n_inner, stream);
    });
}

int nfm_lie_logm_frechet(int dtype, int D, int64_t n_outer, int64_t n_inner, const nfm_operand *x,
                         const nfm_operand *g, const nfm_operand *out, void *stream)
{
    int rc = check_batch(dtype, n_outer, n_inner, {D});
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {x, g, out}))) return rc;
    return by_dtype(dtype, [&](auto t) {
        return logm_frechet_t<decltype(t)>(D, x, g, out, n_outer, n_inner, stream);
    });
}

} // extern "C"
