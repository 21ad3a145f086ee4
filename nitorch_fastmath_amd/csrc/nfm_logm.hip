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
#define NFM_LOGM(Dv) \
    case Dv: return logm_one<T, Dv>(m, a, out, no, ni, stream);
    switch (D) {
        NFM_LOGM(1) NFM_LOGM(2) NFM_LOGM(3) NFM_LOGM(4) NFM_LOGM(5) NFM_LOGM(6) NFM_LOGM(7) NFM_LOGM(8)
    default: break;
    }
#undef NFM_LOGM
    return NFM_ESIZE;
}

template <typename T>
static int logm_frechet_t(int D, const nfm_operand *x, const nfm_operand *g, const nfm_operand *out, int64_t no,
                          int64_t ni, void *stream)
{
    const LogmParams p{};
#define NFM_LOGMF(Dv) \
    case Dv: return rec_launch<T, LogmFrechetOp<T, Dv>>(x, g, nullptr, out, no, ni, p, stream);
    switch (D) {
        NFM_LOGMF(1) NFM_LOGMF(2) NFM_LOGMF(3) NFM_LOGMF(4) NFM_LOGMF(5)
    default: break;
    }
#undef NFM_LOGMF
    static_assert(NFM_LOGM_FRECHET_MAX == 5, "the switch above lists the orders");
    return NFM_ESIZE;
}

static int logm_check(int dtype, int D, int64_t no, int64_t ni)
{
    int rc = check_common(dtype, no, ni);
    if (rc) return rc;
    if (D < 1 || D > NFM_MAX_DIM) return NFM_ESIZE;
    return NFM_OK;
}

} // namespace nfm

using namespace nfm;

extern "C" {

int nfm_lie_logm(int dtype, int D, int64_t n_outer, int64_t n_inner, const nfm_operand *x, const nfm_operand *out,
                 void *stream)
{
    int rc = logm_check(dtype, D, n_outer, n_inner);
    if (rc) return rc;
    const bool nonempty = n_outer > 0 && n_inner > 0;
    if ((rc = check_operand(x, dtype, nonempty))) return rc;
    if ((rc = check_operand(out, dtype, nonempty))) return rc;
    return dtype == NFM_F32 ? logm_t<float>(D, nullptr, x, out, n_outer, n_inner, stream)
                            : logm_t<double>(D, nullptr, x, out, n_outer, n_inner, stream);
}

int nfm_lie_logm_solve(int dtype, int D, int64_t n_outer, int64_t n_inner, const nfm_operand *m,
                       const nfm_operand *a, const nfm_operand *out, void *stream)
{
    int rc = logm_check(dtype, D, n_outer, n_inner);
    if (rc) return rc;
    const bool nonempty = n_outer > 0 && n_inner > 0;
    if ((rc = check_operand(m, dtype, nonempty))) return rc;
    if ((rc = check_operand(a, dtype, nonempty))) return rc;
    if ((rc = check_operand(out, dtype, nonempty))) return rc;
    return dtype == NFM_F32 ? logm_t<float>(D, m, a, out, n_outer, n_inner, stream)
                            : logm_t<double>(D, m, a, out, n_outer, n_inner, stream);
}

int nfm_lie_logm_frechet(int dtype, int D, int64_t n_outer, int64_t n_inner, const nfm_operand *x,
                         const nfm_operand *g, const nfm_operand *out, void *stream)
{
    int rc = logm_check(dtype, D, n_outer, n_inner);
    if (rc) return rc;
    const bool nonempty = n_outer > 0 && n_inner > 0;
    if ((rc = check_operand(x, dtype, nonempty))) return rc;
    if ((rc = check_operand(g, dtype, nonempty))) return rc;
    if ((rc = check_operand(out, dtype, nonempty))) return rc;
    return dtype == NFM_F32 ? logm_frechet_t<float>(D, x, g, out, n_outer, n_inner, stream)
                            : logm_frechet_t<double>(D, x, g, out, n_outer, n_inner, stream);
}

} // extern "C"
