// nfm_lie.hip -- matrix exponential and its Frechet derivatives, one matrix per lane
// (reference `_impl/expm.py`).  The ops are in nfm_lie_ops.hpp; every layout mode of the
// record kernel (tiled, packed, transposed, strided, broadcast) comes with rec_launch.
//   expm:     float32 orders 1..8, float64 orders 1..7
//   frechet:  orders 1..4, both dtypes, first (L) and second (L2) derivative
// Every other order answers NFM_ESIZE: the facade takes its torch route there.
#include "nfm_lie_ops.hpp"

namespace nfm {

template <typename T>
static int lie_expm_t(int D, const LieParams &p, int64_t no, int64_t ni, const nfm_operand *x,
                      const nfm_operand *out, void *stream)
{
#define NFM_EXPM(Dv) \
    case Dv: return rec_launch<T, ExpmOp<T, Dv>>(x, nullptr, nullptr, out, no, ni, p, stream);
    switch (D) {
        NFM_EXPM(1) NFM_EXPM(2) NFM_EXPM(3) NFM_EXPM(4) NFM_EXPM(5) NFM_EXPM(6) NFM_EXPM(7)
    default: break;
    }
    // float64 8x8 (128 + 8 doubles live) spills to scratch in its component-major variant: torch route
    if constexpr (sizeof(T) == 4) {
        if (D == 8) return rec_launch<T, ExpmOp<T, 8>>(x, nullptr, nullptr, out, no, ni, p, stream);
    }
#undef NFM_EXPM
    return NFM_ESIZE;
}

template <typename T>
static int lie_frechet_t(int D, const LieParams &p, int64_t no, int64_t ni, const nfm_operand *x,
                         const nfm_operand *a, const nfm_operand *b, const nfm_operand *out, void *stream)
{
#define NFM_FRECHET(Dv)                                                                                      \
    case Dv:                                                                                                 \
        return b ? rec_launch<T, ExpmFrechetOp<T, Dv, 2>>(x, a, b, out, no, ni, p, stream)                  \
                 : rec_launch<T, ExpmFrechetOp<T, Dv, 1>>(x, a, nullptr, out, no, ni, p, stream);
    switch (D) {
        NFM_FRECHET(1) NFM_FRECHET(2) NFM_FRECHET(3) NFM_FRECHET(4)
    default: break;
    }
#undef NFM_FRECHET
    return NFM_ESIZE;
}

static int lie_check(int dtype, int D, int max_order, double tol, int64_t no, int64_t ni)
{
    int rc = check_common(dtype, no, ni);
    if (rc) return rc;
    if (D < 1 || D > NFM_MAX_DIM) return NFM_ESIZE;
    if (!(tol >= 0.0)) return NFM_EINVAL; // NaN or negative
    (void)max_order;                      // any value: < 2 keeps the first-order term only, like the reference
    return NFM_OK;
}

} // namespace nfm

using namespace nfm;

extern "C" {

int nfm_lie_expm(int dtype, int D, int max_order, double tol, int64_t n_outer, int64_t n_inner,
                 const nfm_operand *x, const nfm_operand *out, void *stream)
{
    int rc = lie_check(dtype, D, max_order, tol, n_outer, n_inner);
    if (rc) return rc;
    const bool nonempty = n_outer > 0 && n_inner > 0;
    if ((rc = check_operand(x, dtype, nonempty))) return rc;
    if ((rc = check_operand(out, dtype, nonempty))) return rc;
    const LieParams p{max_order, 0, tol};
    return dtype == NFM_F32 ? lie_expm_t<float>(D, p, n_outer, n_inner, x, out, stream)
                            : lie_expm_t<double>(D, p, n_outer, n_inner, x, out, stream);
}

int nfm_lie_expm_frechet(int dtype, int D, int max_order, double tol, int64_t n_outer, int64_t n_inner,
                         const nfm_operand *x, const nfm_operand *a, const nfm_operand *b,
                         const nfm_operand *out, void *stream)
{
    int rc = lie_check(dtype, D, max_order, tol, n_outer, n_inner);
    if (rc) return rc;
    const bool nonempty = n_outer > 0 && n_inner > 0;
    if ((rc = check_operand(x, dtype, nonempty))) return rc;
    if ((rc = check_operand(a, dtype, nonempty))) return rc;
    if (b && (rc = check_operand(b, dtype, nonempty))) return rc;
    if ((rc = check_operand(out, dtype, nonempty))) return rc;
    const LieParams p{max_order, 0, tol};
    return dtype == NFM_F32 ? lie_frechet_t<float>(D, p, n_outer, n_inner, x, a, b, out, stream)
                            : lie_frechet_t<double>(D, p, n_outer, n_inner, x, a, b, out, stream);
}

} // extern "C"
