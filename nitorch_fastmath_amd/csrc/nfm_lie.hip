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
    return switch_order<8>(D, NFM_ESIZE, [&](auto d) {
        // float64 8x8 (128 + 8 doubles live) spills to scratch in its component-major variant: torch route
        if constexpr (d() <= (sizeof(T) == 4 ? 8 : 7))
            return rec_launch<T, ExpmOp<T, d()>>(x, nullptr, nullptr, out, no, ni, p, stream);
        else
            return (int)NFM_ESIZE;
    });
}

template <typename T>
static int lie_frechet_t(int D, const LieParams &p, int64_t no, int64_t ni, const nfm_operand *x,
                         const nfm_operand *a, const nfm_operand *b, const nfm_operand *out, void *stream)
{
    return switch_order<4>(D, NFM_ESIZE, [&](auto d) {
        return b ? rec_launch<T, ExpmFrechetOp<T, d(), 2>>(x, a, b, out, no, ni, p, stream)
                 : rec_launch<T, ExpmFrechetOp<T, d(), 1>>(x, a, nullptr, out, no, ni, p, stream);
    });
}

// (max_order takes any value: < 2 keeps the first-order term only, like the reference)
static int lie_check(int dtype, int D, double tol, int64_t no, int64_t ni)
{
    const int rc = check_batch(dtype, no, ni, {D});
    if (rc) return rc;
    return tol >= 0.0 ? NFM_OK : NFM_EINVAL; // NaN or negative
}

} // namespace nfm

using namespace nfm;

extern "C" {

int nfm_lie_expm(int dtype, int D, int max_order, double tol, int64_t n_outer, int64_t n_inner,
                 const nfm_operand *x, const nfm_operand *out, void *stream)
{
    int rc = lie_check(dtype, D, tol, n_outer, n_inner);
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {x, out}))) return rc;
    const LieParams p{max_order, 0, tol};
    return by_dtype(dtype, [&](auto t) {
        return lie_expm_t<decltype(t)>(D, p, n_outer, n_inner, x, out, stream);
    });
}

int nfm_lie_expm_frechet(int dtype, int D, int max_order, double tol, int64_t n_outer, int64_t n_inner,
                         const nfm_operand *x, const nfm_operand *a, const nfm_operand *b,
                         const nfm_operand *out, void *stream)
{
    int rc = lie_check(dtype, D, tol, n_outer, n_inner);
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {x, a, {b, b != nullptr}, out}))) return rc;
    const LieParams p{max_order, 0, tol};
    return by_dtype(dtype, [&](auto t) {
        return lie_frechet_t<decltype(t)>(D, p, n_outer, n_inner, x, a, b, out, stream);
    });
}

} // extern "C"
