// nfm_batched.hip -- general small matrices: batchinv / batchdet / batchmatvec
// (reference `_impl/batched.py`).  One matrix per lane; N <= 3 use the reference's
// adjugate closed forms, 4 <= N <= 8 Gauss-Jordan / LU with partial pivoting in
// registers, N > 8 the chains of batch_inv_t / batch_det_t.
#include "nfm_batched_ops.hpp"
#include "nfm_big.hpp"
#include "nfm_rowwave.hpp"
#include "nfm_spd.hpp"

namespace nfm {

// Orders 9..16: contiguous row-major matrices go to the diagonal-pivots-first kernels of nfm_spd.hip (float32
// 9..16, float64 9..13: gen_fits), which hand the wavefronts that need a row exchange to the pivoted elimination;
// float64 14..16 do not fit a lane there and take one matrix per 16 lanes (nfm_rowwave.hip).  Any other layout:
// the LDS-resident kernels of nfm_big.hpp.
template <typename T>
static int batch_inv_t(int N, int flags, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *out,
                       void *stream)
{
    if (N > 8) {
        if (no == 1) {
            int rc = Spd<T>::batch_inv(N, ni, a, out, stream);
            if (rc == NFM_EFALLBACK) rc = RowWave<T>::batch_inv(N, ni, a, out, stream);
            if (rc != NFM_EFALLBACK) return rc;
        }
        return big_batch_inv<T>(N, no, ni, a, out, stream);
    }
    InvParams p{(flags & NFM_FLAG_TS_PERTURB) ? 1 : 0};
    return switch_order<8>(N, NFM_ESIZE, [&](auto n) {
        return rec_launch<T, BatchInvOp<T, n()>>(a, nullptr, nullptr, out, no, ni, p, stream);
    });
}

// orders 9..16: as batch_inv_t
template <typename T>
static int batch_det_t(int N, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *out, void *stream)
{
    if (N > 8) {
        if (no == 1) {
            int rc = Spd<T>::batch_det(N, ni, a, out, stream);
            if (rc == NFM_EFALLBACK) rc = RowWave<T>::batch_det(N, ni, a, out, stream);
            if (rc != NFM_EFALLBACK) return rc;
        }
        return big_batch_det<T>(N, no, ni, a, out, stream);
    }
    NoParamsB p{0};
    return switch_order<8>(N, NFM_ESIZE, [&](auto n) {
        return rec_launch<T, BatchDetOp<T, n()>>(a, nullptr, nullptr, out, no, ni, p, stream);
    });
}

template <typename T>
static int batch_matvec_t(int R, int C, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *v,
                          const nfm_operand *out, void *stream)
{
    NoParamsB p{0};
#define NFM_MV(Rv, Cv) \
    if (R == Rv && C == Cv) return (rec_launch<T, BatchMatvecOp<T, Rv, Cv>>(a, v, nullptr, out, no, ni, p, stream));
    NFM_MV(1, 1) NFM_MV(2, 2) NFM_MV(3, 3) NFM_MV(4, 4) NFM_MV(5, 5) NFM_MV(6, 6) NFM_MV(7, 7) NFM_MV(8, 8)
    NFM_MV(2, 3) NFM_MV(3, 2) NFM_MV(3, 4) NFM_MV(4, 3) NFM_MV(4, 5) NFM_MV(5, 4)
#undef NFM_MV
    return big_batch_matvec<T>(R, C, no, ni, a, v, out, stream);
}

} // namespace nfm

using namespace nfm;

extern "C" {

int nfm_batch_inv(int dtype, int N, int flags, int64_t n_outer, int64_t n_inner, const nfm_operand *a,
                  const nfm_operand *out, void *stream)
{
    int rc = check_batch(dtype, n_outer, n_inner, {N});
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {a, out}))) return rc;
    return by_dtype(dtype, [&](auto t) {
        return batch_inv_t<decltype(t)>(N, flags, n_outer, n_inner, a, out, stream);
    });
}

int nfm_batch_det(int dtype, int N, int64_t n_outer, int64_t n_inner, const nfm_operand *a, const nfm_operand *out,
                  void *stream)
{
    int rc = check_batch(dtype, n_outer, n_inner, {N});
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {a, out}))) return rc;
    return by_dtype(dtype, [&](auto t) {
        return batch_det_t<decltype(t)>(N, n_outer, n_inner, a, out, stream);
    });
}

int nfm_batch_matvec(int dtype, int rows, int cols, int64_t n_outer, int64_t n_inner, const nfm_operand *a,
                     const nfm_operand *v, const nfm_operand *out, void *stream)
{
    int rc = check_batch(dtype, n_outer, n_inner, {rows, cols});
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {a, v, out}))) return rc;
    return by_dtype(dtype, [&](auto t) {
        return batch_matvec_t<decltype(t)>(rows, cols, n_outer, n_inner, a, v, out, stream);
    });
}

} // extern "C"
