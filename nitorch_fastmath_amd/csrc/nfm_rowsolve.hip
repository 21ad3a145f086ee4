// nfm_rowsolve.hip -- A X = B for one general or positive definite matrix of order 9..16 per 16 / R lanes and up
// to 8 right-hand sides (reference `sugar.py`: lmdiv / rmdiv / solvevec / inv at the orders past the lane-per-system
// kernels of nfm_sugar.hip).  A lane holds R rows of the augmented matrix [A | B]:
//   'lu'  : Gauss-Jordan with partial pivoting, the first unused row with the largest key pivots (roww_tile's
//           search); the pivot row stays where it is and reaches the other lanes by ds_bpermute or through a
//           per-matrix LDS slot of N + KB values; the lane slot that pivoted at step k ends with row k of X over its
//           pivot.  A zero pivot gives inf / NaN in that record only.
//   'chol': the same elimination without the search (step k pivots on row k), on the matrix rebuilt from the lower
//           triangle; a pivot that is not > 0 (NaN included) makes every value of that record's X NaN.
// The multiply-adds are written out (fma_) and the objects are built with -ffp-contract=off: column j of X has the
// same bits whatever K, whatever width KB it ran at and whichever layout kind moved it.
// Without NFM_ROWSOLVE_PART: the entry points nfm_rowsolve and nfm_rowsolve_max_cols.  With
// -DNFM_ROWSOLVE_PART=0..15: one object per (dtype, N), both methods, the widths 1 / 2 / 4 / 8 and the two layout
// kinds, in the one form of rowsolve_choice: PART = dtype * 8 + N - 9.
#include "nfm_rowsolve_core.hpp"
#include "nfm_solve_entry.hpp"

namespace nfm {

#define NFM_ROWSOLVE_ARGS                                                                                          \
    int K, int chol, int col0, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *b,                 \
        const nfm_operand *out, void *stream
template <int PART>
int rowsolve_part(NFM_ROWSOLVE_ARGS);

#ifdef NFM_ROWSOLVE_PART

#if NFM_ROWSOLVE_PART < 8
using TS = float;
#else
using TS = double;
#endif
constexpr int kN = NFM_ROWSOLVE_PART % 8 + rows::kRowsolveMinDim;

// records of rows x cols elements back to back, row-major, one batch level (the stride of an extent of one is not
// looked at)
static bool rowsolve_dense(const nfm_operand *op, int nrows, int cols, int64_t ni)
{
    if (ni > 1 && op->stride_inner != (int64_t)nrows * cols) return false;
    if (op->stride_row != cols) return false;
    return cols == 1 || op->stride_col == 1;
}

template <int KB, bool CHOL>
static int rowsolve_launch(int K, int col0, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *b,
                           const nfm_operand *out, void *stream)
{
    constexpr rows::RsChoice c = rows::rowsolve_choice(sizeof(TS) == 8, kN);
    static_assert(c.rows == 1 || c.rows == 2 || c.rows == 4, "rows per lane");
    static_assert(rows::lds_elems<TS, kN, KB, c.lds>() * sizeof(TS) <= 64 * 1024, "the tile fits the static LDS limit");
    const int64_t nblk = (ni + rows::MPB - 1) / rows::MPB;
    if (nblk > 0x7fffffffLL) return NFM_ESIZE;
    const bool dense = no == 1 && rowsolve_dense(a, kN, kN, ni) && (b == nullptr || rowsolve_dense(b, kN, K, ni)) &&
                       rowsolve_dense(out, kN, K, ni);
    const Opnd da = make_opnd(a, 0), dout = make_opnd(out, 0);
    const Opnd db = b ? make_opnd(b, 0) : Opnd{nullptr, 0, 0, 0, 0, 0};
    const dim3 grid((unsigned)nblk, (unsigned)no, 1), block(256 / c.rows, 1, 1);
    if (dense)
        hipLaunchKernelGGL((rows::rowsolve_kernel<TS, kN, KB, CHOL, c.rows, c.lds, false>), grid, block, 0,
                           static_cast<hipStream_t>(stream), da, db, dout, ni, K, col0, b != nullptr);
    else
        hipLaunchKernelGGL((rows::rowsolve_kernel<TS, kN, KB, CHOL, c.rows, c.lds, true>), grid, block, 0,
                           static_cast<hipStream_t>(stream), da, db, dout, ni, K, col0, b != nullptr);
    return launch_status();
}

template <>
int rowsolve_part<NFM_ROWSOLVE_PART>(NFM_ROWSOLVE_ARGS)
{
    auto width = [&](auto kb) {
        constexpr int KB = kb;
        return chol ? rowsolve_launch<KB, true>(K, col0, no, ni, a, b, out, stream)
                    : rowsolve_launch<KB, false>(K, col0, no, ni, a, b, out, stream);
    };
    switch (rows::rowsolve_width(K)) {
    case 1: return width(std::integral_constant<int, 1>{});
    case 2: return width(std::integral_constant<int, 2>{});
    case 4: return width(std::integral_constant<int, 4>{});
    default: return width(std::integral_constant<int, 8>{});
    }
}

#endif // NFM_ROWSOLVE_PART

} // namespace nfm

#ifndef NFM_ROWSOLVE_PART

using namespace nfm;

static bool rowsolve_order(int N) { return N >= rows::kRowsolveMinDim && N <= NFM_MAX_DIM; }

extern "C" {

int nfm_rowsolve_max_cols(int dtype, int N)
{
    const int rc = max_cols_answer(dtype, {N}, NFM_MAX_DIM, rows::kRowsolveMaxCols);
    return rc < 0 || rowsolve_order(N) ? rc : (int)NFM_ESIZE;
}

int nfm_rowsolve(int dtype, int N, int K, int flags, int64_t n_outer, int64_t n_inner,
                 const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                 const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                 void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc, void *stream)
{
    const int rc = check_batch(dtype, n_outer, n_inner, {N, K}, NFM_MAX_DIM);
    if (rc) return rc;
    if (!rowsolve_order(N)) return NFM_ESIZE;
    if (flags != NFM_SOLVE_LU && flags != NFM_SOLVE_CHOL) return NFM_EINVAL;
    const nfm_operand oa = flat_operand(a, a_so, a_si, a_sr, a_sc), ob = flat_operand(b, b_so, b_si, b_sr, b_sc),
                      oo = flat_operand(out, o_so, o_si, o_sr, o_sc);
    const SolveRhs rhs = check_rhs(dtype, n_outer, n_inner, K, rows::kRowsolveMaxCols, N, oa, ob, oo);
    if (!rhs.launch) return rhs.rc;
    if (rhs.b == nullptr && flags == NFM_SOLVE_LU) return nfm_batch_inv(dtype, N, 0, n_outer, n_inner, &oa, &oo, stream);
    const int part = (dtype == NFM_F64 ? 8 : 0) + N - rows::kRowsolveMinDim;
    const int chol = flags == NFM_SOLVE_CHOL;
    auto run = [&](int k, int col0, const nfm_operand &o) {
        return switch_order<16>(part + 1, NFM_ESIZE, [&](auto p) {
            constexpr int P = p;
            return rowsolve_part<P - 1>(k, chol, col0, n_outer, n_inner, &oa, rhs.b, &o, stream);
        });
    };
    if (rhs.b != nullptr) return run(K, 0, oo);
    // the identity: one launch per block of columns, on offset views of out
    const size_t elem = dtype == NFM_F64 ? 8 : 4;
    for (int c0 = 0; c0 < N; c0 += rows::kRowsolveMaxCols) {
        nfm_operand o = oo;
        o.ptr = static_cast<char *>(oo.ptr) + (int64_t)c0 * oo.stride_col * (int64_t)elem;
        const int k = N - c0 < rows::kRowsolveMaxCols ? N - c0 : rows::kRowsolveMaxCols;
        const int r = run(k, c0, o);
        if (r) return r;
    }
    return NFM_OK;
}

} // extern "C"

#endif
