// nfm_solve_entry.hpp -- the host code that the entry points of the solve families of `sugar` share
// (nfm_sugar.hip, nfm_svd.hip, nfm_lstsq.hip): their C arguments are flat -- a pointer and four strides per
// matrix --, so every entry point builds its nfm_operands, answers the same column-cap query, and ends its
// prologue with the same checks of the right-hand side; the host entries walk strided records.  Host code only.
#pragma once
#include "nfm_common.hpp"

namespace nfm {

inline nfm_operand flat_operand(const void *ptr, int64_t so, int64_t si, int64_t sr, int64_t sc)
{
    return {const_cast<void *>(ptr), so, si, sr, sc};
}

// the answer of a `*_max_cols` entry: `cap`, the family's table at `dims`, or the code of a bad dtype, then of a
// dimension outside 1..max_dim
inline int max_cols_answer(int dtype, std::initializer_list<int> dims, int max_dim, int cap)
{
    const int rc = check_batch(dtype, 1, 1, dims, max_dim);
    return rc ? rc : cap;
}

// The end of a solve entry's prologue, after check_batch and the family's own checks (flags, rcond, rows): the
// optional right-hand side, the column cap, the operands, the empty batch -- in this order, which is part of the
// ABI.  `identity_k` is the K of a call without B (B is then the identity), 0 for a family that requires B.
struct SolveRhs {
    int rc;               // the entry's answer when there is nothing to launch
    bool launch;
    const nfm_operand *b; // nullptr: the identity
};

inline SolveRhs check_rhs(int dtype, int64_t n_outer, int64_t n_inner, int K, int cap, int identity_k,
                          const nfm_operand &oa, const nfm_operand &ob, const nfm_operand &oo)
{
    const bool empty = n_outer == 0 || n_inner == 0;
    // (an empty batch carries null pointers throughout: B is then taken as present)
    const bool identity = identity_k > 0 && ob.ptr == nullptr && !empty;
    if (identity && K != identity_k) return {NFM_EINVAL, false, nullptr};
    if (!identity && K > cap) return {NFM_ESIZE, false, nullptr};
    const int rc = check_operands(dtype, n_outer, n_inner, {&oa, {&ob, !identity}, &oo});
    if (rc || empty) return {rc, false, nullptr};
    return {NFM_OK, true, identity ? nullptr : &ob};
}

// the rows x cols matrix of record (o, i) of a host operand, to and from a dense row-major array
template <typename T>
inline void host_gather(const nfm_operand *op, int64_t o, int64_t i, int rows, int cols, T *dst)
{
    const T *p = static_cast<const T *>(op->ptr) + o * op->stride_outer + i * op->stride_inner;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) dst[r * cols + c] = p[r * op->stride_row + c * op->stride_col];
}

template <typename T>
inline void host_scatter(const nfm_operand *op, int64_t o, int64_t i, int rows, int cols, const T *src)
{
    T *p = static_cast<T *>(op->ptr) + o * op->stride_outer + i * op->stride_inner;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) p[r * op->stride_row + c * op->stride_col] = src[r * cols + c];
}

} // namespace nfm
