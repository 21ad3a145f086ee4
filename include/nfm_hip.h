/* nfm_hip.h -- C ABI of libnfm_hip.so, the MI355X (gfx950) backend for the
 * per-element small-matrix hot path of nitorch-fastmath.
 *
 * The reference has no FFI of its own for this path: its public functions are
 * plain Python (`nitorch_fastmath/sym.py:28-37`, `batched.py:16-17`,
 * `qr.py:1-11`, `reduce.py:38-41`) and the shipped `sym_*` implementation comes
 * from the external `jitfields.sym` module (`sym.py:37`).  This header is the
 * boundary a maintainer binds instead (ctypes stub in INTEGRATION.md): one
 * entry point per reference function family, plain pointers / sizes / strides,
 * no torch types.  Every entry point
 *   - launches asynchronously on the `hipStream_t` passed as `stream`
 *     (NULL = the default stream) on the CURRENT device, never synchronises,
 *     never allocates or frees memory (graph-capture safe);
 *   - returns 0 on success, a negative NFM_E* code for a rejected argument,
 *     or a positive hipError_t if the launch itself failed;
 *   - is reentrant and stateless.
 *
 * Batch model.  The facade flattens the broadcast batch shape to two levels,
 * n_outer x n_inner (n_outer == 1 for ordinary contiguous tensors; two levels
 * cover channel-first fields (B, C, *spatial) without a copy).  Strides are in
 * ELEMENTS; 0 = broadcast.  An operand is read as
 *     ptr[o * stride_outer + i * stride_inner + r * stride_row + c * stride_col]
 * with (r, c) the matrix row/column for full matrices and r = 0, c = component
 * for vectors and compact-symmetric storage.
 *
 * Compact symmetric layout (reference `sym.py:7-14`, `_impl/sym.py:21-27`):
 * K = M(M+1)/2 components, the diagonal first, then the strict upper triangle
 * row by row: [a00 a11 .. a(M-1)(M-1) | a01 a02 .. a0(M-1) a12 ..].
 */
#ifndef NFM_HIP_H
#define NFM_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFM_VERSION 5 /* 5: NFM_MAT_PIVOTED / NFM_INVERT_PIVOTED; 2: nfm_qr_eig_sym takes flags (NFM_EIG_*); nfm_reduce_median added; 3: nfm_reduce_median_mid;
                         4: nfm_qr_eig_sym flags: bit 2 is NFM_EIG_FAST (flags == with_u is the reference order again) */
#define NFM_MAX_DIM 16 /* largest matrix order handled (3x3 .. 16x16 and below) */

/* dtype codes */
#define NFM_F32 0
#define NFM_F64 1

/* error codes (negative) */
#define NFM_OK 0
#define NFM_EINVAL (-1)   /* null pointer / negative size / bad flag */
#define NFM_EDTYPE (-2)   /* unsupported dtype code */
#define NFM_ESIZE (-3)    /* matrix order outside 1..NFM_MAX_DIM, or batch too large */
#define NFM_EALIGN (-4)   /* pointer not aligned to the element size */
#define NFM_EWORKSPACE (-5) /* workspace too small */

/* `mat_kind` of the sym_* entry points: how the matrix operand's last dim of
 * length NN is interpreted, reference `sym.py:16-24`. */
#define NFM_MAT_SYM 0  /* NN = M(M+1)/2 compact symmetric */
#define NFM_MAT_DIAG 1 /* NN = M       diagonal           */
#define NFM_MAT_SCAL 2 /* NN = 1       scaled identity    */
#define NFM_MAT_FULL 3 /* NN = M*M     full, row-major via stride_row/stride_col */
/* flag, OR-ed into `mat_kind` of nfm_sym_solve (and bit 1 = value 2 of `diag_only` of nfm_sym_invert): orders 9..16 go
 * straight to the pivoted elimination, without the attempt that serves positive definite matrices -- for callers who
 * know their matrices are indefinite (a batch of those pays the attempt for nothing) */
#define NFM_MAT_PIVOTED 16
#define NFM_INVERT_DIAG 1
#define NFM_INVERT_PIVOTED 2

typedef struct nfm_operand {
    void *ptr;            /* device pointer */
    int64_t stride_outer; /* elements */
    int64_t stride_inner; /* elements */
    int64_t stride_row;   /* elements; full matrices only */
    int64_t stride_col;   /* elements; component stride for vectors / compact storage */
} nfm_operand;

/* ------------------------------------------------------------------ sym ---- */

/* x = mat \ vec.  Replaces `sym_solve` / `sym_solve_` (`sym.py:33`; in-repo
 * implementation `_impl/sym.py:327-398`).  M <= 4: the reference's closed forms,
 * evaluated in its operation order (bit-identical to its CPU path); M > 4: LU with
 * partial pivoting of the full matrix in registers / LDS, like the
 * `torch.linalg.solve` branch (`_impl/sym.py:392-396`); contiguous operands at
 * M = 9..16 (here, in nfm_sym_invert and in nfm_sym_det): the unpivoted LDL^T of the
 * compact record first, the pivoted elimination for every wavefront that holds a matrix
 * which is not positive definite -- same answers within rounding.  `eps` (NULL or M doubles on
 * the HOST) is added to the diagonal first (documented intent of `_impl/sym.py:356-357`).
 * `out` may alias `vec` (in-place variant). */
int nfm_sym_solve(int dtype, int M, int mat_kind, int64_t n_outer, int64_t n_inner,
                  const nfm_operand *mat, const nfm_operand *vec, const nfm_operand *out,
                  const double *eps, void *stream);

/* out = mat * vec            (mode  0)  `sym_matvec`        `_impl/sym.py:134-172`
 * out = inp + mat * vec      (mode +1)  `sym_addmatvec(_)`  `sym.py:31`
 * out = inp - mat * vec      (mode -1)  `sym_submatvec(_)`  `sym.py:32`
 * `inp` is ignored for mode 0; `out` may alias `inp`. */
int nfm_sym_matvec(int dtype, int M, int mat_kind, int mode, int64_t n_outer, int64_t n_inner,
                   const nfm_operand *mat, const nfm_operand *vec, const nfm_operand *inp,
                   const nfm_operand *out, void *stream);

/* out = compact inverse of a compact symmetric matrix (diag_only & NFM_INVERT_DIAG: its M
 * diagonal entries; diag_only & NFM_INVERT_PIVOTED: see NFM_MAT_PIVOTED).  Replaces
 * `sym_invert` / `sym_invert_` (`sym.py:34`, `_impl/sym.py:455-493`).  One factorisation per
 * matrix (the reference runs M full solves).  `out` may alias `mat` when the diagonal flag
 * is not set. */
int nfm_sym_invert(int dtype, int M, int diag_only, int64_t n_outer, int64_t n_inner,
                   const nfm_operand *mat, const nfm_operand *out, void *stream);

/* determinant of compact symmetric matrices, `sym_det` `_impl/sym.py:401-452` (quirk Q2
 * fixed: M comes from the compact dim).  out: one element per matrix (stride_col unused). */
int nfm_sym_det(int dtype, int M, int64_t n_outer, int64_t n_inner, const nfm_operand *mat,
                const nfm_operand *out, void *stream);

/* compact -> full (M x M), `sym_to_full` `_impl/sym.py:16-60`. */
int nfm_sym_to_full(int dtype, int M, int64_t n_outer, int64_t n_inner, const nfm_operand *mat,
                    const nfm_operand *out, void *stream);

/* compact x x^T of a vector, `sym_outer` `_impl/sym.py:496-528`. */
int nfm_sym_outer(int dtype, int M, int64_t n_outer, int64_t n_inner, const nfm_operand *x,
                  const nfm_operand *out, void *stream);

/* out_ii = x_i y_i, out_ij = x_i y_j + x_j y_i (i < j), negated when neg != 0: the pull-back
 * of the full-matrix cotangent x y^T onto compact storage.  No reference counterpart: it is
 * the building block of the backward passes of sym_matvec / sym_solve (autograd). */
int nfm_sym_outer2(int dtype, int M, int neg, int64_t n_outer, int64_t n_inner, const nfm_operand *x,
                   const nfm_operand *y, const nfm_operand *out, void *stream);

/* compact J^T H J, `sym_matmul` `_impl/sym.py:637-670`; jac is (K x D) full, hess compact
 * (hess_kind NFM_MAT_SYM) or diagonal (NFM_MAT_DIAG).  For K == D in {2, 3} the reference
 * evaluates J H J^T (quirk Q16, `jhj2`/`jhj3` `_impl/sym.py:540-597`); so does this. */
int nfm_sym_matmul(int dtype, int K, int D, int hess_kind, int64_t n_outer, int64_t n_inner,
                   const nfm_operand *jac, const nfm_operand *hess, const nfm_operand *out,
                   void *stream);

/* EXTENSION (no counterpart in the reference): x = (J^T H J)^-1 g in one kernel -- the
 * Gauss-Newton step its callers chain as `sym_solve(sym_matmul(jac, hess), grad, eps)`
 * (`_impl/sym.py:637-670` then `:327-398`), without the HBM round trip of the compact
 * (D x D) product.  Same arithmetic as the two calls: bit-identical results.  K, D in 1..4
 * (NFM_ESIZE otherwise: chain the two calls); eps as for nfm_sym_solve, length D. */
int nfm_sym_matmul_solve(int dtype, int K, int D, int hess_kind, int64_t n_outer, int64_t n_inner,
                         const nfm_operand *jac, const nfm_operand *hess, const nfm_operand *grad,
                         const nfm_operand *out, const double *eps, void *stream);

/* EXTENSION (no counterpart in the reference): spectral functions of compact symmetric matrices,
 * out = V f(max(L, vmin)) V^T for mat = V L V^T, compact in and compact out: one read of the M (M + 1) / 2 values, the
 * eigendecomposition in the lane's registers (the fast sweep arithmetic of nfm_qr_eig_sym, NFM_EIG_FAST), one write.
 * fn: NFM_FUN_*; p: the exponent of NFM_FUN_POW (ignored otherwise); has_min != 0 clamps the eigenvalues from below
 * at vmin before f (required by NFM_FUN_CLAMP, whose f is the identity).  Domains, judged after the clamp: EXP and
 * CLAMP any real eigenvalue; LOG, RSQRT, POW with p < 0: > 0; SQRT, POW with p >= 0: >= 0.  A record with an
 * eigenvalue outside the domain, or with an entry that is not finite, is NaN in every component; the other records
 * do not notice.  `out` may be `mat` (in place).
 * nfm_sym_funm_backward: gmat = the gradient with respect to the compact record, given the cotangent gout of the
 * compact result (Daleckii-Krein with closed-form divided differences; the decomposition is recomputed from mat).
 * Compact convention of the module: a compact off-diagonal component stands for both mirrored entries, so the full
 * symmetric cotangent is G_ii = g_ii, G_ij = g_ij / 2, and the result is S_ii on the diagonal and 2 S_ij off it,
 * S = V [(V^T G V) o F] V^T, F_kl = f[l_k, l_l].  `gmat` may be `gout`.
 * M in 1..nfm_sym_funm_max_order(dtype, backward).  Status precedence: NFM_EDTYPE; NFM_EINVAL negative count;
 * NFM_ESIZE n_outer; NFM_ESIZE M outside 1..NFM_MAX_DIM; NFM_EINVAL unknown fn; NFM_ESIZE M above the compiled
 * cap (the caller's own route: the Python facade runs torch.linalg.eigh there); NFM_EINVAL p or vmin not finite,
 * NFM_FUN_CLAMP without has_min; then the operands in argument order. */
#define NFM_FUN_EXP 0
#define NFM_FUN_LOG 1
#define NFM_FUN_SQRT 2
#define NFM_FUN_RSQRT 3
#define NFM_FUN_POW 4
#define NFM_FUN_CLAMP 5
int nfm_sym_funm(int dtype, int M, int fn, double p, int has_min, double vmin, int64_t n_outer, int64_t n_inner,
                 const nfm_operand *mat, const nfm_operand *out, void *stream);
int nfm_sym_funm_backward(int dtype, int M, int fn, double p, int has_min, double vmin, int64_t n_outer,
                          int64_t n_inner, const nfm_operand *mat, const nfm_operand *gout,
                          const nfm_operand *gmat, void *stream);
/* largest M with a kernel (backward != 0: of nfm_sym_funm_backward); 0 for an unknown dtype */
int nfm_sym_funm_max_order(int dtype, int backward);
/* CPU: the scalar formulas the kernels evaluate, for n eigenvalues lam of the dtype: f[i] = f(max(lam_i, vmin)) and
 * dd[i * n + j] = the first divided difference of f o max(., vmin) at (lam_i, lam_j); NaN where a clamped
 * eigenvalue is outside the domain.  NFM_EDTYPE / NFM_EINVAL as above (and for n < 0 or a null pointer with n > 0). */
int nfm_sym_funm_host_eval(int dtype, int fn, double p, int has_min, double vmin, int n, const void *lam, void *f,
                           void *dd);

/* EXTENSION (no counterpart in the reference): spectral kernels of a pencil (base, mat) of compact symmetric
 * matrices, base positive definite: with base = V L V^T, W = V L^-1/2, W^T mat W = Q M Q^T, X = W Q and Z = X^-T, both
 * decompositions in the lane's registers (the arithmetic of nfm_sym_funm), every record read once.
 * nfm_sym_pencil_funm: out = base^1/2 f(base^-1/2 mat base^-1/2) base^1/2 = Z f(M) Z^T, fn in NFM_FUN_EXP ..
 * NFM_FUN_POW (POW with exponent t: the point base #_t mat of the geodesic; LOG / EXP: the Riemannian log / exp map at
 * base); NFM_FUN_CLAMP and has_min != 0 are NFM_EINVAL.  `out` may be either input.
 * nfm_sym_pencil_funm_backward: gmat = the gradient with respect to `mat` for the cotangent gout of the compact
 * result, X [(Z^T G Z) o F] X^T, in the compact convention of nfm_sym_funm_backward.
 * nfm_sym_pencil_eig: mode NFM_PENCIL_EIG: the M generalised eigenvalues of mat x = mu base x, ascending;
 * NFM_PENCIL_DIST2: sum_i log^2 mu_i, the squared affine-invariant distance (one value); NFM_PENCIL_DIST: its root.
 * nfm_sym_pencil_dist_backward: mode NFM_PENCIL_DIST2 or NFM_PENCIL_DIST; gout = the cotangent of that value (one per
 * record); grads = records of 2 M (M + 1) / 2 values: the compact gradient with respect to base, then the one with
 * respect to mat, -c X diag(2 log mu) X^T and c X diag(2 log mu / mu) X^T (exact and zero at base == mat); for
 * NFM_PENCIL_DIST c = gout / (2 d), defined as 0 at d == 0 (a subgradient).
 * A record with an entry of base or mat that is not finite, a computed eigenvalue of base that is not positive, or
 * a mu outside the domain of f (the distance: mu <= 0) is NaN in every component; the other records do not notice.
 * M in 1..nfm_sym_pencil_max_order(dtype, op).  Status precedence: that of nfm_sym_funm (NFM_EINVAL for an unknown
 * fn or mode before NFM_ESIZE for M above the compiled cap, then NFM_EINVAL for p not finite, then the operands in
 * argument order). */
#define NFM_PENCIL_OP_FUNM 0
#define NFM_PENCIL_OP_FUNM_BACKWARD 1
#define NFM_PENCIL_OP_EIG 2
#define NFM_PENCIL_OP_DIST_BACKWARD 3
#define NFM_PENCIL_EIG 0
#define NFM_PENCIL_DIST2 1
#define NFM_PENCIL_DIST 2
int nfm_sym_pencil_funm(int dtype, int M, int fn, double p, int has_min, double vmin, int64_t n_outer,
                        int64_t n_inner, const nfm_operand *base, const nfm_operand *mat, const nfm_operand *out,
                        void *stream);
int nfm_sym_pencil_funm_backward(int dtype, int M, int fn, double p, int has_min, double vmin, int64_t n_outer,
                                 int64_t n_inner, const nfm_operand *base, const nfm_operand *mat,
                                 const nfm_operand *gout, const nfm_operand *gmat, void *stream);
int nfm_sym_pencil_eig(int dtype, int M, int mode, int64_t n_outer, int64_t n_inner, const nfm_operand *base,
                       const nfm_operand *mat, const nfm_operand *out, void *stream);
int nfm_sym_pencil_dist_backward(int dtype, int M, int mode, int64_t n_outer, int64_t n_inner,
                                 const nfm_operand *base, const nfm_operand *mat, const nfm_operand *gout,
                                 const nfm_operand *grads, void *stream);
/* largest M with a kernel for op = NFM_PENCIL_OP_*; 0 for an unknown dtype or op */
int nfm_sym_pencil_max_order(int dtype, int op);

/* EXTENSION (no counterpart in the reference): the sorted eigendecomposition mat = V diag(l) V^T of compact symmetric
 * matrices, in the lane's registers (the arithmetic of nfm_sym_funm; its scale rule puts every finite record in range).
 * flags = NFM_EIGH_ASCENDING, _DESCENDING or _ABS (ascending |l|, ties by l ascending), or'ed with NFM_EIGH_VECTORS.
 * nfm_sym_eigh: without NFM_EIGH_VECTORS out holds records of the M values; with it, records of M + M M values:
 * the values, then V row-major (column k belongs to value k).  The component of largest magnitude of every column is
 * positive (the first such component among exact ties; the rule is applied after the sort).
 * nfm_sym_eigh_backward: gmat = the gradient with respect to the compact record for the cotangents gval (M values)
 * and gvec (M M values, row-major; NULL: the values alone, and NFM_EIGH_VECTORS in flags is ignored):
 * S = V W V^T, W_kk = gval_k, W_kl = (B_kl - B_lk) / (2 (l_l - l_k)) with B = V^T gvec, returned as S_ii and 2 S_ij
 * (the compact convention of nfm_sym_funm_backward).  The decomposition is recomputed from mat by the same code: the
 * same order and signs.  THE GAP RULE: a pair with |l_k - l_l| <= 16 M eps max_i |l_i| has W_kl = 0, so the gradient
 * of every finite record is finite.  `gmat` may be `gval`.
 * A record with an entry that is not finite is NaN in every component (values, vectors, gradient); the other records
 * do not notice.
 * M in 1..nfm_sym_eigh_max_order(dtype, op), op = NFM_EIGH_OP_*.  Status precedence: that of nfm_sym_funm
 * (NFM_EINVAL for unknown flags before NFM_ESIZE for M above the compiled cap, then the operands in argument
 * order). */
#define NFM_EIGH_ASCENDING 0
#define NFM_EIGH_DESCENDING 1
#define NFM_EIGH_ABS 2
#define NFM_EIGH_VECTORS 4
#define NFM_EIGH_OP_VALUES 0
#define NFM_EIGH_OP_VECTORS 1
#define NFM_EIGH_OP_VALUES_BACKWARD 2
#define NFM_EIGH_OP_BACKWARD 3
int nfm_sym_eigh(int dtype, int M, int flags, int64_t n_outer, int64_t n_inner, const nfm_operand *mat,
                 const nfm_operand *out, void *stream);
int nfm_sym_eigh_backward(int dtype, int M, int flags, int64_t n_outer, int64_t n_inner, const nfm_operand *mat,
                          const nfm_operand *gval, const nfm_operand *gvec, const nfm_operand *gmat, void *stream);
/* largest M with a kernel for op = NFM_EIGH_OP_*; 0 for an unknown dtype or op */
int nfm_sym_eigh_max_order(int dtype, int op);
/* CPU: what the kernels do after the sweeps, in place on n host records of order N <= 8 (NFM_ESIZE beyond): lam
 * (n N values) and vec (n N N values, row-major, or NULL) are sorted into `order` (NFM_EIGH_ASCENDING .. _ABS, no
 * flag) and the sign rule is applied; w (n N N values, or NULL) receives the weights 1 / (l_l - l_k) at [k][l] under
 * the gap rule (0 on the diagonal).  NFM_EDTYPE; NFM_EINVAL for n < 0, an unknown order or lam == NULL with n > 0. */
int nfm_sym_eigh_host_finish(int dtype, int order, int N, int64_t n, void *lam, void *vec, void *w);

/* EXTENSION (no counterpart in the reference): Cholesky kernels of compact symmetric positive definite matrices,
 * mat = L L^T with L lower triangular, in the lane's registers; every record is read once.  Compact in, compact out:
 * L_ij (i >= j) is stored where the compact layout stores (i, j), so the first M values of a factor are its diagonal.
 * nfm_sym_chol: op =
 *   NFM_CHOL_FACTOR              out = L (M (M + 1) / 2 values); vec is not read (NULL)
 *   NFM_CHOL_APPLY_L / _LT       out = L vec / L^T vec (M values)
 *   NFM_CHOL_APPLY_LINV / _LTINV out = L^-1 vec / L^-T vec (M values); or'ed with NFM_CHOL_FACTORED, the four apply
 *                                ops read `mat` as a factor that is already there (the result of NFM_CHOL_FACTOR)
 *   NFM_CHOL_LOGDET              out = log det mat = 2 sum_i log L_ii (one value); vec is not read (NULL)
 *   NFM_CHOL_MAHA / _MAHA_SQRT   out = vec^T mat^-1 vec = |L^-1 vec|^2 (one value) / its root
 *   NFM_CHOL_LOGPDF              out = -(M log 2 pi + log det mat + vec^T mat^-1 vec) / 2 (one value)
 * nfm_sym_chol_backward: op = NFM_CHOL_LOGDET, _MAHA, _MAHA_SQRT or _LOGPDF; gout = the cotangent of the value (one
 * per record); gpacked = records of M (M + 1) / 2 + M values (NFM_CHOL_LOGDET: M (M + 1) / 2, vec is not read): the
 * gradient with respect to mat in the compact convention of nfm_sym_funm_backward (S_ii, 2 S_ij), then the one with
 * respect to vec.  With w = mat^-1 vec: LOGDET S = gout mat^-1; MAHA S = -gout w w^T, gvec = 2 gout w; MAHA_SQRT the
 * same with gout / (2 d), zero where d == 0; LOGPDF S = -gout (mat^-1 - w w^T) / 2, gvec = -gout w.  The factor is
 * recomputed from mat.
 * A record with an entry of mat or vec that is not finite, or with a pivot a_jj - sum_k l_jk^2 that is not > 0, is NaN
 * in every value (results and gradients); the other records do not notice.  Nothing is scaled and nothing overflows
 * that mat and its root do not.
 * M in 1..nfm_sym_chol_max_order(dtype, class), class = NFM_CHOL_CLASS_*.  Status precedence: that of nfm_sym_funm
 * (NFM_EINVAL for an unknown op, or NFM_CHOL_FACTORED on an op that is not an apply, before NFM_ESIZE for M above the
 * compiled cap, then the operands in argument order; an operand the op does not read is not looked at). */
#define NFM_CHOL_FACTOR 0
#define NFM_CHOL_APPLY_L 1
#define NFM_CHOL_APPLY_LT 2
#define NFM_CHOL_APPLY_LINV 3
#define NFM_CHOL_APPLY_LTINV 4
#define NFM_CHOL_LOGDET 5
#define NFM_CHOL_MAHA 6
#define NFM_CHOL_MAHA_SQRT 7
#define NFM_CHOL_LOGPDF 8
#define NFM_CHOL_FACTORED 16
#define NFM_CHOL_CLASS_FACTOR 0
#define NFM_CHOL_CLASS_APPLY 1
#define NFM_CHOL_CLASS_SCALAR 2
#define NFM_CHOL_CLASS_BACKWARD 3
int nfm_sym_chol(int dtype, int M, int op, int64_t n_outer, int64_t n_inner, const nfm_operand *mat,
                 const nfm_operand *vec, const nfm_operand *out, void *stream);
int nfm_sym_chol_backward(int dtype, int M, int op, int64_t n_outer, int64_t n_inner, const nfm_operand *mat,
                          const nfm_operand *vec, const nfm_operand *gout, const nfm_operand *gpacked, void *stream);
/* largest M with a kernel for op_class = NFM_CHOL_CLASS_*; 0 for an unknown dtype or class */
int nfm_sym_chol_max_order(int dtype, int op_class);
/* CPU: the record routines the kernels run, on n contiguous host records of order M <= 8 (NFM_ESIZE beyond): mat (n
 * M (M + 1) / 2 values), vec (n M values, or NULL for an op without one), out (n records of the op's result).  With
 * gout (n values) given, the backward routine of `op` runs instead and out receives the packed gradients.
 * NFM_EDTYPE; NFM_EINVAL for n < 0, an unknown op (with gout: an op without a gradient), or a null mat, out or needed
 * vec with n > 0. */
int nfm_sym_chol_host(int dtype, int M, int op, int64_t n, const void *mat, const void *vec, const void *gout,
                      void *out);

/* EXTENSION: the gradient of the factor itself (the backward pass of NFM_CHOL_FACTOR and of the four apply ops), one
 * record per lane: the factor is recomputed (or adopted) in registers and pulled back by two triangular sweeps.
 * nfm_sym_chol_grad: op =
 *   NFM_CHOL_FACTOR         gout = the cotangent of the factor: M (M + 1) / 2 values per record, one per stored entry
 *                           L_ij (i >= j), each counted once; vec is not read (NULL); gpacked = M (M + 1) / 2 values:
 *                           S = L^-T (P + P^T) L^-1 / 2, P = the lower triangle of L^T gout with a halved diagonal, in
 *                           the compact convention of nfm_sym_chol_backward (S_ii, 2 S_ij).  Or'ed with
 *                           NFM_CHOL_FACTORED, `mat` is the factor already computed (the saved result of the forward).
 *   NFM_CHOL_APPLY_*        gout = the cotangent of the applied vector (M values); gpacked = M (M + 1) / 2 + M values,
 *                           the gradient with respect to mat, then the one with respect to vec (gvec).  With y the
 *                           forward result: _L gvec = L^T gout, G = tril(gout vec^T); _LT gvec = L gout, G = tril(vec
 *                           gout^T); _LINV gvec = L^-T gout, G = -tril(gvec y^T); _LTINV gvec = L^-1 gout, G = -tril(y
 *                           gvec^T).  G is pulled back to S as above; or'ed with NFM_CHOL_FACTORED, `mat` is a factor
 *                           and the first part of gpacked is G itself, plain: one value per stored entry.
 * The scalar op codes are NFM_EINVAL here (their gradient is nfm_sym_chol_backward).  Bad records as nfm_sym_chol (with
 * NFM_CHOL_FACTORED: a diagonal that is not > 0), and a cotangent entry that is not finite: NaN in every value.
 * M in 1..nfm_sym_chol_grad_max_order(dtype, class), class = NFM_CHOL_CLASS_FACTOR or NFM_CHOL_CLASS_APPLY (0 for any
 * other class or dtype).  Status precedence: that of nfm_sym_chol. */
int nfm_sym_chol_grad(int dtype, int M, int op, int64_t n_outer, int64_t n_inner, const nfm_operand *mat,
                      const nfm_operand *vec, const nfm_operand *gout, const nfm_operand *gpacked, void *stream);
int nfm_sym_chol_grad_max_order(int dtype, int op_class);
/* CPU: the same record routines on n contiguous host records of order M <= 8 (NFM_ESIZE beyond): mat (n M (M + 1) / 2
 * values), vec (n M values, or NULL for NFM_CHOL_FACTOR), gout and out as gout and gpacked above.  NFM_EDTYPE;
 * NFM_EINVAL for n < 0, an op that is neither the factor nor an apply, or a null mat, gout, out or needed vec with
 * n > 0. */
int nfm_sym_chol_grad_host(int dtype, int M, int op, int64_t n, const void *mat, const void *vec, const void *gout,
                           void *out);

/* -------------------------------------------------------------- batched ---- */

#define NFM_FLAG_TS_PERTURB 1 /* add (max|A| - min|A|) * 1e-12 to det for N in {2,3}:
                                 the TorchScript forms `inv2`/`inv3`, `_impl/batched.py:74-76,94-96` */

/* out = a^-1 for general N x N matrices, `batchinv` `_impl/batched.py:101-130`.
 * N <= 3: adjugate / det; N > 3: in-register Gauss-Jordan with partial pivoting
 * (the reference falls back to LAPACK getrf/getri there); contiguous operands at
 * N = 9..16 (float64: 9..13), here and in nfm_batch_det: the elimination without row
 * exchanges first, accepted while every diagonal pivot is within 1/8 of its column's
 * maximum (threshold pivoting), the pivoted elimination for the groups of matrices that
 * hold one which needs an exchange -- same answers within rounding.  out may alias a. */
int nfm_batch_inv(int dtype, int N, int flags, int64_t n_outer, int64_t n_inner,
                  const nfm_operand *a, const nfm_operand *out, void *stream);

/* det(a), `batchdet` `_impl/batched.py:35-63`. */
int nfm_batch_det(int dtype, int N, int64_t n_outer, int64_t n_inner, const nfm_operand *a,
                  const nfm_operand *out, void *stream);

/* out = a v for (rows x cols) matrices, `batchmatvec` `_impl/batched.py:154-190`. */
int nfm_batch_matvec(int dtype, int rows, int cols, int64_t n_outer, int64_t n_inner,
                     const nfm_operand *a, const nfm_operand *v, const nfm_operand *out,
                     void *stream);

/* EXTENSION (no counterpart in the reference): singular value and polar decompositions of general N x N matrices,
 * one record per lane: the one-sided Jacobi sweeps of nfm_svd_solve (prescale by a power of two, relative rotation
 * test, null guard, at most NFM_SVD_MAX_SWEEPS sweeps) on the rows of [a | I], a sort by descending singular value,
 * and for rank-deficient records an orthonormal completion of the right singular vectors.
 *   nfm_batch_svdvals: out record S (N), non-negative, descending.
 *   nfm_batch_svd:     out record [S (N) | U (N x N) | Vh (N x N)], row-major blocks of one packed record of
 *                      N + 2 N^2 values, a = U diag(S) Vh; U and Vh are orthogonal for every finite record.
 *   nfm_batch_polar:   out record [R (N x N) | P (N x N)], a = R P, R = U Vh orthogonal, P = Vh^T diag(S) Vh with
 *                      exactly equal mirrored entries.  For a singular record P is unique and R is one valid factor.
 *   nfm_batch_polar_backward: ga = the gradient with respect to a given the cotangents gr of R and gp of P (either may
 *                      be NULL, meaning zeros; not both).  The decomposition is recomputed from a.  With
 *                      B = U^T gr V and C = V^T sym(gp) V: ga = U X V^T, X_ij = ((B - B^T)_ij + 2 s_i C_ij) / (s_i + s_j):
 *                      finite at repeated singular values.  A record with two numerically null singular values
 *                      (R is not differentiable there) and a non-zero gr is NaN; its gp part is finite.
 * The out / gr / gp / ga operands describe their packed record with stride_col (stride_row is ignored for the
 * packed outputs of the three forward entries; gr, gp and ga are N x N operands like a).  A record with an entry
 * that is not finite gives a NaN record and nothing else.  N in 1..nfm_polar_max_order(dtype, op).
 * Status precedence: NFM_EDTYPE; NFM_EINVAL negative count; NFM_ESIZE n_outer; NFM_ESIZE N outside 1..NFM_MAX_DIM;
 * NFM_ESIZE N above the compiled cap (the caller's own route: the Python facade runs torch.linalg.svd there);
 * NFM_EINVAL gr and gp both NULL; then the operands in argument order. */
#define NFM_POLAR_OP_SVDVALS 0
#define NFM_POLAR_OP_SVD 1
#define NFM_POLAR_OP_POLAR 2
#define NFM_POLAR_OP_POLAR_BACKWARD 3
int nfm_batch_svdvals(int dtype, int N, int64_t n_outer, int64_t n_inner, const nfm_operand *a,
                      const nfm_operand *out, void *stream);
int nfm_batch_svd(int dtype, int N, int64_t n_outer, int64_t n_inner, const nfm_operand *a, const nfm_operand *out,
                  void *stream);
int nfm_batch_polar(int dtype, int N, int64_t n_outer, int64_t n_inner, const nfm_operand *a,
                    const nfm_operand *out, void *stream);
int nfm_batch_polar_backward(int dtype, int N, int64_t n_outer, int64_t n_inner, const nfm_operand *a,
                             const nfm_operand *gr, const nfm_operand *gp, const nfm_operand *ga, void *stream);
/* largest N with a kernel for op (NFM_POLAR_OP_*); 0 for an unknown dtype or op */
int nfm_polar_max_order(int dtype, int op);
/* CPU: the record routine of the kernels on n contiguous row-major host records (a: n x N x N; out as the entry
 * of op writes it, packed; gr / gp only for NFM_POLAR_OP_POLAR_BACKWARD, either may be NULL).  N in
 * 1..NFM_SVD_MAX_DIM whatever the compiled caps.  Returns the largest number of sweeps a record took (>= 0), or
 * NFM_EDTYPE, NFM_EINVAL (n < 0, unknown op, a null pointer with n > 0, no cotangent), NFM_ESIZE. */
int nfm_polar_host(int dtype, int op, int N, int64_t n, const void *a, const void *gr, const void *gp, void *out);

/* ------------------------------------------------------------------ lie ---- */

/* out = expm(x) for (D x D) matrices, `expm` / `expm_derivatives` without derivatives
 * (`_impl/expm.py:15-49`, series `:139-190`).  Per matrix: scaling by 2^-s with ||x||_1 / 2^s <= 1,
 * the reference's Taylor series up to the degree at which the bound of its term passes its own stop
 * test (sum of squares <= D^2 tol, at most max_order terms), s squarings (quirk Q17); a matrix with a
 * non-finite entry gives NaN everywhere (Q18).  D == 1 is exp().  float32 D = 1..8, float64 D = 1..7;
 * NFM_ESIZE for every other order. */
int nfm_lie_expm(int dtype, int D, int max_order, double tol, int64_t n_outer, int64_t n_inner,
                 const nfm_operand *x, const nfm_operand *out, void *stream);

/* Frechet derivatives of expm at x, the terms `dE` / `hE` of `expm_derivatives`
 * (`_impl/expm.py:161-176`) for one direction (pair) per matrix:
 *   b == NULL: out = L(x, a)      = d/dt expm(x + t a) at t = 0
 *   else:      out = L2(x, a, b)  = d2/dt du expm(x + t a + u b) at 0 (symmetric in a and b)
 * Same scaling, degree and squarings as nfm_lie_expm.  The adjoint L(x^T, g) is this call with x's
 * stride_row and stride_col swapped.  D = 1..4, both dtypes; NFM_ESIZE otherwise. */
int nfm_lie_expm_frechet(int dtype, int D, int max_order, double tol, int64_t n_outer, int64_t n_inner,
                         const nfm_operand *x, const nfm_operand *a, const nfm_operand *b,
                         const nfm_operand *out, void *stream);

/* out = logm(x), the principal logarithm of (D x D) matrices (`_impl/logm.py:102`, scipy on the CPU in the
 * reference).  Per matrix: Denman-Beavers square roots until ||x - I||_1 <= 0.25, then 2^(s+1) atanh of
 * (x - I)(x + I)^-1 by its series (quirk Q20).  Arithmetic and output in `dtype` (Q21).  A matrix with a
 * non-finite entry, a singular one, or one with an eigenvalue on the closed negative real axis gives NaN
 * everywhere (Q22); logm(I) is exactly 0.  D == 1 is log().  float32 D = 1..8, float64 D = 1..7; NFM_ESIZE
 * for every other order. */
int nfm_lie_logm(int dtype, int D, int64_t n_outer, int64_t n_inner, const nfm_operand *x,
                 const nfm_operand *out, void *stream);

/* out = logm(m^-1 a): one pivoted elimination on [m | a] in the lane, then the body of nfm_lie_logm -- the
 * step of `meanm` (`lie.py:78-79`), with m at stride 0 along the set.  Same orders and NaN rule. */
int nfm_lie_logm_solve(int dtype, int D, int64_t n_outer, int64_t n_inner, const nfm_operand *m,
                       const nfm_operand *a, const nfm_operand *out, void *stream);

/* out = L_log(x, g) = d/dt logm(x + t g) at t = 0: the steps of nfm_lie_logm differentiated.  The adjoint
 * L_log(x^T, g) is this call with x's stride_row and stride_col swapped.  D = 1..5, both dtypes; NFM_ESIZE
 * otherwise. */
int nfm_lie_logm_frechet(int dtype, int D, int64_t n_outer, int64_t n_inner, const nfm_operand *x,
                         const nfm_operand *g, const nfm_operand *out, void *stream);

/* ------------------------------------------------------------ reductions ---- */

#define NFM_RED_NANSUM 0 /* `nansum` reduce.py:471-510 : NaN -> 0              */
#define NFM_RED_NANMAX 1 /* `nanmax` reduce.py:255-316 : NaN -> -inf           */
#define NFM_RED_NANMIN 2 /* `nanmin` reduce.py:319-380 : NaN -> +inf           */
#define NFM_RED_SUM 3    /* `sum`    reduce.py:431-468 : NaN propagates        */
#define NFM_RED_MAX 4    /* `max`    reduce.py:145-197                         */
#define NFM_RED_MIN 5    /* `min`    reduce.py:200-252                         */
#define NFM_RED_NANCOUNT 6 /* number of non-NaN elements (weights of `nanmean` reduce.py:591-594) */
#define NFM_RED_NANSUMSQ 7 /* sum of squares of the non-NaN elements (`nanvar` reduce.py:679-680) */

/* bytes of device workspace `nfm_reduce_all` needs (independent of n). */
size_t nfm_reduce_workspace_bytes(void);

/* Full reduction of n contiguous elements to ONE scalar.  Sums are accumulated in
 * double whatever the input dtype; `out_dtype` is the dtype of *out (the `dtype=`
 * argument of the reference functions).  n may exceed 2^32.  workspace: device
 * memory of nfm_reduce_workspace_bytes() bytes, 16-byte aligned. */
int nfm_reduce_all(int dtype, int op, int out_dtype, int64_t n, const void *x, void *workspace,
                   size_t workspace_bytes, void *out, void *stream);

/* Reduction over the middle axis of a contiguous (outer, red, inner) view
 * (`_reduce_index` / `sum` with `dim=`, `reduce.py:49-142`, `:431-510`); out is (outer, inner)
 * of `out_dtype`; idx (may be NULL; max/min ops only) receives the int64 position along `red`
 * of the selected element (first occurrence).  Shapes with few outputs and a long reduced
 * axis are cut into chunks reduced in parallel and folded in a fixed order: they need
 * nfm_reduce_dim_workspace_bytes(...) bytes of device workspace (0 for the other shapes;
 * workspace may then be NULL).  The plan depends on the shape only: results are reproducible. */
size_t nfm_reduce_dim_workspace_bytes(int dtype, int op, int64_t outer, int64_t red, int64_t inner,
                                      int want_idx);
int nfm_reduce_dim(int dtype, int op, int out_dtype, int64_t outer, int64_t red, int64_t inner,
                   const void *x, void *workspace, size_t workspace_bytes, void *out, int64_t *idx,
                   void *stream);

/* One pass over a contiguous (outer, red, inner) view producing, per (outer, inner) entry,
 * four doubles [count, sum(x - K), sum((x - K)^2), K] over the non-NaN elements of the
 * reduced axis (K = a finite element of that slice, chosen by the kernel).  The raw material
 * of `nanmean` / `nanvar` / `nanstd` / `mean` / `var` / `std` (`reduce.py:513-763`).
 * workspace: nfm_reduce_moments_workspace_bytes(...) bytes. */
size_t nfm_reduce_moments_workspace_bytes(int dtype, int64_t outer, int64_t red, int64_t inner);
int nfm_reduce_moments(int dtype, int64_t outer, int64_t red, int64_t inner, const void *x,
                       void *workspace, size_t workspace_bytes, double *out, void *stream);

/* mean / var / std over the middle axis in ONE pass (the moments above, finished in the
 * kernel): `mean` `reduce.py:513-550`, `nanmean :553-594`, `var :597-635`, `nanvar :638-685`,
 * `std :688-726`, `nanstd :729-763`.  stat = NFM_STAT_MEAN|VAR|STD, or-ed with
 * NFM_STAT_OMITNAN (ignore NaNs; otherwise a NaN in the slice gives NaN) and
 * NFM_STAT_UNBIASED (var/std: multiply by n / (n - 1), `reduce.py:682-684`).
 * out is (outer, inner) of `out_dtype`; workspace as for nfm_reduce_moments. */
#define NFM_STAT_MEAN 0
#define NFM_STAT_VAR 1
#define NFM_STAT_STD 2
#define NFM_STAT_OMITNAN 4
#define NFM_STAT_UNBIASED 8
int nfm_reduce_stat(int dtype, int stat, int out_dtype, int64_t outer, int64_t red, int64_t inner,
                    const void *x, void *workspace, size_t workspace_bytes, void *out, void *stream);

/* Median of every row of a contiguous (rows, red) array, `median` `reduce.py:384-428` (which
 * moves the reduced dims last and calls torch.median; the facade does the same move): the
 * LOWER median (rank (count - 1) / 2), on order-preserving integer keys: a register sorting network
 * per row for rows of up to 128 elements (float64: 64), radix selection for longer ones.
 * omitnan = 0: a NaN in a row makes its median NaN (idx: the first NaN) -- what the reference
 * computes; omitnan = 1: the median of the non-NaN elements (all NaN: NaN, idx 0) -- what its
 * docstring promises (quirk Q14).  val: (rows) of `dtype`; idx: (rows) int64 or NULL = the first
 * position holding the median value.  Rows of more than 1024 elements need a workspace of
 * nfm_reduce_median_workspace_bytes(rows, red) bytes (0 for shorter rows) and rows <= 65535. */
size_t nfm_reduce_median_workspace_bytes(int64_t rows, int64_t red);
int nfm_reduce_median(int dtype, int omitnan, int64_t rows, int64_t red, const void *x, void *workspace,
                      size_t workspace_bytes, void *val, void *idx, void *stream);

/* The same median over the MIDDLE dim of a contiguous (outer, red, inner) array -- the channel dim of a
 * channel-first field -- without the transposing copy that moving the reduced dim last would cost (the
 * reference makes that copy: `reduce.py:112-113`).  One row per lane, so only for
 * 2 <= red <= nfm_reduce_median_lane_max(dtype) (128 for float32, 64 for float64; NFM_ESIZE beyond).
 * val / idx: (outer, inner), idx = position along the reduced dim. */
int nfm_reduce_median_lane_max(int dtype);
int nfm_reduce_median_mid(int dtype, int omitnan, int64_t outer, int64_t red, int64_t inner, const void *x, void *val,
                          void *idx, void *stream);

/* Quantiles of every row of a contiguous (rows, red) array: the median's radix selection at several
 * arbitrary ranks per row.  The reference has no counterpart (its one order statistic is `median`,
 * `reduce.py:384-428`); the conventions are the median's: keys ordered -0.0 before +0.0 and NaN last,
 * omitnan = 0: a NaN in a row makes every quantile of the row NaN, omitnan = 1: the quantiles of the
 * non-NaN elements (all NaN: NaN).  With count = the elements counted, p = fl64(q * (count - 1)),
 * lo = floor(p), hi = ceil(p), w = p - lo and v_lo, v_hi the order statistics of those ranks:
 * NFM_QUANTILE_LOWER v_lo; HIGHER v_hi; NEAREST the rank rint(p), half to even; MIDPOINT = LINEAR with
 * w = 0.5; LINEAR v_lo when v_lo == v_hi (no arithmetic: two equal infinities give that infinity), else in
 * float64 w < 0.5 ? a + w (b - a) : b - (b - a) (1 - w), rounded once to `dtype`.
 * q: nq numbers in [0, 1] on the HOST, read during the call and passed to the kernels by value (nothing is
 * copied to the device: the call can be captured in a graph).  val: (nq, rows) of `dtype`.  pos: NULL or
 * (nq, rows, 2) int64 = the first position in the row holding v_lo and the first holding v_hi (LOWER,
 * HIGHER, NEAREST: twice the position of the chosen element; a NaN result: 0, 0).
 * Rows of more than 1024 elements need a workspace of nfm_reduce_quantile_workspace_bytes(rows, red, nq)
 * bytes (0 for shorter rows; it grows with nq) and rows <= 65535.
 * Checks, before any HIP call, in this precedence: dtype (NFM_EDTYPE); rows < 0, red < 0, nq < 1, a bad
 * interp (NFM_EINVAL); nq > nfm_reduce_quantile_max_q() (NFM_ESIZE); q NULL, a q outside [0, 1] or NaN
 * (NFM_EINVAL); rows == 0: NFM_OK without a launch; red == 0, x or val NULL (NFM_EINVAL); red > 1024:
 * rows > 65535 (NFM_ESIZE), then a workspace that is NULL or too small (NFM_EINVAL, as nfm_reduce_median).
 * nfm_reduce_quantile_plan_host runs the kernels' own rank routine on the CPU: the ranks the selection
 * resolves (LOWER / HIGHER / NEAREST: lo == hi == the chosen rank, w = 0; MIDPOINT: w = 0.5) for count >= 1
 * (count == 0, a bad q or interp, a NULL output: NFM_EINVAL). */
#define NFM_QUANTILE_LINEAR 0
#define NFM_QUANTILE_LOWER 1
#define NFM_QUANTILE_HIGHER 2
#define NFM_QUANTILE_NEAREST 3
#define NFM_QUANTILE_MIDPOINT 4
int nfm_reduce_quantile_max_q(void); /* quantiles one launch takes (8) */
size_t nfm_reduce_quantile_workspace_bytes(int64_t rows, int64_t red, int nq);
int nfm_reduce_quantile(int dtype, int omitnan, int interp, int64_t rows, int64_t red, int nq, const double *q,
                        const void *x, void *workspace, size_t workspace_bytes, void *val, void *pos, void *stream);
int nfm_reduce_quantile_plan_host(double q, uint64_t count, int interp, uint64_t *lo, uint64_t *hi, double *w);

/* ------------------------------------------------------------------- qr ---- */
/* Real dtypes.  Multi-output routines write ONE packed, contiguous output record per
 * matrix into `out` (n_outer * n_inner records, batch-major); the layout of the record
 * is given with each entry point.  Inputs are ordinary strided operands. */

#define NFM_SIDE_LEFT 0
#define NFM_SIDE_RIGHT 1
#define NFM_SIDE_BOTH 2

/* c = x / r, s = -y / r, r = sqrt(x^2 + y^2); r == 0 -> (1, 0).  `givens` `_impl/qr.py:326-369`.
 * x, y: one element per batch entry; out record: [c, s]. */
int nfm_qr_givens(int dtype, int64_t n_outer, int64_t n_inner, const nfm_operand *x,
                  const nfm_operand *y, void *out, void *stream);

/* IN PLACE on `a` (N x N): rotate rows (left), columns (right) or both i and j.
 * `givens_apply_` `_impl/qr.py:370-429`.  c, s: N components per batch entry (stride_col 0 =
 * one coefficient for the whole row/column, the usual case). */
int nfm_qr_givens_apply(int dtype, int N, int side, int i, int j, int64_t n_outer, int64_t n_inner,
                        const nfm_operand *a, const nfm_operand *c, const nfm_operand *s, void *stream);

/* Householder vector of x (length N) reflecting onto component `basis`, and the projection
 * alpha.  `householder_` `_impl/qr.py:55-69`.  out record: [u (N) | alpha]. */
int nfm_qr_householder(int dtype, int N, int basis, int64_t n_outer, int64_t n_inner,
                       const nfm_operand *x, void *out, void *stream);

/* IN PLACE on `a` (N x N): apply P = I - 2 u u^T, u of length m acting on the trailing m
 * rows (left) / columns (right).  One reflector of `householder_apply_` `_impl/qr.py:72-106`. */
int nfm_qr_householder_apply(int dtype, int N, int m, int side, int64_t n_outer, int64_t n_inner,
                             const nfm_operand *a, const nfm_operand *u, void *stream);

/* Householder reduction to Hessenberg form (sym == 0: `hessenberg_` `_impl/qr.py:117-141`) or
 * of a symmetric matrix to tridiagonal form reading only the `upper` / lower triangle
 * (sym != 0: `hessenberg_sym_upper_/lower_` `:280-323`; output filled symmetric).
 * out record: [H (N*N row-major) | with_u: (N-2) reflectors, reflector k in a slot of N-1
 * elements, its N-1-k entries first, zero padded]. */
int nfm_qr_hessenberg(int dtype, int N, int sym, int upper, int with_u, int64_t n_outer,
                      int64_t n_inner, const nfm_operand *a, void *out, void *stream);

/* Q, R of an upper-Hessenberg matrix by N-1 Givens rotations, `qr_hessenberg_`
 * `_impl/qr.py:432-454`.  out record: [Q (N*N) | R (N*N)]. */
int nfm_qr_qr_hessenberg(int dtype, int N, int64_t n_outer, int64_t n_inner, const nfm_operand *h,
                         void *out, void *stream);

/* One QR step H <- R Q (and U <- U Q when u != NULL), `rq_hessenberg_` `_impl/qr.py:457-530`.
 * sym != 0: the tridiagonal shortcut of the reference; sym == 0: the true R Q for any
 * Hessenberg input (quirk Q8 fixed).  out record: [H' (N*N) | U' (N*N) if u]. */
int nfm_qr_rq_hessenberg(int dtype, int N, int sym, int64_t n_outer, int64_t n_inner,
                         const nfm_operand *h, const nfm_operand *u, void *out, void *stream);

/* Eigenvalues (unsorted, deflation order) and optionally eigenvectors of symmetric matrices:
 * tridiagonalisation + explicit QR with Wilkinson shifts, `eig_sym` `qr.py:30-100`,
 * `_fwd_eig_sym` `_impl/qr.py:665-681`.  Convergence is judged per matrix with the
 * reference's criterion (quirk Q9).  out record: [vals (N) | NFM_EIG_VECTORS: vecs (N*N
 * row-major, eigenvectors in columns)].
 * flags: NFM_EIG_VECTORS  also compute the eigenvectors (`compute_u`); flags == 0 / 1 is exactly the
 *                          reference's `compute_u` argument and selects the reference's arithmetic:
 *                          its operation order, its tolerance, correctly rounded division and
 *                          square root -- bit-identical to the CPU restatement (same deflation
 *                          order, same eigenvector signs).
 *        NFM_EIG_FAST     opt-in: the sweeps use v_rsq + Newton steps (one for float32, two for
 *                          float64) and fma contraction, the last 2x2 block is diagonalised by one
 *                          Jacobi rotation, and `tol` is floored at the working precision of the
 *                          dtype, max(tol, (eps/4)^2): as accurate against the exact eigenvalues
 *                          and 2-3x the throughput, but the deflation ORDER and the eigenvector
 *                          SIGNS differ from the reference's for a share of the matrices (float32:
 *                          2 % at 3x3, 35 % at 8x8) and float32 values by up to 1.4e-6. */
#define NFM_EIG_VECTORS 1
#define NFM_EIG_FAST 2
int nfm_qr_eig_sym(int dtype, int N, int upper, int flags, int max_iter, double tol,
                   int64_t n_outer, int64_t n_inner, const nfm_operand *a, void *out, void *stream);

/* ---------------------------------------------------------------- simplex ---- */

/* softmax / log_softmax / logsumexp / logit along the middle axis of a contiguous (outer, K, inner)
 * view, with the reference's implicit class (`simplex.py`), one voxel per lane.
 * flags: NFM_SIMPLEX_IMPLICIT_IN   the input has a hidden class besides its K stored ones (logit 0; for
 *                                  logit: probability 1 - sum, clamped at 1e-8); K' = K + 1 classes take
 *                                  part in the arithmetic, the hidden one at position implicit_index;
 *        NFM_SIMPLEX_IMPLICIT_OUT  the output does not store class implicit_index.
 * 0 <= implicit_index < K'.  Without IMPLICIT_IN, logit takes class implicit_index as its reference.
 * x: (outer, K, inner); out: (outer, K' - IMPLICIT_OUT, inner), at least one class; lse: (outer, inner), the
 * per-voxel logsumexp -- the only output of NFM_SIMPLEX_LOGSUMEXP (out is ignored), optional second output
 * of NFM_SIMPLEX_SOFTMAX, NULL otherwise.  K' = 1..17 runs with the classes in registers (K <= 16 with a hidden class, K <= 17 without), K up to
 * NFM_SIMPLEX_MAX_K in sweeps over the class axis; NFM_ESIZE beyond.  NaN or +inf anywhere in a voxel makes
 * its whole result NaN (as does a voxel of -inf without a hidden class). */
#define NFM_SIMPLEX_SOFTMAX 0
#define NFM_SIMPLEX_LOG_SOFTMAX 1
#define NFM_SIMPLEX_LOGSUMEXP 2
#define NFM_SIMPLEX_LOGIT 3
#define NFM_SIMPLEX_SOFTMAX_BWD 4     /* saved = softmax output, grad_output like the output */
#define NFM_SIMPLEX_LOGSUMEXP_BWD 5   /* saved = input, grad_output (outer, inner) */
#define NFM_SIMPLEX_LOG_SOFTMAX_BWD 6 /* saved = input, grad_output like the output */
#define NFM_SIMPLEX_IMPLICIT_IN 1
#define NFM_SIMPLEX_IMPLICIT_OUT 2
#define NFM_SIMPLEX_MAX_K 48
int nfm_simplex_forward(int dtype, int op, int flags, int implicit_index, int64_t outer, int64_t K, int64_t inner,
                        const void *x, void *out, void *lse, void *stream);

/* Backward passes (op = NFM_SIMPLEX_*_BWD; flags, implicit_index, outer, K, inner as in the forward call):
 * grad_input (outer, K, inner) from one saved tensor and grad_output.  A class the output dropped has no
 * grad_output (it reads as 0); softmax rebuilds its probability as 1 - sum of the stored ones. */
int nfm_simplex_backward(int dtype, int op, int flags, int implicit_index, int64_t outer, int64_t K, int64_t inner,
                         const void *saved, const void *grad_output, void *grad_input, void *stream);

/* ---------------------------------------------------------------- special ---- */

/* Special functions of `special.py` over a flat range of n elements (float32 / float64), one 16-byte vector
 * per lane, any element-aligned pointers.  Return codes: NFM_EDTYPE unknown dtype; NFM_EINVAL mode outside
 * 0..2, nu < 0 or not finite, N < 0, K < 0, order < 1, n < 0, a null pointer with n > 0; NFM_ESIZE
 * N > NFM_SPECIAL_MAX_N; NFM_EALIGN a pointer not aligned to its element size; n == 0 succeeds with null
 * pointers.  The output of a forward call may be its input (in place).
 *
 * besseli: the modified Bessel function of the first kind I_nu(z), z >= 0.  mode 0: I_nu(z); 1: I_nu(z)
 * exp(-z); 2: log I_nu(z).  nu == 0 and nu == 1 run the reference's polynomials (A&S 9.8.1-9.8.4, 5e-7 from
 * the function); any other nu >= 0 is the function itself (series / uniform asymptotic expansion in double).
 * z = 0: 1 / 1 / 0 at nu = 0, 0 / 0 / -inf above; z = +inf: +inf / 0 / +inf; NaN -> NaN; z < 0 at another nu
 * than 0 or 1 -> NaN. */
#define NFM_SPECIAL_MAX_N 8
int nfm_special_besseli(int dtype, int mode, double nu, int64_t n, const void *z, void *out, void *stream);
/* grad_z = grad_out * d(out)/dz from z and the saved output: with r = I_{nu+1}(z) / I_nu(z),
 * d log I = r + nu/z, dI = I (r + nu/z), d(I exp(-z)) = I exp(-z) (r + nu/z - 1); the limit at z = 0. */
int nfm_special_besseli_backward(int dtype, int mode, double nu, int64_t n, const void *z, const void *out,
                                 const void *grad_out, void *grad_z, void *stream);
/* I_{nu+1}(x) / I_nu(x) by Amos (1974): eq. 20a at order nu + K, N rounds of eq. 20b (N <= NFM_SPECIAL_MAX_N),
 * K steps of the backward recurrence; 0 at x = 0 and 1 at x = +inf. */
int nfm_special_besseli_ratio(int dtype, double nu, int N, int K, int64_t n, const void *x, void *out, void *stream);
/* grad_x = grad_out * (1 - r^2 - (2 nu + 1) r / x) on the saved output r (1 / (2 nu + 2) at x = 0). */
int nfm_special_besseli_ratio_backward(int dtype, double nu, int64_t n, const void *x, const void *out,
                                       const void *grad_out, void *grad_x, void *stream);
/* sum_{p=1..order} digamma(x + (1 - p) / 2); digamma(0) = -inf, NaN at the negative integers. */
int nfm_special_mvdigamma(int dtype, int order, int64_t n, const void *x, void *out, void *stream);
/* grad_x = grad_out * sum_p trigamma(x + (1 - p) / 2). */
int nfm_special_mvdigamma_backward(int dtype, int order, int64_t n, const void *x, const void *grad_out, void *grad_x,
                                   void *stream);
/* The same arithmetic on the CPU with host pointers and no GPU: what a host test can check numerically.
 * func: NFM_SPECIAL_*; mode_or_order: mode of besseli, order of mvdigamma; unused arguments are ignored
 * (saved_out / grad_out may be NULL for the forward functions). */
#define NFM_SPECIAL_BESSELI 0
#define NFM_SPECIAL_BESSELI_BWD 1
#define NFM_SPECIAL_RATIO 2
#define NFM_SPECIAL_RATIO_BWD 3
#define NFM_SPECIAL_MVDIGAMMA 4
#define NFM_SPECIAL_MVDIGAMMA_BWD 5
int nfm_special_host_eval(int func, int dtype, int mode_or_order, double nu, int N, int K, int64_t n, const void *x,
                          const void *saved_out, const void *grad_out, void *result);

/* ------------------------------------------------------------------ sugar ---- */

/* X = A^-1 B for one N x N matrix and one N x K matrix of right-hand sides per batch element: `lmdiv`, and through
 * swapped row / column strides `rmdiv` (X B = A  <=>  B^T X^T = A^T), `solvevec` (K = 1) and `inv` of the
 * reference's `sugar.py:75-341`.  N, K in 1..NFM_SOLVE_MAX_DIM (NFM_ESIZE beyond, and for K above
 * nfm_sugar_max_cols(dtype, N): solve B in blocks of columns).  Each operand is given as a raw pointer and the
 * four strides of `struct nfm_operand` (elements; 0 = broadcast), and is read in place whatever they are.
 * flags NFM_SOLVE_LU: Gaussian elimination with partial pivoting (getrf / getrs, what `torch.linalg.solve` runs);
 * a singular record gives inf / NaN.  NFM_SOLVE_CHOL: A = L L^T from the LOWER triangle of A, the upper one is
 * never read; a record with a pivot that is not positive gets NaN in every entry of its result (no exception).
 * b == NULL: B is the identity and K must equal N (the inverse; NFM_SOLVE_LU then runs nfm_batch_inv).
 * `out` may alias `b`.  Status precedence: NFM_EDTYPE; NFM_EINVAL negative count; NFM_ESIZE n_outer; NFM_ESIZE
 * N or K; NFM_EINVAL unknown flag, or b == NULL with K != N; then a, b, out in this order: NFM_EINVAL for a null
 * pointer with a non-empty batch, NFM_EALIGN.  An empty batch with null pointers succeeds without a launch. */
#define NFM_SOLVE_LU 0
#define NFM_SOLVE_CHOL 1
#define NFM_SOLVE_MAX_DIM 8
int nfm_sugar_solve(int dtype, int N, int K, int flags, int64_t n_outer, int64_t n_inner,
                    const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                    const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                    void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc, void *stream);
/* largest K one nfm_sugar_solve call takes at order N (the register file bounds [A | B] per lane); NFM_EDTYPE /
 * NFM_ESIZE for an unknown dtype / an order outside 1..NFM_SOLVE_MAX_DIM */
int nfm_sugar_max_cols(int dtype, int N);

/* The same solve for the square orders NFM_ROWSOLVE_MIN_DIM..NFM_MAX_DIM (9..16), one row of [A | B] per lane slot
 * (16 / R lanes per matrix): the arguments, the flags, the identity for b == NULL (K == N; NFM_SOLVE_LU then runs
 * nfm_batch_inv, NFM_SOLVE_CHOL one launch per block of columns), the layouts read in place and `out` aliasing `b`
 * are those of nfm_sugar_solve.  NFM_SOLVE_LU pivots on the first row with the largest |a_rk| (compared at 20
 * mantissa bits in float64); NFM_SOLVE_CHOL eliminates without exchanges on the matrix rebuilt from the LOWER
 * triangle and gives NaN in every entry of a record with a pivot that is not positive.  Column j of X has the same
 * bits whatever K it was solved with and whatever the layout.  K in 1..nfm_rowsolve_max_cols(dtype, N) with a b.
 * Status precedence: NFM_EDTYPE; NFM_EINVAL negative count; NFM_ESIZE n_outer; NFM_ESIZE N outside 9..16 or K
 * outside 1..16; NFM_EINVAL unknown flag, or b == NULL with K != N; NFM_ESIZE K above the cap; then a, b, out in
 * this order: NFM_EINVAL for a null pointer with a non-empty batch, NFM_EALIGN.  An empty batch with null pointers
 * succeeds without a launch. */
#define NFM_ROWSOLVE_MIN_DIM 9
int nfm_rowsolve(int dtype, int N, int K, int flags, int64_t n_outer, int64_t n_inner,
                 const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                 const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                 void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc, void *stream);
/* largest K one nfm_rowsolve call takes at order N; NFM_EDTYPE / NFM_ESIZE for an unknown dtype / an order outside
 * NFM_ROWSOLVE_MIN_DIM..NFM_MAX_DIM */
int nfm_rowsolve_max_cols(int dtype, int N);

/* X = A^+ B for one M x N matrix and one M x K matrix of right-hand sides per batch element, by a one-sided Jacobi
 * SVD held in the lane's registers: `lmdiv` / `rmdiv` / `solvevec` / `inv` of the reference's `sugar.py` with
 * method 'svd' or 'pinv', and its non-square systems (least squares for M > N, minimum norm for M < N).  X is
 * N x K.  M, N, K in 1..NFM_SVD_MAX_DIM (NFM_ESIZE beyond, and for K above nfm_svd_max_cols(dtype, M, N): solve B
 * in blocks of columns).  The operand fields are those of nfm_sugar_solve; every layout is read in place.
 * flags NFM_SVD_PLAIN ('svd'): X = V S^-1 U^T B with every singular value; a zero one gives inf / NaN for that
 * record only.  NFM_SVD_PINV ('pinv'): the singular values sigma <= rcond sigma_max are dropped
 * (`torch.linalg.pinv`'s reading of rcond); rcond is ignored under NFM_SVD_PLAIN.
 * b == NULL: B is the M x M identity and K must equal M (the inverse / pseudo-inverse, N x M).  `out` may alias `b`
 * when M == N.  The sweep loop of a record is bounded by NFM_SVD_MAX_SWEEPS whatever the input (NaN included).
 * Status precedence: NFM_EDTYPE; NFM_EINVAL negative count; NFM_ESIZE n_outer; NFM_ESIZE M, N or K; NFM_EINVAL
 * unknown flag, an rcond that is negative or NaN, or b == NULL with K != M; NFM_ESIZE K above the cap; then a, b,
 * out in this order: NFM_EINVAL for a null pointer with a non-empty batch, NFM_EALIGN.  An empty batch with null
 * pointers succeeds without a launch. */
#define NFM_SVD_PLAIN 0
#define NFM_SVD_PINV 1
#define NFM_SVD_MAX_DIM 8
#define NFM_SVD_MAX_SWEEPS 16
int nfm_svd_solve(int dtype, int M, int N, int K, int flags, double rcond, int64_t n_outer, int64_t n_inner,
                  const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                  const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                  void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc, void *stream);
/* the same arithmetic on the calling thread, for records in host memory (one after the other, through the routine
 * the kernel runs): a check of the arithmetic that needs no device.  Same arguments and status codes; on success
 * the return value is the largest number of sweeps a record took (0 for an empty batch and for M == 1). */
int nfm_svd_solve_host(int dtype, int M, int N, int K, int flags, double rcond, int64_t n_outer, int64_t n_inner,
                       const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                       const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                       void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc);
/* largest K one nfm_svd_solve call takes for M x N records; NFM_EDTYPE / NFM_ESIZE for an unknown dtype / a size
 * outside 1..NFM_SVD_MAX_DIM */
int nfm_svd_max_cols(int dtype, int M, int N);

/* X = A^+ B for one TALL M x N matrix and one M x K matrix of right-hand sides per batch element: the least-squares
 * solves of `lmdiv` / `solvevec` / `rmdiv` with more rows than nfm_svd_solve holds.  X (N x K) = pinv(A, rcond) B:
 * the minimum-norm least-squares solution, singular values sigma <= rcond sigma_max dropped (`torch.linalg.pinv`'s
 * reading of rcond; the reference turns every non-square system into `pinv`, so there is no flags argument).  The
 * M rows of [A | B] stream once past an N x N triangle R and Q^T B held in the lane's registers (Givens rotations;
 * every record scaled by a running power of two, so any finite record is in range), and the Jacobi routine of
 * nfm_svd_solve finishes on R, which has the singular values of A: one read of A and B, one write of X, one launch,
 * no workspace, no host sync.  Rank deficiency is resolved by rcond alone.  A zero record gives X = 0; a NaN or inf
 * in a record gives NaN for that record only.
 * N in 1..8; M in N..NFM_LSTSQ_MAX_ROWS; K in 1..nfm_lstsq_max_cols(dtype, N) (solve B in blocks of columns beyond).
 * The operand fields are those of nfm_svd_solve; every layout is read in place.  `out` must not alias `a` or `b`.
 * Status precedence: NFM_EDTYPE; NFM_EINVAL negative count; NFM_ESIZE n_outer; NFM_ESIZE N or K outside 1..8;
 * NFM_ESIZE M < N or M > NFM_LSTSQ_MAX_ROWS; NFM_EINVAL an rcond that is negative or NaN; NFM_ESIZE K above the cap;
 * then a, b, out in this order: NFM_EINVAL for a null pointer with a non-empty batch, NFM_EALIGN.  An empty batch
 * with null pointers succeeds without a launch. */
#define NFM_LSTSQ_MAX_ROWS 4096
int nfm_lstsq_solve(int dtype, int M, int N, int K, double rcond, int64_t n_outer, int64_t n_inner,
                    const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                    const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                    void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc, void *stream);
/* the same per-record routine on the calling thread, for records in host memory.  Same arguments and status codes;
 * on success the return value is the largest number of sweeps the finishing Jacobi loop took (0 for an empty batch
 * and for N == 1). */
int nfm_lstsq_solve_host(int dtype, int M, int N, int K, double rcond, int64_t n_outer, int64_t n_inner,
                         const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                         const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                         void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc);
/* largest K one nfm_lstsq_solve call takes at N columns; NFM_EDTYPE / NFM_ESIZE for an unknown dtype / an N outside
 * 1..8 */
int nfm_lstsq_max_cols(int dtype, int N);

/* --------------------------------------------------------- realtransforms ---- */

/* Discrete cosine / sine transforms of types I, II, III along the middle axis of a contiguous (outer, N, inner)
 * view (`realtransforms.py`: dct, dst and, with norm and type flipped by the caller, idct, idst), one line per
 * lane as a direct sum against a table of cosines / sines that each workgroup builds for itself: one read and
 * one write per element, no workspace, no state.  With the unnormalised ("backward") matrices
 *     DCT-II  2 cos(pi k (2n+1) / 2N)                          DST-II  2 sin(pi (k+1) (2n+1) / 2N)
 *     DCT-III x0 + 2 sum_{n>=1} x_n cos(pi (2k+1) n / 2N)      DST-III (-1)^k x_{N-1} + 2 sum_{n<N-1} x_n sin(pi (2k+1) (n+1) / 2N)
 *     DCT-I   x0 + (-1)^k x_{N-1} + 2 sum x_n cos(pi k n / (N-1))   DST-I  2 sin(pi (k+1) (n+1) / (N+1))
 * norm NFM_RT_FORWARD scales by 1 / 2L (L = N; N - 1 for DCT-I, N + 1 for DST-I), NFM_RT_ORTHO by 1 / sqrt(2L) and
 * rescales the end terms so that the matrix is orthogonal (scipy's `orthogonalize=True`), NFM_RT_ORTHO_SCIPY is the
 * reference's 'ortho_scipy': 'ortho' for every DCT and for type I; for DST-II the FIRST output and for DST-III the
 * FIRST input carry the sqrt(2) correction instead of the last.  All of it happens in the one launch.
 * transpose != 0 applies the transposed matrix (the adjoint: what a backward pass needs).  `out` may alias `x`.
 * N in 1..nfm_rt_max_len(dtype); DCT-I needs N >= 2.
 * Status precedence: NFM_EDTYPE; NFM_EINVAL negative N / outer / inner; NFM_EINVAL unknown kind, type, norm or
 * transpose, N == 0, DCT-I with N == 1; NFM_ESIZE an element count past int64; NFM_RT_EFALLBACK N above the cap (the
 * caller's own route: the Python facade composes the transform from torch.fft there); then x, out: NFM_EINVAL
 * for a null pointer with a non-empty batch, NFM_EALIGN.  An empty batch succeeds without a launch. */
#define NFM_RT_DCT 0
#define NFM_RT_DST 1
#define NFM_RT_BACKWARD 0
#define NFM_RT_FORWARD 1
#define NFM_RT_ORTHO 2
#define NFM_RT_ORTHO_SCIPY 3
#define NFM_RT_MAX_N 256          /* no build serves longer lines; nfm_rt_max_len is the cap of this build */
#define NFM_RT_EFALLBACK (-100)   /* the line is longer than the kernels serve */
int nfm_rt_transform(int dtype, int kind, int type, int norm, int transpose, int64_t N, int64_t outer, int64_t inner,
                     const void *x, void *out, void *stream);
/* the same per-line routine on the calling thread, for tensors in host memory: a check of the arithmetic that
 * needs no device.  Same arguments and status codes; N up to NFM_RT_MAX_N whatever the kernels' cap. */
int nfm_rt_transform_host(int dtype, int kind, int type, int norm, int transpose, int64_t N, int64_t outer,
                          int64_t inner, const void *x, void *out);
/* longest line nfm_rt_transform takes for the dtype (NFM_EDTYPE for an unknown one) */
int nfm_rt_max_len(int dtype);
/* The same transform as a matrix product on the matrix cores, for the long axes the lane kernels leave out: a
 * workgroup stages 32 whole lines in LDS and contracts them against the same table with v_mfma_*_16x16x4 (exact
 * float32 / float64 fma chains).  Same arguments, checks and status codes as nfm_rt_transform; every N in
 * 1..NFM_RT_MAX_N is served (NFM_RT_EFALLBACK above), `out` may alias `x`, no workspace, no host sync. */
int nfm_rt_transform_mm(int dtype, int kind, int type, int norm, int transpose, int64_t N, int64_t outer,
                        int64_t inner, const void *x, void *out, void *stream);
/* longest line a caller should route to nfm_rt_transform_mm for the dtype: the largest of 128 / 256 at which it
 * is not slower than the torch.fft composition in both layouts, 64 if neither (NFM_EDTYPE for an unknown dtype) */
int nfm_rt_mm_max_len(int dtype);

/* ------------------------------------------------------------- stochastic ---- */

/* The library side of `stochastic.py` (`trapprox` :9-146, `maxeig_power` :316-362): the operator is the
 * caller's, the probes, inner products, deflation and normalisation around it are these three kernels.
 * Vectors are contiguous runs of n elements at element-aligned device pointers; at most
 * NFM_STOCH_MAX_VECS of them per argument.  Pointer ARRAYS (`x`, `y`, `z`) live on the HOST and are copied
 * into the kernel arguments, so a captured graph keeps them.  No atomics: every result has the same bits on
 * every call, and the same bits whether or not the pointers are 16-byte aligned. */
#define NFM_STOCH_MAX_VECS 8
#define NFM_STOCH_RADEMACHER 0 /* +1 / -1 with probability 1/2 (`stochastic.py:84-88`) */
#define NFM_STOCH_GAUSSIAN 1   /* standard normal (`stochastic.py:90-92`) */
#define NFM_STOCH_SCALE_NONE 0          /* sigma = 1 */
#define NFM_STOCH_SCALE_RSQRT 1         /* sigma = 1 / sqrt(*s) */
#define NFM_STOCH_SCALE_RSQRT_OR_DROP 2 /* the same if *s > (64 eps_dtype)^2 * *s_ref and *s is finite and positive;
                                           otherwise the output is zeroed */

/* Philox4x32-10 on the host: counter[4], key[2] -> out[4].  The generator of nfm_stoch_fill, for known-answer tests. */
int nfm_stoch_philox_host(const uint32_t *counter, const uint32_t *key, uint32_t *out);

/* out[i] = probe element `offset + i`, i in [0, n).  Element e is a function of (seed, e) alone: the same bits
 * whatever the launch geometry, the split of a range into several calls or the alignment of `out`.
 * Key = (seed low word, seed high word).
 * RADEMACHER: counter (e / 128 low, high, 0, 0); bit (e % 128) % 32 of word (e % 128) / 32: set = +1, clear = -1.
 * GAUSSIAN:   counter (e / 4 low, high, 0, 1); words (w0, w1), (w2, w3) are two Box-Muller pairs with
 *             u = (2 (w >> 9) + 1) 2^-24, r = sqrt(-2 ln u_a); elements 0..3 of the counter are
 *             r0 cos, r0 sin, r1 cos, r1 sin of 2 pi u_b; evaluated in float for NFM_F32, in double for NFM_F64. */
int nfm_stoch_fill(int dtype, int kind, uint64_t seed, int64_t offset, int64_t n, void *out, void *stream);

/* bytes of device workspace nfm_stoch_gram needs for (p, q) (independent of n); 0 for p or q outside 1..8 */
size_t nfm_stoch_gram_workspace_bytes(int p, int q);

/* out[j q + k] (+)= sum_i X_j[i] Y_k[i], 1 <= p, q <= NFM_STOCH_MAX_VECS (the m^2 `dot`s of `outerpp`,
 * `stochastic.py:111-116`, and every `flatten().dot()`).  Each X_j and Y_k is read once; products and sums in
 * double.  `out`: p q doubles anywhere in device memory (8-byte aligned); `accumulate` != 0 adds to them.
 * n == 0 sets them to 0 (or leaves them, with `accumulate`). */
int nfm_stoch_gram(int dtype, int p, int q, int64_t n, const void *const *x, const void *const *y, void *workspace,
                   size_t workspace_bytes, double *out, int accumulate, void *stream);

/* Z_k = sigma (Y_k - sum_j X_j C[j q + k]), 0 <= p <= 8 (0: a pure scale; x and c may be NULL), 1 <= q <= 8
 * (`mmpp`, `stochastic.py:118-123`, and `v /= dot(v, v).sqrt_()`, :359).  `c` (p q doubles), `s_ref` and `s` are
 * DEVICE pointers; `scale_op` is one of NFM_STOCH_SCALE_*.  Arithmetic in double, one rounding on store.
 * z[k] may be y[k] (in place); other overlaps are not allowed. */
int nfm_stoch_combine(int dtype, int p, int q, int64_t n, const void *const *x, const double *c, const void *const *y,
                      void *const *z, int scale_op, const double *s_ref, const double *s, void *stream);

/* ------------------------------------------------------------------- misc ---- */

const char *nfm_strerror(int code);
int nfm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NFM_HIP_H */
