"""
"Syntactic sugar" linear algebra on MI355X -- drop-in for `nitorch_fastmath.sugar` (`sugar.py`).

`lmdiv`, `rmdiv`, `solvevec` and `inv` on matrices of at most 8 rows and columns run one lane-per-system HIP
kernel: `nfm_sugar_solve` for `lu` / `chol` on square matrices (Gaussian elimination with partial pivoting on
`[A | B]`, or Cholesky from the lower triangle), `nfm_svd_solve` for `svd` / `pinv` and for every non-square
system (one-sided Jacobi SVD on the rows of `[A | B]`: least squares for m > n, minimum norm for m < n).  Tall
least-squares systems -- more than 8 rows (up to 4096), at most 8 columns: a model fit per voxel -- run
`nfm_lstsq_solve`: the rows of `[A | B]` stream once past an n x n triangle in the lane's registers (Givens
rotations) and the same Jacobi routine finishes on it, `pinv(a, rcond) @ b` in one launch.  Square
systems of order 9..16 with `lu` / `chol` run `nfm_rowsolve`: the rows of `[A | B]` spread over the lanes of a
matrix, Gauss-Jordan with partial pivoting (`lu`) or without exchanges on the lower triangle (`chol`).  The
reference runs torch's batched LU / SVD, which are slow on tiny matrices.  Transposed, broadcast, padded and
channel-first operands are read in place.  Non-square systems of more than 8 columns, square orders above 16,
`inv` of a tall matrix,
and `svd` / `pinv` / non-square calls that need a gradient, take
the reference's own torch composition on the device; the remaining names (`kron2`, `outer`, `trace`, `dot`,
`mdot`, `is_orthonormal`, `round`) are torch compositions on the device, without a kernel.

Deviations from the reference, on purpose: `rmdiv` computes the documented
`A B^-1` for any `k`; `inv(method='chol')` returns the inverse for 2-D inputs too; on the kernel path a record
that is not positive definite (`chol`) or is singular (`lu`, `svd`) gets NaN / inf results instead of an
exception for the whole batch; `kron2` keeps the reference's layout, which is not `torch.kron`'s; `pinv` drops
the singular values `<= rcond sigma_max` from squared row norms; `inv(method='svd', out=)` fills `out`.
"""
__all__ = [
    'kron2',
    'lmdiv',
    'rmdiv',
    'inv',
    'matvec',
    'solvevec',
    'outer',
    'trace',
    'dot',
    'mdot',
    'is_orthonormal',
    'round',
]
import collections
import torch
from . import _lib
from ._dispatch import Batch, broadcast_shapes, call, dtype_code, expand_batch, needs_grad, prepare

MAX_ORDER = _lib.SOLVE_MAX_DIM
_FLAGS = {'lu': _lib.SOLVE_LU, 'chol': _lib.SOLVE_CHOL}
_SVD_FLAGS = {'svd': _lib.SVD_PLAIN, 'pinv': _lib.SVD_PINV}
SVD_MAX_DIM = _lib.SVD_MAX_DIM
LSTSQ_MAX_ROWS, LSTSQ_MAX_N = _lib.LSTSQ_MAX_ROWS, _lib.LSTSQ_MAX_N

# One kernel family behind `lmdiv` / `inv`, for an (m, n) system and k columns of b:
#   entry    : its C entry point, `entry(dtype code, *scalars(m, n, k, flag, rcond), n_outer, n_inner, a, b, out,
#              stream)`
#   cap      : its column-cap query, `cap(dtype code, *dims(m, n))`
#   identity : the axis of `a` that is the k of a call with b=None (the identity), None when b is required
_Family = collections.namedtuple('_Family', 'entry scalars cap dims identity')
_SQUARE = _Family('nfm_sugar_solve', lambda m, n, k, flag, rcond: (n, k, flag),
                  'nfm_sugar_max_cols', lambda m, n: (n,), -1)
_SVD = _Family('nfm_svd_solve', lambda m, n, k, flag, rcond: (m, n, k, flag, float(rcond)),
               'nfm_svd_max_cols', lambda m, n: (m, n), -2)
_LSTSQ = _Family('nfm_lstsq_solve', lambda m, n, k, flag, rcond: (m, n, k, float(rcond)),
                 'nfm_lstsq_max_cols', lambda m, n: (n,), None)
_ROWSOLVE = _Family('nfm_rowsolve', lambda m, n, k, flag, rcond: (n, k, flag),
                    'nfm_rowsolve_max_cols', lambda m, n: (n,), -1)
ROWSOLVE_ORDERS = range(_lib.ROWSOLVE_MIN_DIM, _lib.MAX_DIM + 1)
_caps = {}


def _cap(query, dtype, *dims):
    """the library's answer to the column-cap query `query`, asked once per (dtype, dims)"""
    key = (query, dtype, dims)
    if key not in _caps:
        _caps[key] = int(getattr(_lib.lib(), query)(dtype_code(dtype), *dims))
    return _caps[key]


def max_cols(dtype, n):
    """Columns of `b` one launch takes at order `n` (the library's table, `nfm_sugar_max_cols`)."""
    return _cap(_SQUARE.cap, dtype, n)


def rowsolve_max_cols(dtype, n):
    """Columns of `b` one launch takes at an order `n` in 9..16 (the library's answer, `nfm_rowsolve_max_cols`)."""
    return _cap(_ROWSOLVE.cap, dtype, n)


def _square_family(n):
    """the kernel family of a square `lu` / `chol` system of order n, None beyond the kernels"""
    if 0 < n <= MAX_ORDER:
        return _SQUARE
    return _ROWSOLVE if n in ROWSOLVE_ORDERS else None


def svd_max_cols(dtype, m, n):
    """Columns of `b` one launch takes for an `m x n` system (the library's table, `nfm_svd_max_cols`)."""
    return _cap(_SVD.cap, dtype, m, n)


def lstsq_max_cols(dtype, n):
    """Columns of `b` one launch takes for a tall system of `n` columns (the library's table, `nfm_lstsq_max_cols`)."""
    return _cap(_LSTSQ.cap, dtype, n)


def _method(method, a):
    """the reference's reading of `method`: prefixes, any case; non-square systems are `pinv`"""
    m = str(method).lower()
    if a.shape[-1] != a.shape[-2]:
        return 'pinv'
    for name in ('lu', 'chol', 'svd', 'pinv'):
        if m.startswith(name):
            return name
    raise ValueError('Unknown inversion method {}.'.format(method))


def _fields(op):
    return op.ptr, op.stride_outer, op.stride_inner, op.stride_row, op.stride_col


def _launch(family, dev, dtype, scalars, a, b, out):
    """one call of the family's entry point; a / b / out share their batch dims (views); b None: the identity"""
    tensors = [a, out] if b is None else [a, b, out]
    bt = Batch(out.shape[:-2], tensors, [2] * len(tensors))
    o = bt.operands
    fb = (None, 0, 0, 0, 0) if b is None else _fields(o[1])
    call(getattr(_lib.lib(), family.entry), dev, dtype_code(dtype), *scalars, bt.n_outer, bt.n_inner,
         *_fields(o[0]), *fb, *_fields(o[-1]))
    bt.finish()


def _like(like, shape, dtype, dev):
    """a channel-first / matrix-first right-hand side hands its layout on to the result"""
    if (like is not None and tuple(like.shape) == tuple(shape) and not like.is_contiguous() and like.numel() > 0
            and 0 not in like.stride()):
        cand = torch.empty_like(like)
        if cand.stride() == like.stride():
            return cand
    return torch.empty(shape, dtype=dtype, device=dev)


def _blocks(k, cap):
    """the column blocks [c0, c1) of k columns at `cap` columns per launch"""
    return [(c0, min(c0 + cap, k)) for c0 in range(0, k, cap)]


def _kernel_solve(family, a, b, out=None, flag=None, rcond=None):
    """X = a^-1 b (a^+ b) on the kernels of `family`: a (..., m, n) in the family's range; b (..., m, k), or None
    for the identity where the family has one; forward only.  A k that fits one launch is one launch on a, b and
    out themselves; more columns are one launch per block of columns, on views of b and out."""
    dev, dtype = a.device, a.dtype
    m, n = a.shape[-2:]
    if b is None:
        k, batch = a.shape[family.identity], a.shape[:-2]
    else:
        k, batch = b.shape[-1], broadcast_shapes(a.shape[:-2], b.shape[:-2])
    shape = tuple(batch) + (n, k)
    if out is None:
        out = _like(b, shape, dtype, dev)
    elif tuple(out.shape) != shape or out.dtype != dtype or out.device != dev:
        raise ValueError(f'out= must be a {dtype} tensor of shape {shape} on {dev}')
    if out.numel() == 0:
        return out
    a = expand_batch(batch, a, 2)
    if b is not None:
        b = expand_batch(batch, b, 2)
        cap = _cap(family.cap, dtype, *family.dims(m, n))
        if k > cap:
            for c0, c1 in _blocks(k, cap):
                _launch(family, dev, dtype, family.scalars(m, n, c1 - c0, flag, rcond), a, b[..., c0:c1],
                        out[..., c0:c1])
            return out
    _launch(family, dev, dtype, family.scalars(m, n, k, flag, rcond), a, b, out)
    return out


def _svd_ok(a):
    return 0 < a.shape[-1] <= SVD_MAX_DIM and 0 < a.shape[-2] <= SVD_MAX_DIM


def _lstsq_ok(a):
    return SVD_MAX_DIM < a.shape[-2] <= LSTSQ_MAX_ROWS and 0 < a.shape[-1] <= LSTSQ_MAX_N


def _check_out(out, *tensors):
    if out is not None and torch.is_grad_enabled() and any(t.requires_grad for t in tensors + (out,)):
        raise RuntimeError('out= is not supported for tensors that require grad')


def _torch_lmdiv(a, b, method, rcond, out):
    """the reference's composition (sugar.py:123-137), on the device"""
    if method == 'lu':
        return torch.linalg.solve(a, b, out=out)
    if method == 'chol':
        return torch.cholesky_solve(b, torch.linalg.cholesky(a, upper=False), upper=False, out=out)
    if method == 'svd':
        u, s, v = torch.svd(a)
        return torch.matmul(v, u.transpose(-1, -2).matmul(b) / s[..., None], out=out)
    return torch.matmul(torch.linalg.pinv(a, rcond=rcond), b, out=out)


def kron2(a, b):
    """Kronecker product of two matrices, in the reference's layout (sugar.py:43-72).

    a : `(..., m, n)`, b : `(..., p, q)` -> `(..., p*m, q*n)` with
    `ab.reshape([P, M, Q, N])[p, m, q, n] == a[m, n] * b[p, q]` (not `torch.kron`'s block order)."""
    _, _, (a, b) = prepare(None, a, b, grad_ok=True)
    m, n = a.shape[-2:]
    p, q = b.shape[-2:]
    ab = b[..., :, None, :, None] * a[..., None, :, None, :]
    return ab.reshape(tuple(ab.shape[:-4]) + (m * p, n * q))


def lmdiv(a, b, method='lu', rcond=1e-15, out=None):
    """Left matrix division `A^-1 B` (sugar.py:75-137).

    a : `(..., m, n)`, b : `(..., m, k)` -> `(..., n, k)`; batch dims broadcast.
    method : `{'lu', 'chol', 'svd', 'pinv'}`; non-square `a` always takes `pinv`.
    `a` with m, n <= 8 runs a HIP kernel: elimination (`lu`), Cholesky from the lower triangle only (`chol`), or
    the Jacobi SVD (`svd`, `pinv`, every non-square `a`; forward only -- with a gradient: the torch composition).
    A square `a` of order 9..16 with `lu` / `chol` runs the row-per-lane kernel (`nfm_rowsolve`): the same
    contract -- lower triangle only and NaN records for `chol`, inf / NaN in a singular record for `lu`, every
    layout read in place, differentiable with `lu` -- and a column of the result does not depend on how many
    columns `b` has.  Order 17 and above take the torch composition.
    `pinv` drops the singular values `<= rcond sigma_max`; `svd` divides by every one of them.
    A tall `a` with 8 < m <= 4096 rows and n <= 8 columns runs the streaming least-squares kernel
    (`nfm_lstsq_solve`; forward only): exactly `pinv(a, rcond) @ b`, the minimum-norm least-squares solution.
    Rank deficiency is resolved by `rcond` alone, as in `torch.linalg.pinv`: at the default `rcond = 1e-15` a
    numerically rank-deficient float32 record is as meaningless here as it is there -- pass an `rcond` of the
    order of the data's precision for such fits.  Wide systems with more than 8 columns take the torch
    composition."""
    dev, dtype, (a, b) = prepare(None, a, b, grad_ok=True)
    _check_out(out, a, b)
    method = _method(method, a)
    if b.shape[-2] != a.shape[-2]:
        raise ValueError(f'system {tuple(a.shape[-2:])} and right-hand side {tuple(b.shape[-2:])} do not match')
    if method in _SVD_FLAGS:
        if needs_grad(a, b):
            return _torch_lmdiv(a, b, method, rcond, out)
        if method == 'pinv' and _lstsq_ok(a):
            return _kernel_solve(_LSTSQ, a, b, out, rcond=rcond)
        if not _svd_ok(a):
            return _torch_lmdiv(a, b, method, rcond, out)
        return _kernel_solve(_SVD, a, b, out, _SVD_FLAGS[method], rcond)
    family = _square_family(a.shape[-1])
    if family is None:
        return _torch_lmdiv(a, b, method, rcond, out)
    if needs_grad(a, b):
        if method == 'chol' and a.requires_grad:     # differentiates through the lower triangle only, like torch
            return _torch_lmdiv(a, b, method, rcond, None)
        from ._autograd import LmdivFn
        return LmdivFn.apply(a, b, _FLAGS[method])
    return _kernel_solve(family, a, b, out, _FLAGS[method])


def rmdiv(a, b, method='lu', rcond=1e-15, out=None):
    """Right matrix division `A B^-1` (sugar.py:140-191, as documented).

    a : `(..., k, m)`, b : `(..., m, m)` -> `(..., k, m)`: `X B = A` is `B^T X^T = A^T`, the kernel of `lmdiv`
    on views with row and column strides swapped.  (The reference's code returns `A^T B^-T`.)"""
    _, _, (a, b) = prepare(None, a, b, grad_ok=True)
    _check_out(out, a, b)
    x = lmdiv(b.transpose(-1, -2), a.transpose(-1, -2), method=method, rcond=rcond,
              out=None if out is None else out.transpose(-1, -2))
    return x.transpose(-1, -2) if out is None else out


def inv(a, method='lu', rcond=1e-15, out=None):
    """Matrix inversion (sugar.py:194-258).  `lu`: `batchinv` up to order 16; `chol`: the kernel of `lmdiv`
    against an identity generated in registers (order <= 16; 9..16 on the row-per-lane kernel), for every batch rank; `svd` / `pinv` and every
    non-square `a` (m, n <= 8): the Jacobi SVD kernel against the identity, `(..., n, m)`."""
    dev, dtype, (a,) = prepare(None, a, grad_ok=True)
    _check_out(out, a)
    method = _method(method, a)
    n = a.shape[-1]

    def give(res):
        if out is None:
            return res
        out.copy_(res)
        return out
    if method == 'lu':
        if 0 < n <= _lib.MAX_DIM:
            from .batched import batchinv
            return give(batchinv(a))
        return torch.linalg.inv(a, out=out)
    if method == 'chol':
        family = _square_family(n)
        if family is not None and not needs_grad(a):
            return _kernel_solve(family, a, None, out, _lib.SOLVE_CHOL)
        eye = torch.eye(n, dtype=dtype, device=dev)
        return torch.cholesky_solve(eye, torch.linalg.cholesky(a, upper=False), upper=False, out=out)
    if _svd_ok(a) and not needs_grad(a):
        return _kernel_solve(_SVD, a, None, out, _SVD_FLAGS[method], rcond)
    if method == 'svd':
        u, s, v = torch.svd(a)
        return give(v.matmul(u.transpose(-1, -2) / s[..., None]))
    return torch.linalg.pinv(a, rcond=rcond, out=out)


def matvec(mat, vec, out=None):
    """Matrix-vector product with broadcasting (sugar.py:261-287): `batchmatvec` up to 16 x 16, torch beyond."""
    _, _, (mat, vec) = prepare(None, mat, vec, grad_ok=True)
    _check_out(out, mat, vec)
    m, n = mat.shape[-2:]
    if 0 < m <= _lib.MAX_DIM and 0 < n <= _lib.MAX_DIM:
        from .batched import batchmatvec
        res = batchmatvec(mat, vec)
        if out is None:
            return res
        out.copy_(res)
        return out
    return torch.matmul(mat, vec.unsqueeze(-1), out=None if out is None else out.unsqueeze(-1)).squeeze(-1)


def solvevec(mat, vec, method='lu', rcond=1e-15, out=None):
    """Left matrix-vector division `A^-1 b` (sugar.py:290-341): `lmdiv` with one column, on views -- a tall `mat`
    (8 < m <= 4096 rows, n <= 8 columns) is the least-squares fit `pinv(mat, rcond) @ vec` on the streaming kernel,
    rank deficiency resolved by `rcond` alone."""
    vec = torch.as_tensor(vec)
    return lmdiv(mat, vec.unsqueeze(-1), method=method, rcond=rcond,
                 out=None if out is None else out.unsqueeze(-1)).squeeze(-1)


def outer(a, b, out=None):
    """Outer product `a b^T` of two batched vectors (sugar.py:344-375)."""
    _, _, (a, b) = prepare(None, a, b, grad_ok=True)
    return torch.matmul(a.unsqueeze(-1), b.unsqueeze(-2), out=out)


def trace(a, keepdim=False):
    """Batched trace (sugar.py:378-399); `keepdim` keeps two singleton dims."""
    _, _, (a,) = prepare(None, a, grad_ok=True)
    t = torch.diagonal(a, 0, -1, -2).sum(-1)
    return t[..., None, None] if keepdim else t


def dot(a, b, keepdim=False, out=None):
    """Batched dot product of two vectors (sugar.py:402-453)."""
    _, _, (a, b) = prepare(None, a, b, grad_ok=True)
    if out is not None:
        out = out[..., None] if keepdim else out[..., None, None]
    res = torch.matmul(a.unsqueeze(-2), b.unsqueeze(-1), out=out)
    return res[..., 0] if keepdim else res[..., 0, 0]


def mdot(a, b, keepdim=False, out=None):
    """Frobenius inner product of two matrices (sugar.py:456-500)."""
    _, _, (a, b) = prepare(None, a, b, grad_ok=True)
    flat = tuple(a.shape[:-2]) + (-1,)
    if out is not None and keepdim:
        out = out.squeeze(-1).squeeze(-1)
    res = dot(a.reshape(flat), b.reshape(flat), out=out)
    return res[..., None, None] if keepdim else res


def is_orthonormal(basis, return_matrix=False):
    """Is `basis` (F, N, [M]) an orthonormal basis?  Optionally also the (F, F) matrix of inner products
    (sugar.py:503-535)."""
    _, _, (basis,) = prepare(None, basis, grad_ok=True)
    flat = basis.reshape(basis.shape[0], -1)
    mat = flat @ flat.transpose(0, 1)
    mat = torch.triu(mat) + torch.triu(mat, 1).transpose(0, 1)       # the reference mirrors the upper triangle
    check = torch.allclose(mat, torch.eye(basis.shape[0], dtype=basis.dtype, device=basis.device))
    return (check, mat) if return_matrix else check


def round(t, decimals=0):
    """Round to the given number of decimals (sugar.py:538-553)."""
    _, _, (t,) = prepare(None, t, grad_ok=True)
    return torch.round(t * 10 ** decimals) / (10 ** decimals)
