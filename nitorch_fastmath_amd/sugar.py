"""
"Syntactic sugar" linear algebra on MI355X -- drop-in for `nitorch_fastmath.sugar` (`sugar.py`).

`lmdiv`, `rmdiv`, `solvevec` and `inv` on matrices of at most 8 rows and columns run one lane-per-system HIP
kernel: `nfm_sugar_solve` for `lu` / `chol` on square matrices (Gaussian elimination with partial pivoting on
`[A | B]`, or Cholesky from the lower triangle), `nfm_svd_solve` for `svd` / `pinv` and for every non-square
system (one-sided Jacobi SVD on the rows of `[A | B]`: least squares for m > n, minimum norm for m < n).  Tall
least-squares systems -- more than 8 rows (up to 4096), at most 8 columns: a model fit per voxel -- run
`nfm_lstsq_solve`: the rows of `[A | B]` stream once past an n x n triangle in the lane's registers (Givens
rotations) and the same Jacobi routine finishes on it, `pinv(a, rcond) @ b` in one launch.  The
reference runs torch's batched LU / SVD, which are slow on tiny matrices.  Transposed, broadcast, padded and
channel-first operands are read in place.  More than 8 columns, square orders above 8, `inv` of a tall matrix,
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
import torch
from . import _lib
from ._dispatch import Batch, broadcast_shapes, call, dtype_code, expand_batch, needs_grad, prepare

MAX_ORDER = _lib.SOLVE_MAX_DIM
_FLAGS = {'lu': _lib.SOLVE_LU, 'chol': _lib.SOLVE_CHOL}
_SVD_FLAGS = {'svd': _lib.SVD_PLAIN, 'pinv': _lib.SVD_PINV}
SVD_MAX_DIM = _lib.SVD_MAX_DIM
LSTSQ_MAX_ROWS, LSTSQ_MAX_N = _lib.LSTSQ_MAX_ROWS, _lib.LSTSQ_MAX_N
_caps = {}
_svd_caps = {}
_lstsq_caps = {}


def max_cols(dtype, n):
    """Columns of `b` one launch takes at order `n` (the library's table, `nfm_sugar_max_cols`)."""
    key = (dtype, n)
    if key not in _caps:
        _caps[key] = int(_lib.lib().nfm_sugar_max_cols(dtype_code(dtype), n))
    return _caps[key]


def svd_max_cols(dtype, m, n):
    """Columns of `b` one launch takes for an `m x n` system (the library's table, `nfm_svd_max_cols`)."""
    key = (dtype, m, n)
    if key not in _svd_caps:
        _svd_caps[key] = int(_lib.lib().nfm_svd_max_cols(dtype_code(dtype), m, n))
    return _svd_caps[key]


def lstsq_max_cols(dtype, n):
    """Columns of `b` one launch takes for a tall system of `n` columns (the library's table, `nfm_lstsq_max_cols`)."""
    key = (dtype, n)
    if key not in _lstsq_caps:
        _lstsq_caps[key] = int(_lib.lib().nfm_lstsq_max_cols(dtype_code(dtype), n))
    return _lstsq_caps[key]


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


def _launch(dev, dtype, n, k, flag, a, b, out):
    """one nfm_sugar_solve call; a / b / out share their batch dims (views); b None: the identity"""
    batch = out.shape[:-2]
    tensors = [a, out] if b is None else [a, b, out]
    bt = Batch(batch, tensors, [2] * len(tensors))
    o = bt.operands
    fb = (None, 0, 0, 0, 0) if b is None else _fields(o[1])
    call(_lib.lib().nfm_sugar_solve, dev, dtype_code(dtype), n, k, flag, bt.n_outer, bt.n_inner,
         *_fields(o[0]), *fb, *_fields(o[-1]))
    bt.finish()


def _svd_launch(dev, dtype, m, n, k, flag, rcond, a, b, out):
    """one nfm_svd_solve call; a / b / out share their batch dims (views); b None: the identity"""
    batch = out.shape[:-2]
    tensors = [a, out] if b is None else [a, b, out]
    bt = Batch(batch, tensors, [2] * len(tensors))
    o = bt.operands
    fb = (None, 0, 0, 0, 0) if b is None else _fields(o[1])
    call(_lib.lib().nfm_svd_solve, dev, dtype_code(dtype), m, n, k, flag, float(rcond), bt.n_outer, bt.n_inner,
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


def _solve(a, b, flag, out=None):
    """X = a^-1 b on the kernel: a (..., n, n), n <= 8; b (..., n, k) or None (identity); forward only.
    More columns than one launch takes: one launch per block of columns, on views of b and out."""
    dev, dtype = a.device, a.dtype
    n = a.shape[-1]
    k = n if b is None else b.shape[-1]
    batch = a.shape[:-2] if b is None else broadcast_shapes(a.shape[:-2], b.shape[:-2])
    shape = tuple(batch) + (n, k)
    if out is None:
        out = _like(b, shape, dtype, dev)
    elif tuple(out.shape) != shape or out.dtype != dtype or out.device != dev:
        raise ValueError(f'out= must be a {dtype} tensor of shape {shape} on {dev}')
    if out.numel() == 0:
        return out
    a = expand_batch(batch, a, 2)
    if b is None:
        _launch(dev, dtype, n, n, flag, a, None, out)
        return out
    b = expand_batch(batch, b, 2)
    cap = max_cols(dtype, n)
    for c0 in range(0, k, cap):
        c1 = min(c0 + cap, k)
        if c0 == 0 and c1 == k:
            _launch(dev, dtype, n, k, flag, a, b, out)
        else:
            _launch(dev, dtype, n, c1 - c0, flag, a, b[..., c0:c1], out[..., c0:c1])
    return out


def _svd_ok(a):
    return 0 < a.shape[-1] <= SVD_MAX_DIM and 0 < a.shape[-2] <= SVD_MAX_DIM


def _svd_solve(a, b, flag, rcond, out=None):
    """X = a^+ b on the kernel: a (..., m, n), m, n <= 8; b (..., m, k) or None (identity, k = m); forward only.
    Column blocks as in `_solve`."""
    dev, dtype = a.device, a.dtype
    m, n = a.shape[-2:]
    k = m if b is None else b.shape[-1]
    batch = a.shape[:-2] if b is None else broadcast_shapes(a.shape[:-2], b.shape[:-2])
    shape = tuple(batch) + (n, k)
    if out is None:
        out = _like(b, shape, dtype, dev)
    elif tuple(out.shape) != shape or out.dtype != dtype or out.device != dev:
        raise ValueError(f'out= must be a {dtype} tensor of shape {shape} on {dev}')
    if out.numel() == 0:
        return out
    a = expand_batch(batch, a, 2)
    if b is None:
        _svd_launch(dev, dtype, m, n, m, flag, rcond, a, None, out)
        return out
    b = expand_batch(batch, b, 2)
    cap = svd_max_cols(dtype, m, n)
    for c0 in range(0, k, cap):
        c1 = min(c0 + cap, k)
        if c0 == 0 and c1 == k:
            _svd_launch(dev, dtype, m, n, k, flag, rcond, a, b, out)
        else:
            _svd_launch(dev, dtype, m, n, c1 - c0, flag, rcond, a, b[..., c0:c1], out[..., c0:c1])
    return out


def _lstsq_ok(a):
    return SVD_MAX_DIM < a.shape[-2] <= LSTSQ_MAX_ROWS and 0 < a.shape[-1] <= LSTSQ_MAX_N


def _lstsq_launch(dev, dtype, m, n, k, rcond, a, b, out):
    """one nfm_lstsq_solve call; a / b / out share their batch dims (views)"""
    bt = Batch(out.shape[:-2], [a, b, out], [2, 2, 2])
    o = bt.operands
    call(_lib.lib().nfm_lstsq_solve, dev, dtype_code(dtype), m, n, k, float(rcond), bt.n_outer, bt.n_inner,
         *_fields(o[0]), *_fields(o[1]), *_fields(o[2]))
    bt.finish()


def _lstsq_solve(a, b, rcond, out=None):
    """X = pinv(a, rcond) b on the streaming kernel: a (..., m, n), 8 < m <= 4096, n <= 8; b (..., m, k); forward
    only.  Column blocks as in `_solve`."""
    dev, dtype = a.device, a.dtype
    m, n = a.shape[-2:]
    k = b.shape[-1]
    batch = broadcast_shapes(a.shape[:-2], b.shape[:-2])
    shape = tuple(batch) + (n, k)
    if out is None:
        out = _like(b, shape, dtype, dev)
    elif tuple(out.shape) != shape or out.dtype != dtype or out.device != dev:
        raise ValueError(f'out= must be a {dtype} tensor of shape {shape} on {dev}')
    if out.numel() == 0:
        return out
    a, b = expand_batch(batch, a, 2), expand_batch(batch, b, 2)
    cap = lstsq_max_cols(dtype, n)
    for c0 in range(0, k, cap):
        c1 = min(c0 + cap, k)
        if c0 == 0 and c1 == k:
            _lstsq_launch(dev, dtype, m, n, k, rcond, a, b, out)
        else:
            _lstsq_launch(dev, dtype, m, n, c1 - c0, rcond, a, b[..., c0:c1], out[..., c0:c1])
    return out


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
            return _lstsq_solve(a, b, rcond, out)
        if not _svd_ok(a):
            return _torch_lmdiv(a, b, method, rcond, out)
        return _svd_solve(a, b, _SVD_FLAGS[method], rcond, out)
    if a.shape[-1] > MAX_ORDER or a.shape[-1] == 0:
        return _torch_lmdiv(a, b, method, rcond, out)
    if needs_grad(a, b):
        if method == 'chol' and a.requires_grad:     # differentiates through the lower triangle only, like torch
            return _torch_lmdiv(a, b, method, rcond, None)
        from ._autograd import LmdivFn
        return LmdivFn.apply(a, b, _FLAGS[method])
    return _solve(a, b, _FLAGS[method], out)


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
    against an identity generated in registers (order <= 8), for every batch rank; `svd` / `pinv` and every
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
        if 0 < n <= MAX_ORDER and not needs_grad(a):
            return _solve(a, None, _lib.SOLVE_CHOL, out)
        eye = torch.eye(n, dtype=dtype, device=dev)
        return torch.cholesky_solve(eye, torch.linalg.cholesky(a, upper=False), upper=False, out=out)
    if _svd_ok(a) and not needs_grad(a):
        return _svd_solve(a, None, _SVD_FLAGS[method], rcond, out)
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
