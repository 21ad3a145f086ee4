"""
Batched determinant / inverse / matrix-vector product for large batches of small
general matrices on MI355X -- drop-in for `nitorch_fastmath.batched`
(`batched.py:16-17`, `_impl/batched.py`).

The reference has closed forms for 1x1..3x3 on the GPU and falls back to torch
(LAPACK / MAGMA-style batched LU) otherwise; here every order 1..16 is one
lane-per-matrix HIP kernel: adjugate closed forms up to 3x3, in-register
Gauss-Jordan / LU with partial pivoting up to 8x8, LDS-resident LU up to 16x16.

EXTENSION (not in the reference): `batchsvdvals`, `batchsvd` and `batchpolar`, the singular value and polar
decompositions of general square matrices up to 8x8 by a one-sided Jacobi SVD in the registers of one lane.
"""
__all__ = ['batchmatvec', 'batchdet', 'batchinv', 'batchsvdvals', 'batchsvd', 'batchpolar']
import torch
from . import _lib
from ._dispatch import Batch, broadcast_shapes, expand_batch, launch, max_order, needs_grad, prepare


def _like_or_contiguous(like, shape, dtype, dev):
    """Matrix-first / channel-first operands of the output's shape hand their layout on (the call
    then runs through the SoA tiles end to end); everything else gets a contiguous output."""
    if (like is not None and tuple(like.shape) == tuple(shape) and not like.is_contiguous()
            and like.stride(-1) != 1 and like.numel() > 0 and 0 not in like.stride()):
        cand = torch.empty_like(like, dtype=dtype)
        if cand.stride() == like.stride():
            return cand
    return torch.empty(shape, dtype=dtype, device=dev)


def batchdet(a):
    """Batched determinant for large batches of small matrices.

    a : `(..., n, n) tensor` -> `(...) tensor`.  Replaces `_impl/batched.py:35-63`.
    """
    from ._autograd import BatchDetFn
    if needs_grad(a):
        return BatchDetFn.apply(torch.as_tensor(a))
    dev, dtype, (a,) = prepare(None, a)
    n = a.shape[-1]
    assert a.shape[-2] == n, 'Expected square matrices'
    if n > _lib.MAX_DIM:          # the reference's own route for every order (`_impl/batched.py:53-54`), on the device
        return torch.linalg.det(a)
    batch = a.shape[:-2]
    out = torch.empty(batch, dtype=dtype, device=dev)
    b = Batch(batch, [a, out], [2, 0], pack=n > 8)
    launch(_lib.lib().nfm_batch_det, dev, dtype, (n,), b)
    return out


def batchinv(a, perturb=False):
    """Batched inversion for large batches of small matrices.

    a : `(..., n, n) tensor` -> `(..., n, n) tensor`.  Replaces `_impl/batched.py:101-130`.

    perturb : bool, default=False
        Reproduce the TorchScript closed forms `inv2`/`inv3` exactly, including their
        determinant perturbation `(max|a| - min|a|) * 1e-12` (`_impl/batched.py:74-76`).
        The default matches the reference's CPU path (`a.inverse()`).
    """
    from ._autograd import BatchInvFn
    if needs_grad(a):
        return BatchInvFn.apply(torch.as_tensor(a), bool(perturb))
    dev, dtype, (a,) = prepare(None, a)
    n = a.shape[-1]
    assert a.shape[-2] == n, 'Expected square matrices'
    if n > _lib.MAX_DIM:          # `a.inverse()` (`_impl/batched.py:119-120`), on the device
        return torch.linalg.inv(a)
    batch = a.shape[:-2]
    out = _like_or_contiguous(a if n <= 8 else None, tuple(batch) + (n, n), dtype, dev)
    b = Batch(batch, [a, out], [2, 2], pack=n > 8)
    launch(_lib.lib().nfm_batch_inv, dev, dtype, (n, _lib.FLAG_TS_PERTURB if perturb else 0), b)
    return out


def batchmatvec(mat, vec):
    """Batched matrix-vector product for large batches of small matrices.

    mat : `(..., m, n)`, vec : `(..., n)` -> `(..., m)`.  Replaces `_impl/batched.py:154-190`.
    """
    from ._autograd import BatchMatvecFn
    if needs_grad(mat, vec):
        return BatchMatvecFn.apply(torch.as_tensor(mat), torch.as_tensor(vec))
    dev, dtype, (mat, vec) = prepare(None, mat, vec)
    m, n = mat.shape[-2:]
    if vec.shape[-1] != n:
        raise ValueError(f'matrix {tuple(mat.shape[-2:])} and vector ({vec.shape[-1]},) do not match')
    batch = broadcast_shapes(mat.shape[:-2], vec.shape[:-1])
    out = _like_or_contiguous(vec if m == n else None, tuple(batch) + (m,), dtype, dev)
    b = Batch(batch, [expand_batch(batch, mat, 2), expand_batch(batch, vec, 1), out], [2, 1, 1])
    launch(_lib.lib().nfm_batch_matvec, dev, dtype, (m, n), b)
    return out


# ---------------------------------------------------------------- singular values, SVD, polar (extension)
# (dtype, op, n, channel_first) measured slower than the torch composition the call would otherwise take
# (profiles/polar_table.md): routed back to it.  None so far.
_POLAR_TORCH_ROUTE = frozenset()


def polar_max_order(dtype, op):
    """largest order with a kernel: the compiled table of the library (`nfm_polar_max_order`); `op` is one of
    'svdvals', 'svd', 'polar', 'polar_backward'"""
    code = {'svdvals': _lib.POLAR_SVDVALS, 'svd': _lib.POLAR_SVD, 'polar': _lib.POLAR_POLAR,
            'polar_backward': _lib.POLAR_POLAR_BACKWARD}[op]
    return max_order('nfm_polar_max_order', dtype, code)


def _channel_first(a):
    """the matrix dims outermost in memory and the batch dense behind them: `(n, n, *batch)` seen as `(*batch, n, n)`"""
    return (a.dim() > 2 and a.numel() > 0 and not a.is_contiguous() and a.stride(-1) != 1
            and a.movedim((-2, -1), (0, 1)).is_contiguous())


def _square(a):
    a = torch.as_tensor(a)
    if a.dim() < 2 or a.shape[-1] != a.shape[-2]:
        raise ValueError(f'expected square matrices (..., n, n), got {tuple(a.shape)}')
    if a.dtype not in (torch.float32, torch.float64):
        raise TypeError(f'nitorch_fastmath_amd supports float32 and float64 tensors, got {a.dtype}')
    return a


def _on_kernel(a, op):
    n = a.shape[-1]
    return (a.is_cuda and 1 <= n <= polar_max_order(a.dtype, op)
            and (a.dtype, op, n, _channel_first(a)) not in _POLAR_TORCH_ROUTE)


def _packed_launch(entry, a, ncomp):
    """one forward kernel: `a` read in place, one packed record of `ncomp` values per matrix; a channel-first
    operand gets a channel-first result"""
    dev, dtype, (a,) = prepare(None, a, grad_ok=True)
    n = a.shape[-1]
    batch = tuple(a.shape[:-2])
    if _channel_first(a):
        out = torch.empty((ncomp,) + batch, dtype=dtype, device=dev).movedim(0, -1)
    else:
        out = torch.empty(batch + (ncomp,), dtype=dtype, device=dev)
    launch(entry, dev, dtype, (n,), Batch(batch, [a, out], [2, 1]))
    return out


def _svdvals(a):
    if not _on_kernel(a, 'svdvals'):
        from . import _polar
        return _polar.svdvals(a)
    return _packed_launch(_lib.lib().nfm_batch_svdvals, a, a.shape[-1])


def _svd(a):
    if not _on_kernel(a, 'svd'):
        from . import _polar
        return _polar.svd(a)
    n = a.shape[-1]
    out = _packed_launch(_lib.lib().nfm_batch_svd, a, n + 2 * n * n)
    return (out[..., n:n + n * n].unflatten(-1, (n, n)), out[..., :n], out[..., n + n * n:].unflatten(-1, (n, n)))


def _svd_kernel(a):
    """the SVD kernel as the factorisation of the torch compositions, where it covers an order that the polar kernels
    do not (float64 8 x 8 forward, the larger orders of the backward kernel): the composition is then as accurate as
    the kernels, which `torch.linalg.svd` on the device is not on graded matrices"""
    return _svd if _on_kernel(a, 'svd') else None


def _polar_forward(a):
    if not _on_kernel(a, 'polar'):
        from . import _polar
        return _polar.polar(a, _svd_kernel(a))
    n = a.shape[-1]
    out = _packed_launch(_lib.lib().nfm_batch_polar, a, 2 * n * n)
    return out[..., :n * n].unflatten(-1, (n, n)), out[..., n * n:].unflatten(-1, (n, n))


def _polar_backward(a, gr, gp):
    """gradient of (R, P) = polar(a) with respect to `a`; `gr` / `gp` None: zeros"""
    if gr is None and gp is None:
        return torch.zeros_like(a)
    if not _on_kernel(a, 'polar_backward'):
        from . import _polar
        return _polar.polar_backward(a, gr, gp, _svd_kernel(a))
    dev, dtype, (a, gr, gp) = prepare(None, a, gr, gp, grad_ok=True)
    n = a.shape[-1]
    batch = a.shape[:-2]
    ga = _like_or_contiguous(a, tuple(a.shape), dtype, dev)
    ops = [a] + [expand_batch(batch, g, 2) for g in (gr, gp) if g is not None] + [ga]
    b = Batch(batch, ops, [2] * len(ops))
    slots = [0, None if gr is None else 1, None if gp is None else len(ops) - 2, len(ops) - 1]
    launch(_lib.lib().nfm_batch_polar_backward, dev, dtype, (n,), b, slots=slots)
    return ga


def batchsvdvals(a):
    """EXTENSION: singular values of large batches of small square matrices.

    a : `(..., n, n) tensor` -> `(..., n) tensor`, non-negative, in descending order.

    One lane per matrix: a one-sided Jacobi SVD in registers (`n <= 8`; `torch.linalg.svdvals` on the device above
    the compiled cap and for CPU tensors).  Contiguous, channel-first `(n, n, *batch)`, padded, offset and broadcast
    operands are read in place.  No host synchronisation and no exception for bad data: a matrix with an entry that
    is not finite gives NaN values, its neighbours do not notice; the call can be captured in a graph.
    Differentiable: the gradient is `U diag(g) Vh` (one SVD kernel in the backward pass).
    """
    a = _square(a)
    if needs_grad(a):
        from ._autograd import BatchSvdvalsFn
        return BatchSvdvalsFn.apply(a)
    return _svdvals(a)


def batchsvd(a):
    """EXTENSION: singular value decomposition of large batches of small square matrices.

    a : `(..., n, n) tensor` -> `(U, S, Vh)` with `a = U diag(S) Vh`, `S` non-negative and descending.

    `U` and `Vh` are orthogonal for every finite matrix, rank-deficient ones and the zero matrix included (the
    right singular vectors of a numerically null singular value are an orthonormal completion of the others).  The
    signs of paired columns, and the basis inside a repeated singular value, are not specified.  The three results
    are views of one packed record per matrix.  Layouts, bad data and graphs as `batchsvdvals`.

    There is NO kernel gradient for `U` and `Vh`: a call whose operand requires grad takes `torch.linalg.svd`,
    forward and backward, whose gradient is infinite or NaN at repeated singular values.  `batchsvdvals` and
    `batchpolar` have regular gradients of their own.
    """
    a = _square(a)
    if needs_grad(a):
        return tuple(torch.linalg.svd(a))
    return _svd(a)


def batchpolar(a, side='right'):
    """EXTENSION: polar decomposition of large batches of small square matrices.

    a : `(..., n, n) tensor` -> `(R, P)` with `a = R P` (`side='right'`) or `a = P R` (`side='left'`): `R` orthogonal,
    `P` symmetric (exactly equal mirrored entries) positive semi-definite.

    `R = U Vh` and `P = Vh^T diag(S) Vh` from the SVD in the lane's registers.  For a singular matrix `P` is still
    unique and `R` is one valid orthogonal factor (`U Vh` with the completed `Vh` of `batchsvd`).  `side='left'` is
    the right decomposition of the transposed view, transposed back.  Layouts, bad data and graphs as `batchsvdvals`.
    Orders that the SVD kernel covers and a polar kernel does not (`polar_max_order`: float64 8x8; the gradient at
    float32 8x8 and float64 6x6..8x8) run the SVD kernel and the same formulas as broadcast products in torch.

    Differentiable through one backward kernel that recomputes the decomposition: with `B = U^T gR V` and
    `C = V^T sym(gP) V`, the gradient is `U X V^T`, `X_ij = ((B - B^T)_ij + 2 s_i C_ij) / (s_i + s_j)` -- sums in the
    denominators, finite and accurate at repeated and clustered singular values (the identity transform).  A matrix
    of rank `<= n - 2`, where `R` is not differentiable, with a non-zero `gR` gets a NaN gradient; its `gP` part
    stays finite.
    """
    if side not in ('right', 'left'):
        raise ValueError(f"side must be 'right' or 'left', got {side!r}")
    a = _square(a)
    if side == 'left':
        r, p = batchpolar(a.transpose(-1, -2), 'right')
        return r.transpose(-1, -2), p
    if needs_grad(a):
        from ._autograd import BatchPolarFn
        return BatchPolarFn.apply(a)
    return _polar_forward(a)
