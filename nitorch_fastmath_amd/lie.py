"""
Matrix exponential of small matrices and its derivatives on MI355X -- drop-in for
`nitorch_fastmath.lie.expm` / `expm_derivatives` (`lie.py:5-8`, `_impl/expm.py`).

One matrix per lane (`nfm_lie.hip`): per-matrix scaling and squaring around the reference's
Taylor series (quirks Q17-Q19 in DESIGN.md section 2).  Kernels: the exponential at float32
orders 1..8 and float64 orders 1..7, its first and second Frechet derivatives at orders 1..4.
Every other order takes a torch route on the device: `torch.linalg.matrix_exp`, and for the
derivatives the block identities

    L(X, A)     = expm([[X, A], [0, X]])[:D, D:]
    L2(X, A, B) = expm([[X, A, B, 0], [0, X, 0, B], [0, 0, X, A], [0, 0, 0, X]])[:D, 3D:]

`max_order` and `tol` do not apply on that route (matrix_exp picks its own degree).
`logm` and `meanm` are not names of this module: they live in `nitorch_fastmath_amd.logm`.
"""
__all__ = ['expm', 'expm_derivatives']
import torch
from . import _lib
from ._dispatch import Batch, broadcast_shapes, expand_batch, launch, needs_grad, no_grad_required, prepare

FORWARD_MAX = {torch.float32: 8, torch.float64: 7}   # orders with an expm kernel (include/nfm_hip.h)
FRECHET_MAX = 4                                       # orders with a Frechet kernel


def __getattr__(name):
    if name in ('logm', 'meanm'):
        raise AttributeError(f'nitorch_fastmath_amd.lie does not provide {name}: import it from '
                             f'nitorch_fastmath_amd.logm (`from nitorch_fastmath_amd.logm import {name}`)')
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


def _compose(X, basis):
    """M = sum_f x_f B_f (`_impl/expm.py:140-145`), broadcasting like the reference"""
    if X.shape[-1] != basis.shape[-3]:
        raise ValueError(f'{X.shape[-1]} parameters for a basis of {basis.shape[-3]} matrices')
    return torch.einsum('...f,...fij->...ij', X, basis)


def _limits(max_order, tol):
    max_order = int(max(min(int(max_order), 2 ** 31 - 1), -(2 ** 31)))
    tol = float(tol)
    if not tol >= 0:
        raise ValueError(f'tol must be >= 0, got {tol}')
    return max_order, tol


def _expm(M, max_order, tol):
    """expm of a (..., D, D) GPU tensor (no autograd): the kernel, or matrix_exp above its orders"""
    D = M.shape[-1]
    if M.shape[-2] != D:
        raise ValueError(f'expected square matrices, got {tuple(M.shape[-2:])}')
    if D > FORWARD_MAX[M.dtype]:
        return torch.linalg.matrix_exp(M)
    dev = M.device
    batch = M.shape[:-2]
    out = torch.empty(tuple(batch) + (D, D), dtype=M.dtype, device=dev)
    b = Batch(batch, [M, out], [2, 2])
    launch(_lib.lib().nfm_lie_expm, dev, M.dtype, (D, max_order, tol), b)
    return out


def _frechet_torch(M, A, B=None):
    D = M.shape[-1]
    batch = broadcast_shapes(M.shape[:-2], A.shape[:-2], *(() if B is None else (B.shape[:-2],)))
    k = 2 if B is None else 4
    Z = M.new_zeros(tuple(batch) + (k * D, k * D))
    for q in range(k):
        Z[..., q * D:(q + 1) * D, q * D:(q + 1) * D] = M
    if B is None:
        Z[..., :D, D:] = A
        return torch.linalg.matrix_exp(Z)[..., :D, D:].contiguous()
    Z[..., :D, D:2 * D] = A
    Z[..., :D, 2 * D:3 * D] = B
    Z[..., D:2 * D, 3 * D:] = B
    Z[..., 2 * D:3 * D, 3 * D:] = A
    return torch.linalg.matrix_exp(Z)[..., :D, 3 * D:].contiguous()


def _frechet(M, A, B, max_order, tol):
    """L(M, A) (B None) or L2(M, A, B), broadcast over the batch dims (no autograd)"""
    D = M.shape[-1]
    if D > FRECHET_MAX:
        return _frechet_torch(M, A, B)
    dev = M.device
    ops = [M, A] + ([] if B is None else [B])
    batch = broadcast_shapes(*[t.shape[:-2] for t in ops])
    out = torch.empty(tuple(batch) + (D, D), dtype=M.dtype, device=dev)
    b = Batch(batch, [expand_batch(batch, t, 2) for t in ops] + [out], [2] * (len(ops) + 1))
    launch(_lib.lib().nfm_lie_expm_frechet, dev, M.dtype, (D, max_order, tol), b, (0, 1, None if B is None else 2, -1))
    return out


def expm(X, basis=None, max_order=10000, tol=1e-32):
    """Matrix exponential.  Replaces `_impl/expm.py:15-49` (same signature, broadcasting and autograd).

    X : `(..., D, D)` log-matrix, or `(..., F)` parameters when `basis` `(..., F, D, D)` is given.
    max_order, tol : the series stops at the degree whose term bound passes the reference's test
        `sum(T_n^2) <= D^2 tol` (at most `max_order`), after scaling by 2^-s.  The derivative
        kernels (the backward here, dX / dB / hX of `expm_derivatives`) run one (L) or two (L2) degrees further,
        still at most `max_order`: their terms lag the exponential's by that many powers of the matrix.
    Returns `(..., D, D)`.  Differentiable: the backward runs the Frechet kernel, L(M^T, G).
    """
    from ._autograd import ExpmFn
    max_order, tol = _limits(max_order, tol)
    _, _, (X, basis) = prepare(None, X, basis, grad_ok=True)
    M = X if basis is None else _compose(X, basis)
    if M.shape[-2] != M.shape[-1]:
        raise ValueError(f'expected square matrices, got {tuple(M.shape[-2:])}')
    if needs_grad(M):
        if M.shape[-1] > FORWARD_MAX[M.dtype]:
            return torch.linalg.matrix_exp(M)
        return ExpmFn.apply(M, max_order, tol)
    return _expm(M, max_order, tol)


def expm_derivatives(X, basis=None, grad_X=False, grad_basis=False, hess_X=False, max_order=10000, tol=1e-32):
    """Matrix exponential and its derivatives.  Replaces `_impl/expm.py:52-199` (same signature and output
    shapes and orderings; forward-only, like every facade function that is not `expm`).

    X : `(..., D, D)`, or `(..., F)` with `basis` `(..., F, D, D)`; without a basis F = D^2 and the basis is
        one-hot in row-major order (f = i D + j).
    Returns E `(..., D, D)`, then if asked for: dX `(..., F, D, D)`, dX[f] = L(M, B_f);
    dB `(..., F, D, D, D, D)`, dB[f, i, j] = x_f L(M, e_ij); hX `(..., F, F, D, D)`, hX[f, g] = L2(M, B_f, B_g)
    (also for a batched X, where the reference raises: Q19).
    """
    max_order, tol = _limits(max_order, tol)
    dev, dtype, (X, basis) = prepare(None, X, basis, grad_ok=True)
    no_grad_required(X, basis)
    if basis is None:
        D = X.shape[-1]
        if X.shape[-2] != D:
            raise ValueError(f'expected square matrices, got {tuple(X.shape[-2:])}')
        M = X
        param = X.reshape(X.shape[:-2] + (D * D,))
    else:
        D = basis.shape[-1]
        M = _compose(X, basis)
        param = X
    batch = M.shape[:-2]
    onehot = None
    if basis is None or grad_basis:
        onehot = torch.eye(D * D, dtype=dtype, device=dev).reshape(D * D, D, D)
    if basis is None:
        basis = onehot
    F = basis.shape[-3]
    out = [_expm(M, max_order, tol)]
    Mx = M.unsqueeze(-3)                     # (..., 1, D, D): stride 0 along the basis
    dX = None
    if grad_X or (grad_basis and basis is onehot):
        dX = _frechet(Mx, basis, None, max_order, tol)
    if grad_X:
        out.append(dX)
    if grad_basis:
        Lij = dX if basis is onehot else _frechet(Mx, onehot, None, max_order, tol)   # (..., D*D, D, D)
        Lij = Lij.reshape(tuple(batch) + (1, D, D, D, D))
        p = param.reshape(tuple(param.shape) + (1, 1, 1, 1))
        out.append((p * Lij).contiguous())
    if hess_X:
        hX = torch.empty(tuple(batch) + (F, F, D, D), dtype=dtype, device=dev)
        for f in range(F):                   # L2 is symmetric in its directions: g >= f only
            h = _frechet(Mx, basis[..., f:f + 1, :, :], basis[..., f:, :, :], max_order, tol)
            hX[..., f, f:, :, :] = h
            hX[..., f + 1:, f, :, :] = h[..., 1:, :, :]
        out.append(hX)
    return out[0] if len(out) == 1 else out
