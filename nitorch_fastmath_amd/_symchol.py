"""Cholesky functions of compact symmetric matrices in plain torch: the route of `sym.sym_chol`, `sym_chol_apply`,
`sym_logdet`, `sym_mahalanobis` and `sym_gauss_logpdf` for the orders that have no kernel (`nfm_sym_chol_max_order`,
`nfm_sym_chol_grad_max_order`), and what the backward pass of `sym_chol` / `sym_chol_apply` differentiates when a second
derivative is asked for (`create_graph=True`: the backward kernels are differentiable once).
Private and device-agnostic: it runs on CPU tensors too when called directly (the host tests do).

compact -> full -> `torch.linalg.cholesky_ex` -> products and triangular solves, differentiated by torch.  The bad-record
rule of csrc/nfm_symchol_ops.hpp: a record with an entry (of the matrix or of the vector) that is not finite, or one
that `cholesky_ex` refuses (`info != 0`: a pivot that is not > 0), is NaN in every value of its result AND of its
gradient; it is factored as the identity, so its neighbours never see it.  No exception, no host synchronisation.
"""
import math
import torch
from ._symfun import order_of, pack, to_full

OPS = ('L', 'LT', 'Linv', 'LTinv')


def _eye(mat, M):
    e = torch.zeros(mat.shape[-1], dtype=mat.dtype, device=mat.device)
    e[:M] = 1
    return e


def _lower(mat, factored=False):
    """(M, L full lower, bad) of compact records `mat`; a bad record is factored as the identity"""
    M = order_of(mat.shape[-1])
    eye = _eye(mat, M)
    bad = ~torch.isfinite(mat).all(-1)
    if factored:
        bad = bad | ~(mat[..., :M] > 0).all(-1)
        return M, torch.tril(to_full(torch.where(bad[..., None], eye, mat), M)), bad
    safe = torch.where(bad[..., None], eye, mat)
    if not (torch.is_grad_enabled() and mat.requires_grad):
        # nothing to differentiate: one factorisation, the refused records replaced afterwards
        L, info = torch.linalg.cholesky_ex(to_full(safe, M))
        bad = bad | (info != 0)
        return M, torch.where(bad[..., None, None], torch.eye(M, dtype=mat.dtype, device=mat.device), L), bad
    # a gradient with respect to `mat` is wanted: the refused records are found first, so that the factorisation torch
    # differentiates sees the identity in their place and its backward stays finite
    with torch.no_grad():
        info = torch.linalg.cholesky_ex(to_full(safe, M)).info
    bad = bad | (info != 0)
    return M, torch.linalg.cholesky_ex(to_full(torch.where(bad[..., None], eye, mat), M)).L, bad


def _poison(res, bad, ncomp, *inputs):
    """NaN in every value of the bad records of `res`, and in every value of their gradients: the added term is NaN
    there with derivative NaN, and exactly zero with derivative zero elsewhere"""
    nan = torch.where(bad, float('nan'), 0.0).to(res.dtype)
    term = nan
    for t in inputs:
        if t is not None and t.requires_grad:
            term = term + nan * (t - t.detach()).sum(-1)
    return res + term[(...,) + (None,) * ncomp]


def _bad_vec(bad, vec):
    return bad | ~torch.isfinite(vec).all(-1)


def chol(mat):
    """(..., K) -> (..., K): the lower factor, L_ij (i >= j) where the compact layout stores (i, j)"""
    M, L, bad = _lower(mat)
    return _poison(pack(L.transpose(-1, -2), M), bad, 1, mat)


def chol_apply(mat, vec, op, factored=False):
    """L v, L^T v, L^-1 v or L^-T v, (..., N); `factored`: `mat` is the result of `chol`"""
    if op not in OPS:
        raise ValueError(f'op must be one of {OPS}, got {op!r}')
    M, L, bad = _lower(mat, factored)
    v = vec[..., None]
    if op == 'L':
        res = L @ v
    elif op == 'LT':
        res = L.transpose(-1, -2) @ v
    elif op == 'Linv':
        res = torch.linalg.solve_triangular(L, v, upper=False)
    else:
        res = torch.linalg.solve_triangular(L.transpose(-1, -2), v, upper=True)
    return _poison(res[..., 0], _bad_vec(bad, vec), 1, mat, vec)


def _logdet(L):
    return 2 * torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1)


def _maha2(L, vec):
    y = torch.linalg.solve_triangular(L, vec[..., None], upper=False)[..., 0]
    return (y * y).sum(-1)


def logdet(mat):
    """(..., K) -> (...): 2 sum_i log L_ii"""
    _, L, bad = _lower(mat)
    return _poison(_logdet(L), bad, 0, mat)


def mahalanobis(mat, vec, squared=True):
    """v^T A^-1 v = |L^-1 v|^2, or its root (gradient exactly zero where the distance is zero)"""
    _, L, bad = _lower(mat)
    q = _maha2(L, vec)
    if not squared:
        pos = q > 0
        q = torch.where(pos, torch.sqrt(torch.where(pos, q, torch.ones_like(q))), q * 0)
    return _poison(q, _bad_vec(bad, vec), 0, mat, vec)


def gauss_logpdf(mat, resid):
    """-(N log 2 pi + log det A + r^T A^-1 r) / 2"""
    M, L, bad = _lower(mat)
    res = -0.5 * (M * math.log(2 * math.pi) + _logdet(L) + _maha2(L, resid))
    return _poison(res, _bad_vec(bad, resid), 0, mat, resid)
