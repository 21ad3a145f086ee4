"""Sorted eigendecomposition of compact symmetric matrices in plain torch: the route of `sym.sym_eigvals` /
`sym.sym_eigh` for the orders that have no kernel (`nfm_sym_eigh_max_order`), at any order.  Private and
device-agnostic: it runs on CPU tensors too when called directly (the host tests do).

Forward: compact -> full -> `torch.linalg.eigh` -> the sort and the sign rule of csrc/nfm_symeig_ops.hpp.
Backward: S = V W V^T with W_kk = gl_k and W_kl = (B_kl - B_lk) / (2 (l_l - l_k)), B = V^T gV, under the same gap rule
as the kernels (a pair closer than 16 n eps max|l| gets W_kl = 0), NOT torch's own `eigh` backward, which divides by
l_l - l_k whatever it is.  A record with an entry that is not finite is NaN in every component of the values, the
vectors and the gradient.
"""
import torch
from torch.autograd.function import once_differentiable
from ._symfun import order_of, pack, to_full

ASCENDING, DESCENDING, ABS = range(3)      # include/nfm_hip.h: NFM_EIGH_*
GAP = 16.0                                 # the gap rule: |l_k - l_l| <= GAP n eps max|l|


def _sort_index(lam, order):
    """the permutation of the kernels' network: by the key, ties by the sign (of the key; of the value for 'abs')"""
    if order == ABS:
        key, tie = lam.abs(), torch.copysign(torch.ones_like(lam), lam)
    else:
        key = -lam if order == DESCENDING else lam
        tie = torch.copysign(torch.ones_like(lam), key)
    first = torch.sort(tie, dim=-1, stable=True).indices
    second = torch.sort(torch.gather(key, -1, first), dim=-1, stable=True).indices
    return torch.gather(first, -1, second)


def _fix_signs(V):
    """the component of largest magnitude of every column positive, the first such component among exact ties"""
    mag = V.abs()
    top = mag == mag.amax(-2, keepdim=True)
    top = top & (top.cumsum(-2) == 1)
    sign = torch.where((V * top).sum(-2, keepdim=True) < 0, -1.0, 1.0).to(V.dtype)
    return V * sign


def decompose(mat, order):
    """(M, values, vectors, bad): sorted and sign-fixed; a bad record is decomposed as the identity"""
    M = order_of(mat.shape[-1])
    bad = ~torch.isfinite(mat).all(-1)
    eye = torch.eye(M, dtype=mat.dtype, device=mat.device)
    full = torch.where(bad[..., None, None], eye, to_full(mat, M))
    lam, V = torch.linalg.eigh(full)
    idx = _sort_index(lam, order)
    lam = torch.gather(lam, -1, idx)
    V = torch.gather(V, -1, idx[..., None, :].expand(V.shape))
    return M, lam, _fix_signs(V), bad


def _nan_where(bad, x, ncomp):
    return torch.where(bad[(...,) + (None,) * ncomp], torch.full_like(x, float('nan')), x)


def forward(mat, order=ASCENDING, vectors=False):
    """(..., K) compact -> (..., M) values, and (..., M, M) vectors with `vectors`"""
    _, lam, V, bad = decompose(mat, order)
    lam = _nan_where(bad, lam, 1)
    return (lam, _nan_where(bad, V, 2)) if vectors else lam


def gap_weights(lam):
    """(..., M) -> (..., M, M): 1 / (l_l - l_k) at [k, l] under the gap rule, 0 on the diagonal"""
    M = lam.shape[-1]
    d = lam[..., None, :] - lam[..., :, None]
    tol = GAP * M * torch.finfo(lam.dtype).eps * lam.abs().amax(-1)
    close = d.abs() <= tol[..., None, None]
    return torch.where(close, torch.zeros_like(d), 1 / torch.where(close, torch.ones_like(d), d))


def backward(mat, glam, gvec, order=ASCENDING):
    """gradient with respect to the compact record for the cotangents of the values and / or of the vectors (either
    may be None), in the module's compact convention: S_ii and 2 S_ij"""
    _, lam, V, bad = decompose(mat, order)
    return backward_from(lam, V, bad, glam, gvec)


def backward_from(lam, V, bad, glam, gvec):
    """`backward` for a decomposition already at hand: the one the forward pass returned, so that the gradient belongs
    to the returned order and signs (a sign decided by a tie of magnitudes is not the same in two solvers)"""
    M = lam.shape[-1]
    Vt = V.transpose(-1, -2)
    W = torch.zeros_like(V)
    if gvec is not None:
        B = Vt @ gvec.expand(V.shape)
        W = 0.5 * (B - B.transpose(-1, -2)) * gap_weights(lam)
    if glam is not None:
        W = W + torch.diag_embed(glam.expand(lam.shape))
    out = pack(V @ W @ Vt, M, off=2.0)
    return _nan_where(bad, out, 1)


class SymEighFn(torch.autograd.Function):
    """differentiable once, with respect to `mat`; nothing but `mat` is saved"""

    @staticmethod
    def forward(ctx, mat, order, vectors):
        ctx.save_for_backward(mat)
        ctx.order = order
        ctx.set_materialize_grads(False)
        return forward(mat, order, vectors)

    @staticmethod
    @once_differentiable
    def backward(ctx, glam, gvec=None):
        (mat,) = ctx.saved_tensors
        if glam is None and gvec is None:
            return None, None, None
        return backward(mat, glam, gvec, ctx.order), None, None


def sym_eigh(mat, order=ASCENDING, vectors=True):
    return SymEighFn.apply(mat, order, vectors)
