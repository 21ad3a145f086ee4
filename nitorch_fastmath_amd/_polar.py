"""Singular value and polar decompositions of small square matrices in plain torch: the route of `batched.batchsvdvals`,
`batchsvd` and `batchpolar` for the orders that have no kernel (`nfm_polar_max_order`) and for CPU tensors.  Private
and device-agnostic.

Forward: `torch.linalg.svd` / `svdvals`; R = U Vh, P = Vh^T diag(S) Vh (mirrored exactly).
Backward of the polar decomposition: the form of the kernel (csrc/nfm_polar_ops.hpp), with B = U^T gR V and
C = V^T sym(gP) V: U X V^T, X_ij = ((B - B^T)_ij + 2 s_i C_ij) / (s_i + s_j) -- NOT torch's own `svd` backward, which
divides by s_i^2 - s_j^2 and is infinite or NaN at repeated singular values (an isotropic Jacobian).  Same rules as the
kernels: a record with an entry that is not finite is NaN in every component of every result and of the gradient; a
record with two numerically null singular values (s <= n eps |A|_F) and a non-zero gR has a NaN gradient, and its gP
part is finite.
"""
import torch
from ._autograd import _small_matmul as _mm          # broadcast multiply-adds: the same bits at every batch size


def _clean(a):
    """(c a, c, mask of the bad records): the bad records replaced by the identity (LAPACK raises on NaN), every
    record scaled by a power of two c (..., 1, 1) to max |a| in [0.5, 1) as the kernels do -- exact, and the
    batched SVD of the device is not accurate at 2^+-300"""
    bad = ~torch.isfinite(a).flatten(-2).all(-1)
    eye = torch.eye(a.shape[-1], dtype=a.dtype, device=a.device)
    a = torch.where(bad[..., None, None], eye, a)
    _, e = torch.frexp(a.abs().flatten(-2).amax(-1))
    lim = 120 if a.dtype == torch.float32 else 1000
    c = torch.ldexp(torch.ones_like(a[..., 0, 0]), -e.clamp(-lim, lim))[..., None, None]
    return a * c, c, bad


def _nan_where(bad, x):
    return torch.where(bad.reshape(bad.shape + (1,) * (x.dim() - bad.dim())), torch.full_like(x, float('nan')), x)


def svdvals(a):
    a, c, bad = _clean(a)
    return _nan_where(bad, torch.linalg.svdvals(a) / c[..., 0])


def svd(a):
    a, c, bad = _clean(a)
    U, S, Vh = torch.linalg.svd(a)
    return _nan_where(bad, U), _nan_where(bad, S / c[..., 0]), _nan_where(bad, Vh)


def _factors(a, svd_fn):
    """U, S, Vh, c, bad with c a = U diag(S) Vh on the good records.  `svd_fn`: the SVD kernel of the facade, for the
    orders it covers and the composition here does not (it scales and flags the bad records itself: c = 1); its
    results are made contiguous, so that the products below see the same operands whatever the layout of `a`."""
    if svd_fn is None:
        a, c, bad = _clean(a)
        return torch.linalg.svd(a) + (c, bad)
    U, S, Vh = svd_fn(a)
    bad = ~torch.isfinite(S).all(-1)
    eye = torch.eye(a.shape[-1], dtype=a.dtype, device=a.device)
    U, Vh = (torch.where(bad[..., None, None], eye, x).contiguous() for x in (U, Vh))
    S = torch.where(bad[..., None], torch.ones_like(S), S).contiguous()
    return U, S, Vh, torch.ones_like(S[..., :1, None]), bad


def polar(a, svd_fn=None):
    U, S, Vh, c, bad = _factors(a, svd_fn)
    P = _mm(Vh.transpose(-1, -2) * (S / c[..., 0])[..., None, :], Vh)
    P = torch.triu(P) + torch.triu(P, 1).transpose(-1, -2)
    return _nan_where(bad, _mm(U, Vh)), _nan_where(bad, P)


def svdvals_backward(a, g):
    a, _, bad = _clean(a)
    U, _, Vh = torch.linalg.svd(a)
    return _nan_where(bad, _mm(U * g[..., None, :], Vh))


def polar_backward(a, gr, gp, svd_fn=None):
    # S is c sigma: 1 / (sigma_i + sigma_j) = c / (S_i + S_j), and the ratios are free of the scale
    U, S, Vh, c, bad = _factors(a, svd_fn)
    n = a.shape[-1]
    V = Vh.transpose(-1, -2)
    fro = S.square().sum(-1, keepdim=True).sqrt()
    nul = S <= n * torch.finfo(a.dtype).eps * fro
    both = nul[..., :, None] & nul[..., None, :]
    den = torch.where(both, torch.ones_like(fro)[..., None], S[..., :, None] + S[..., None, :])
    X = torch.zeros_like(a)
    if gr is not None:
        gr = gr.expand(a.shape).contiguous()
        B = _mm(_mm(U.transpose(-1, -2), gr), V)
        X = X + torch.where(both, torch.zeros_like(B), (B - B.transpose(-1, -2)) * (c / den))
        bad = bad | ((nul.sum(-1) >= 2) & (gr != 0).flatten(-2).any(-1))
    if gp is not None:
        gp = gp.expand(a.shape).contiguous()
        C = _mm(_mm(Vh, 0.5 * (gp + gp.transpose(-1, -2))), V)
        X = X + torch.where(both, torch.ones_like(C), 2 * S[..., :, None] / den) * C
    return _nan_where(bad, _mm(_mm(U, X), Vh))
