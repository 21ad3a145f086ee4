"""Two-matrix spectral functions of compact symmetric matrices as a composition of single-matrix ones: the route of
`sym.sym_pencil_funm`, `sym_geneigvals` and `sym_dist` for the orders that have no kernel
(`nfm_sym_pencil_max_order`), for the gradients the kernels do not serve (the base of 'log' / 'exp', the
generalised eigenvalues), and the yardstick the fused kernels are measured against.  Private and device-agnostic:
on GPU tensors the spectral functions are `sym.sym_funm` (its kernels, its gradient), on CPU tensors the torch route
`_symfun.sym_funm` -- which is how the host tests check this module.

    S = sqrtm(A), R = rsqrtm(A), C = pack(R B R), G = pack(S f(C) S)

(on the pair divided by the power of two of A's scale, an exact operation that leaves C alone and scales G)

Every piece is differentiable and regular at repeated eigenvalues (closed-form divided differences), and each keeps
the NaN-record rule: a base that is not positive definite or an entry that is not finite gives a NaN record, its
neighbours do not notice.  The eigenvalues and the distance take `torch.linalg.eigvalsh` of C, whose gradient has
no denominators.
"""
import torch
from . import _symfun
from ._symfun import EXP, LOG, SQRT, RSQRT, POW, order_of, pack, to_full


def _funm(x, code, p=None):
    if x.is_cuda:
        from . import sym as S
        return S.sym_funm(x, ('exp', 'log', 'sqrt', 'rsqrt', 'pow')[code], p=p if code == POW else None)
    return _symfun.sym_funm(x, code, p, None)


def _pow2(base):
    """per record, the power of two s with max |A_ij| / s in [1, 2) (1 for a record of zeros or with an entry that is
    not finite; s itself is finite up to the top of the range): a constant of the graph.  C does not change when A and B are divided by it and G is homogeneous of degree one, so
    the chain runs on records of unit scale whatever the caller's units are (float32 fields scaled by 2^+-40 are past
    what the eigensolvers behind the torch route of sym_funm take)."""
    amax = base.detach().abs().amax(-1, keepdim=True)
    ok = torch.isfinite(amax) & (amax > 0)
    return torch.ldexp(torch.ones_like(amax), torch.frexp(torch.where(ok, amax, torch.ones_like(amax))).exponent - 1)


def whiten(base, mat):
    """(M, s, S, compact C = R B R) for compact base A and compact mat B, batch dims broadcast: s the power of two of
    A's scale, S = (A / s)^1/2, R = (A / s)^-1/2, C = R (B / s) R"""
    if base.shape[-1] != mat.shape[-1]:
        raise ValueError(f'base and mat have {base.shape[-1]} and {mat.shape[-1]} components')
    M = order_of(base.shape[-1])
    s = _pow2(base)
    base, mat = base / s, mat / s
    S, R = to_full(_funm(base, SQRT), M), to_full(_funm(base, RSQRT), M)
    C = R @ to_full(mat, M) @ R
    return M, s, S, pack((C + C.transpose(-1, -2)) / 2, M)


def pencil_funm(base, mat, code, p=None):
    """compact A^1/2 f(A^-1/2 B A^-1/2) A^1/2"""
    if code not in (EXP, LOG, SQRT, RSQRT, POW):
        raise ValueError('a pencil function is one of exp, log, sqrt, rsqrt, pow')
    M, s, S, C = whiten(base, mat)
    G = S @ to_full(_funm(C, code, p), M) @ S
    return pack((G + G.transpose(-1, -2)) / 2, M) * s


def geneigvals(base, mat):
    """the eigenvalues of B x = mu A x, ascending; NaN for a bad record"""
    M, _, _, C = whiten(base, mat)
    bad = ~torch.isfinite(C).all(-1)
    eye = torch.eye(M, dtype=C.dtype, device=C.device)
    mu = torch.linalg.eigvalsh(torch.where(bad[..., None, None], eye, to_full(C, M)))
    return torch.where(bad[..., None], torch.full_like(mu, float('nan')), mu)


def dist(base, mat, squared=False):
    """the affine-invariant distance ||log(A^-1/2 B A^-1/2)||_F (or its square); the gradient of the distance itself
    is taken as 0 at d = 0"""
    mu = geneigvals(base, mat)
    bad = ~(mu > 0).all(-1)
    lg = torch.log(torch.where(bad[..., None], torch.ones_like(mu), mu))
    d2 = (lg * lg).sum(-1)
    if not squared:
        pos = d2 > 0
        d2 = torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    return torch.where(bad, torch.full_like(d2, float('nan')), d2)
