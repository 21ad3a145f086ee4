"""Spectral functions of compact symmetric matrices in plain torch: the route of `sym.sym_funm` for the orders
that have no kernel (`nfm_sym_funm_max_order`), at any order.  Private and device-agnostic: it runs on CPU tensors
too when called directly (the host tests do).

Forward: compact -> full -> `torch.linalg.eigh` -> f on the (clamped) eigenvalues -> V f(L) V^T -> compact.
Backward: Daleckii-Krein, S = V [(V^T G V) o F] V^T with F_kl = f[l_k, l_l] from the same closed-form divided
differences as the kernels (csrc/nfm_symfun_ops.hpp), NOT torch's own `eigh` backward: that one divides by
l_k - l_l, which is what this function exists to avoid (repeated and clustered eigenvalues are the common case in
fields of isotropic tensors).  Same domain and NaN rules as the kernels: a record with a clamped eigenvalue outside
the domain of f, or with an entry that is not finite, is NaN in every component of the result and of the gradient.
"""
import torch
from torch.autograd.function import once_differentiable

EXP, LOG, SQRT, RSQRT, POW, CLAMP = range(6)      # include/nfm_hip.h: NFM_FUN_*


def order_of(K):
    M = int(((1 + 8 * K) ** 0.5 - 1) // 2)
    if M * (M + 1) // 2 != K:
        raise ValueError(f'last dimension {K} is not M*(M+1)/2 for any integer M')
    return M


def _index(M, device):
    """rows and columns of the compact components: the diagonal, then the rows of the upper triangle"""
    r = list(range(M)) + [i for i in range(M) for j in range(i + 1, M)]
    c = list(range(M)) + [j for i in range(M) for j in range(i + 1, M)]
    return torch.as_tensor(r, device=device), torch.as_tensor(c, device=device)


def to_full(mat, M, off=1.0):
    """compact -> full symmetric; `off` scales the off-diagonal components (1/2 for a cotangent)"""
    r, c = _index(M, mat.device)
    full = mat.new_zeros(mat.shape[:-1] + (M, M))
    v = mat.clone()
    v[..., M:] *= off
    full[..., r, c] = v
    full[..., c, r] = v
    return full


def pack(full, M, off=1.0):
    r, c = _index(M, full.device)
    out = full[..., r, c].clone()
    out[..., M:] *= off
    return out


def _clamp(x, vmin):
    return x if vmin is None else torch.clamp(x, min=vmin)


def _in_domain(fn, p, x):
    ok = torch.isfinite(x)
    if fn in (LOG, RSQRT) or (fn == POW and p < 0):
        return ok & (x > 0)
    if fn in (SQRT, POW):
        return ok & (x >= 0)
    return ok


def _fval(fn, p, x):
    if fn == EXP:
        return torch.exp(x)
    if fn == LOG:
        return torch.log(x)
    if fn == SQRT:
        return torch.sqrt(x)
    if fn == RSQRT:
        return 1 / torch.sqrt(x)
    if fn == POW:
        return torch.pow(x, p)
    return x


def _fprime(fn, p, a):
    if fn == EXP:
        return torch.exp(a)
    if fn == LOG:
        return 1 / a
    if fn == SQRT:
        return 0.5 / torch.sqrt(a)
    if fn == RSQRT:
        return -0.5 / (a * torch.sqrt(a))
    if fn == POW:
        return torch.zeros_like(a) if p == 0 else p * torch.pow(a, p - 1)
    return torch.ones_like(a)


def _divdiff0(fn, p, a, b):
    """f[a, b] in the closed forms of csrc/nfm_symfun_ops.hpp (a == b: f'(a))"""
    eq = a == b
    one = torch.ones_like(a)
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    if fn == EXP:
        h = 0.5 * a - 0.5 * b
        h2 = h * h
        hs = torch.where(eq, one, h)
        series = 1 + h2 * (1 / 6 + h2 * (1 / 120 + h2 * (1 / 5040)))
        d = torch.exp(0.5 * a + 0.5 * b) * torch.where(h2 < 2.0 ** -12, series, torch.sinh(hs) / hs)
    elif fn == LOG:
        t = torch.where(eq, one, (hi - lo) / lo)
        d = torch.log1p(t) / (t * lo)
    elif fn == SQRT:
        d = 1 / (torch.sqrt(a) + torch.sqrt(b))
    elif fn == RSQRT:
        sa, sb = torch.sqrt(a), torch.sqrt(b)
        d = -1 / (sa * sb * (sa + sb))
    elif fn == POW:
        if p == 0:
            return torch.zeros_like(a)
        t = torch.where(eq, one, (hi - lo) / lo)
        u = p * torch.log1p(t)
        d = torch.where(u.abs() <= 1, torch.pow(lo, p - 1) * (torch.expm1(u) / t),
                        (torch.pow(hi, p) - torch.pow(lo, p)) / torch.where(eq, one, hi - lo))
    else:
        return one
    return torch.where(eq, _fprime(fn, p, a), d)


def divdiff(fn, p, vmin, lam):
    """(..., M) eigenvalues -> (..., M, M) first divided differences of f o max(., vmin)"""
    a, b = torch.broadcast_tensors(lam[..., :, None], lam[..., None, :])
    ca, cb = _clamp(a, vmin), _clamp(b, vmin)
    d = _divdiff0(fn, p, ca, cb)
    if vmin is None:
        return d
    eq = a == b
    one = torch.ones_like(a)
    fac = torch.where(eq, (a >= vmin).to(a.dtype),
                      torch.where((ca != a) | (cb != b), (ca - cb) / torch.where(eq, one, a - b), one))
    return torch.where(fac == 0, torch.zeros_like(d), fac * d)


def _decompose(mat, fn, p, vmin):
    M = order_of(mat.shape[-1])
    bad = ~torch.isfinite(mat).all(-1)
    full = to_full(mat, M)
    eye = torch.eye(M, dtype=mat.dtype, device=mat.device)
    full = torch.where(bad[..., None, None], eye, full)
    lam, V = torch.linalg.eigh(full)
    ok = _in_domain(fn, p, _clamp(lam, vmin))
    bad = bad | ~ok.all(-1)
    lam = torch.where(bad[..., None], torch.ones_like(lam), lam)     # keep the arithmetic of a bad record quiet
    return M, lam, V, bad


def forward(mat, fn, p=None, vmin=None):
    """compact f(A) of compact A, (..., K) -> (..., K)"""
    M, lam, V, bad = _decompose(mat, fn, p, vmin)
    f = _fval(fn, p, _clamp(lam, vmin))
    out = pack((V * f[..., None, :]) @ V.transpose(-1, -2), M)
    return torch.where(bad[..., None], torch.full_like(out, float('nan')), out)


def backward(mat, gout, fn, p=None, vmin=None):
    """gradient with respect to the compact record, given the cotangent of the compact result (the module's
    compact convention: G_ii = g_ii, G_ij = g_ij / 2; the result is S_ii and 2 S_ij)"""
    M, lam, V, bad = _decompose(mat, fn, p, vmin)
    G = to_full(gout.expand(mat.shape), M, off=0.5)
    Vt = V.transpose(-1, -2)
    S = V @ ((Vt @ G @ V) * divdiff(fn, p, vmin, lam)) @ Vt
    out = pack(S, M, off=2.0)
    return torch.where(bad[..., None], torch.full_like(out, float('nan')), out)


class SymFunmFn(torch.autograd.Function):
    """differentiable once, with respect to `mat` only; nothing but `mat` is saved"""

    @staticmethod
    def forward(ctx, mat, fn, p, vmin):
        ctx.save_for_backward(mat)
        ctx.cfg = (fn, p, vmin)
        return forward(mat, fn, p, vmin)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (mat,) = ctx.saved_tensors
        return backward(mat, g, *ctx.cfg), None, None, None


def sym_funm(mat, fn, p=None, vmin=None):
    return SymFunmFn.apply(mat, fn, p, vmin)
