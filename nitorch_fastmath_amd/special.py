"""
Special functions on MI355X -- drop-in for `nitorch_fastmath.special` (`special.py`): `besseli`, `besseli_ratio`
and `mvdigamma`, one kernel launch each (`nfm_special.hip`): one read and one write per element, both branches
of every formula in the same kernel, no mask, no host synchronisation, so a call can be captured in a HIP graph
(`utils.graphed`).

`besseli(nu, z)` at nu = 0 and nu = 1 is the reference's arithmetic (the A&S polynomials, 5e-7 from the
function); at any other nu >= 0 it is the function itself, where the reference is wrong.
float32 and float64 GPU tensors; a tensor whose memory is dense in some order of its dims runs in place and
the result has its strides, anything else takes one `contiguous()`.  Differentiable in the tensor argument
(backward kernels, `_autograd.py`).
"""
__all__ = ['mvdigamma', 'besseli', 'besseli_ratio']
import math
import torch
from . import _lib
from ._dispatch import call, dtype_code, needs_grad, require_gpu

MAX_N = _lib.SP_MAX_N      # besseli_ratio: rounds N served by the kernel (include/nfm_hip.h: NFM_SPECIAL_MAX_N)
_MODES = {None: 0, 0: 0, 1: 1, 2: 2, 'norm': 1, 'log': 2}


def _dense(t):
    """`t` itself when its memory is one dense block in some order of its dims, else a contiguous copy"""
    if t.is_contiguous():
        return t
    dims = sorted((d for d in range(t.dim()) if t.shape[d] != 1), key=lambda d: -t.stride(d))
    expect = 1
    for d in reversed(dims):
        if t.stride(d) != expect:
            return t.contiguous()
        expect *= t.shape[d]
    return t


def _like(t):
    """an uninitialised tensor with exactly `t`'s strides: element k of its memory pairs with element k of `t`'s"""
    return torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device)


def _prepare(name, x):
    if not isinstance(x, torch.Tensor):
        raise RuntimeError(f'nitorch_fastmath_amd.special.{name} takes a tensor on the GPU; got {type(x).__name__}. '
                           'There is no CPU fallback: move the data with .cuda().')
    require_gpu(x)
    dtype_code(x.dtype)
    return _dense(x)


def _nu(nu):
    nu = float(nu)
    if not (nu >= 0 and math.isfinite(nu)):
        raise ValueError(f'nu must be a finite number >= 0, got {nu}')
    return nu


def _besseli_forward(nu, z, code):
    out = _like(z)
    if z.numel():
        call(_lib.lib().nfm_special_besseli, z.device, dtype_code(z.dtype), code, nu, z.numel(), z.data_ptr(), out.data_ptr())
    return out


def _besseli_backward(nu, z, out, g, code):
    g = g.to(z.dtype)
    if g.stride() != z.stride():
        g = _like(z).copy_(g)
    grad = _like(z)
    if z.numel():
        call(_lib.lib().nfm_special_besseli_backward, z.device, dtype_code(z.dtype), code, nu, z.numel(), z.data_ptr(),
             out.data_ptr(), g.data_ptr(), grad.data_ptr())
    return grad


def _ratio_forward(nu, x, N, K):
    """besseli_ratio without autograd: the kernel up to N = MAX_N, the same recurrence in torch ops above"""
    if N > MAX_N:
        with torch.no_grad():
            r = _ratio_torch(nu, x, N, K)
        return r if r.stride() == x.stride() else _like(x).copy_(r)
    out = _like(x)
    if x.numel():
        call(_lib.lib().nfm_special_besseli_ratio, x.device, dtype_code(x.dtype), nu, N, K, x.numel(), x.data_ptr(), out.data_ptr())
    return out


def _ratio_backward(nu, x, out, g):
    g = g.to(x.dtype)
    if g.stride() != x.stride():
        g = _like(x).copy_(g)
    grad = _like(x)
    if x.numel():
        call(_lib.lib().nfm_special_besseli_ratio_backward, x.device, dtype_code(x.dtype), nu, x.numel(), x.data_ptr(),
             out.data_ptr(), g.data_ptr(), grad.data_ptr())
    return grad


def _ratio_torch(nu, X, N, K):
    """the same recurrence from torch ops on the device (N above the kernel's registers)"""
    nu1 = nu + K
    XX = X * X
    rk = [X / ((XX + (nu1 + k + 1.5) ** 2).sqrt() + (nu1 + k + 0.5)) for k in range(N + 1)]
    for m in range(N, 0, -1):
        for k in range(1, m + 1):
            rk[k - 1] = X / ((rk[k] / rk[k - 1] * XX + (nu1 + k) ** 2).sqrt() + (nu1 + k))
        rk.pop(-1)
    r = rk[0]
    iX = X.reciprocal()
    for k in range(K, 0, -1):
        r = (r + iX * (2 * (nu + k))).reciprocal()
    r = torch.where(X == 0, torch.zeros_like(r), r)
    return torch.where(X == float('inf'), torch.ones_like(r), r)


def _digamma_forward(x, order):
    out = _like(x)
    if x.numel():
        call(_lib.lib().nfm_special_mvdigamma, x.device, dtype_code(x.dtype), order, x.numel(), x.data_ptr(), out.data_ptr())
    return out


def _digamma_backward(x, g, order):
    g = g.to(x.dtype)
    if g.stride() != x.stride():
        g = _like(x).copy_(g)
    grad = _like(x)
    if x.numel():
        call(_lib.lib().nfm_special_mvdigamma_backward, x.device, dtype_code(x.dtype), order, x.numel(), x.data_ptr(),
             g.data_ptr(), grad.data_ptr())
    return grad


def mvdigamma(input, order=1):
    """Derivative of the log of the (multivariate) Gamma function (`special.py:8-26`):
    `sum_{p=1..order} digamma(input + (1 - p) / 2)` in one pass, any `order >= 1`.

    `digamma` follows `torch.digamma` at the special values (0 -> -inf, negative integers -> NaN, reflection
    below zero).  Differentiable (backward kernel: the sum of trigammas).
    """
    order = int(order)
    if order < 1:
        raise ValueError(f'order must be >= 1, got {order}')
    x = _prepare('mvdigamma', input)
    if needs_grad(x):
        from . import _autograd
        return _autograd.MvDigammaFn.apply(x, order)
    return _digamma_forward(x, order)


def besseli(nu, z, mode=None):
    """Modified Bessel function of the first kind (`special.py:33-73`).

    nu : number >= 0
    z : tensor, z >= 0
    mode : 0 or None: besseli(nu, z); 1 or 'norm': besseli(nu, z) / exp(z); 2 or 'log': log(besseli(nu, z)).
        Any other string is a ValueError (the reference silently takes it as None).

    nu = 0 and nu = 1: the reference's polynomials, to rounding.  Any other nu: the function itself (the
    reference is wrong there, Q28 / Q29), computed in double whatever the dtype.  z = 0 gives 1 / 1 / 0 at nu = 0
    and 0 / 0 / -inf above; z = +inf gives +inf / 0 / +inf; NaN gives NaN; z < 0 is outside the contract (NaN
    at any nu but 0 and 1).  Differentiable in z (backward kernel from z and the saved output).
    """
    try:
        code = _MODES[mode]
    except (KeyError, TypeError):
        raise ValueError(f"mode must be one of None, 0, 1, 'norm', 2, 'log'; got {mode!r}") from None
    nu = _nu(nu)
    z = _prepare('besseli', z)
    if needs_grad(z):
        from . import _autograd
        return _autograd.BesseliFn.apply(z, nu, code)
    return _besseli_forward(nu, z, code)


def besseli_ratio(nu, X, N=4, K=10):
    """besseli(nu + 1, X) / besseli(nu, X) by Amos (1974) (`special.py:349-409`): eq. 20a at order nu + K, N
    rounds of eq. 20b, K steps of the backward recurrence, the N + 1 running ratios in registers.

    N above 8 runs the same recurrence in torch ops on the device (forward only: the gradient is the same backward
    kernel on the saved output, whichever route computed it).  X = 0 gives 0 and X = +inf gives 1, the
    limits (the reference returns NaN at both).  Differentiable in X (backward kernel: the
    Riccati identity r' = 1 - r^2 - (2 nu + 1) r / X on the saved output).
    """
    nu, N, K = _nu(nu), int(N), int(K)
    if N < 0 or K < 0:
        raise ValueError(f'N and K must be >= 0, got N={N}, K={K}')
    X = _prepare('besseli_ratio', X)
    if needs_grad(X):
        from . import _autograd
        return _autograd.BesseliRatioFn.apply(X, nu, N, K)
    return _ratio_forward(nu, X, N, K)
