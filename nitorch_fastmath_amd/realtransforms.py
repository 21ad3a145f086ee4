"""
Discrete cosine and sine transforms on MI355X -- drop-in for `nitorch_fastmath.realtransforms`
(`realtransforms.py`): `dct`, `dst`, `idct`, `idst` along one axis and `dctn`, `dstn`, `idctn`, `idstn` along
several, types 1, 2 and 3, norms 'backward', 'forward', 'ortho' and the reference's 'ortho_scipy'.

A transform along an axis of length N is a fixed N x N matrix applied to every line.  Up to `max_len(dtype)` one
lane owns one line (`nfm_rt.hip`): the line is read once, every output is a direct sum against a table of
cosines / sines that the workgroup builds for itself, and the normalisation (global factor, end-term
corrections) happens in the same launch.  From there up to `mm_max_len(dtype)` (256 at most: the axes of whole
volumes) a workgroup owns 32 lines and forms the same sums as a matrix product on the matrix cores
(`nfm_rt_mm.hip`): the same table, the same fma chain per output, one read and one write per element, no
workspace.  Any `dim` of a contiguous tensor (or of a dim-permuted view of one) runs in place of a copy; other
non-contiguous inputs take one `contiguous()`.  The n-d forms are one launch per axis, the first from the input
into the result, the rest in place on the result, whichever kernel an axis takes.  Axes longer than
`mm_max_len(dtype)`, CPU tensors and other dtypes take a composition of `torch.fft` calls on the tensor's device
(`_torch_axis`), which applies the same matrices.

The inverses are the forward transform with norm (forward <-> backward) and type (2 <-> 3) flipped.  Half
precision promotes to float32, integers to float64, as upstream.  DCT-I of a single point has no definition
(the reference divides by zero there): ValueError.

Autograd: one Function; its backward is the transposed matrix, one launch per axis through the same Function
(the operator is linear, so it differentiates any number of times).
"""
__all__ = ['dct', 'dst', 'idct', 'idst', 'dctn', 'dstn', 'idctn', 'idstn']
import math
import torch
from . import _lib
from ._dispatch import call, needs_grad

_KERNEL_DTYPES = {torch.float32: _lib.F32, torch.float64: _lib.F64}
_FLIPNORM = {'backward': 'forward', 'forward': 'backward', 'ortho': 'ortho', 'ortho_scipy': 'ortho_scipy'}
_FLIPTYPE = {1: 1, 2: 3, 3: 2}
_max_len = {}
_mm_max_len = {}


def max_len(dtype):
    """longest axis the lane kernels serve for `dtype` (0 for a dtype they do not serve)"""
    code = _KERNEL_DTYPES.get(dtype)
    if code is None:
        return 0
    if code not in _max_len:
        _max_len[code] = int(_lib.lib().nfm_rt_max_len(code))
    return _max_len[code]


def mm_max_len(dtype):
    """longest axis routed to the matrix-core kernel for `dtype` (0 for a dtype it does not serve)"""
    code = _KERNEL_DTYPES.get(dtype)
    if code is None:
        return 0
    if code not in _mm_max_len:
        _mm_max_len[code] = int(_lib.lib().nfm_rt_mm_max_len(code))
    return _mm_max_len[code]


def _plan(kind, type, norm, N, transpose):
    """(type of the pure 2 cos / 2 sin matrix B, pre_first, pre_last, post_first, post_mid, post_last) with
    y = diag(post) B diag(pre) x -- the decomposition `make_plan` of nfm_rt_ops.hpp uses"""
    L = (N + 1 if kind else N - 1) if type == 1 else N
    pre = [1.0, 1.0]
    post = [1.0, 1.0]
    if type == 3:
        pre[1 if kind else 0] = 0.5
    if type == 1 and not kind:
        pre = [0.5, 0.5]
    f = 1.0
    if norm == 'forward':
        f = 1 / (2 * L)
    elif norm in ('ortho', 'ortho_scipy'):
        f = 1 / math.sqrt(2 * L)
        end = 0 if (not kind or (norm == 'ortho_scipy' and type != 1)) else 1
        if type == 2:
            post[end] *= math.sqrt(0.5)
        if type == 3:
            pre[end] *= math.sqrt(2)
        if type == 1 and not kind:
            pre = [p * math.sqrt(2) for p in pre]
            post = [p * math.sqrt(0.5) for p in post]
    bt = type
    if transpose:
        bt = _FLIPTYPE[type]
        pre, post = post, pre
    if N == 1:
        pre = [pre[0] * pre[1], 1.0]
        post = [post[0] * post[1], 1.0]
    return bt, pre[0], pre[1], f * post[0], f, f * post[1]


def _ends(N, first, mid, last, dtype, device):
    v = torch.full((N,), mid, dtype=dtype, device=device)
    v[0] = first
    if N > 1:
        v[-1] = last
    return v


def _torch_axis(x, d, kind, type, norm, transpose):
    """The transform of axis `d` from torch.fft calls on x's device (float32 / float64 x): the matrix
    B[k][n] = 2 cos / 2 sin(pi (a k + b)(c n + e) / D) is the real or imaginary part of a zero-padded DFT of
    twice the length, with a half-sample phase on the input (type III) or on the output (type II)."""
    N = x.shape[d]
    bt, pre0, pre1, post0, postm, post1 = _plan(kind, type, norm, N, transpose)
    x = x.movedim(d, -1)
    x = x * _ends(N, pre0, 1.0, pre1, x.dtype, x.device)
    cdtype = torch.complex64 if x.dtype == torch.float32 else torch.complex128
    if bt == 1:
        if kind:      # 2 sin(pi (k+1)(n+1) / (N+1))
            z = torch.nn.functional.pad(x, (1, 0))
            y = -2 * torch.fft.rfft(z, n=2 * (N + 1), dim=-1)[..., 1:N + 1].imag
        else:         # 2 cos(pi k n / (N-1))
            y = 2 * torch.fft.rfft(x, n=2 * (N - 1), dim=-1)[..., :N].real
    elif bt == 2:
        X = torch.fft.rfft(x, n=2 * N, dim=-1)
        k = torch.arange(N, device=x.device, dtype=torch.float64) + (1 if kind else 0)
        w = torch.polar(torch.ones_like(k), -math.pi * k / (2 * N)).to(cdtype)
        if kind:      # 2 sin(pi (k+1)(2n+1) / 2N)
            y = -2 * (X[..., 1:N + 1] * w).imag
        else:         # 2 cos(pi k (2n+1) / 2N)
            y = 2 * (X[..., :N] * w).real
    else:
        n = torch.arange(N, device=x.device, dtype=torch.float64) + (1 if kind else 0)
        w = torch.polar(torch.ones_like(n), -math.pi * n / (2 * N)).to(cdtype)
        z = x * w
        if kind:      # 2 sin(pi (2k+1)(n+1) / 2N)
            z = torch.nn.functional.pad(z, (1, 0))
            y = -2 * torch.fft.fft(z, n=2 * N, dim=-1)[..., :N].imag
        else:         # 2 cos(pi (2k+1) n / 2N)
            y = 2 * torch.fft.fft(z, n=2 * N, dim=-1)[..., :N].real
    y = y * _ends(N, post0, postm, post1, x.dtype, x.device)
    return y.movedim(-1, d)


def _view(x, d):
    outer = 1
    for s in x.shape[:d]:
        outer *= int(s)
    inner = 1
    for s in x.shape[d + 1:]:
        inner *= int(s)
    return outer, int(x.shape[d]), inner


def _layout(x):
    """(xp, inv): xp a contiguous tensor holding x's elements -- x itself, a dim permutation of x that is
    contiguous (no copy), or a copy -- and `inv` with xp.permute(inv) shaped like x (None: xp is shaped like x)"""
    if x.is_contiguous():
        return x, None
    st = x.stride()
    nd = x.dim()
    perm = sorted(range(nd), key=lambda k: (-st[k], k))
    xp = x.permute(perm)
    if xp.is_contiguous():
        inv = [0] * nd
        for j, k in enumerate(perm):
            inv[k] = j
        return xp, inv
    return x.contiguous(), None


def _route(x, N, force_torch):
    """who transforms an axis of length N of x: 'lane' (nfm_rt_transform), 'mm' (nfm_rt_transform_mm) or 'torch'"""
    if force_torch or not x.is_cuda or N <= 0:
        return 'torch'
    if N <= max_len(x.dtype):
        return 'lane'
    return 'mm' if N <= mm_max_len(x.dtype) else 'torch'


def _apply(x, dims, kind, type, norm, transpose, force_torch=False):
    """the transform of every axis in `dims` of a float32 / float64 tensor, without autograd"""
    for d in dims:
        if kind == _lib.RT_DCT and type == 1 and x.shape[d] == 1:
            raise ValueError('DCT-I needs at least two points along the axis')
    if x.numel() == 0 or not dims:
        return x.clone()
    xp, inv = _layout(x)
    if inv is not None:
        dims = [inv[d] for d in dims]               # xp.permute(inv) == x: axis k of x is axis inv[k] of xp
    cur, out = xp, None
    for d in dims:
        N = cur.shape[d]
        route = _route(cur, N, force_torch)
        if route != 'torch':
            if out is None:
                out = torch.empty_like(cur, memory_format=torch.contiguous_format)
            outer, _, inner = _view(cur, d)
            fn = _lib.lib().nfm_rt_transform if route == 'lane' else _lib.lib().nfm_rt_transform_mm
            call(fn, cur.device, _KERNEL_DTYPES[cur.dtype], kind, type,
                 _lib.RT_NORMS[norm], int(transpose), N, outer, inner, cur.data_ptr(), out.data_ptr())
            cur = out
        else:
            cur = out = _torch_axis(cur, d, kind, type, norm, transpose).contiguous()
    return cur if inv is None else cur.permute(inv)


def _promote(x):
    x = torch.as_tensor(x)
    if not x.dtype.is_floating_point:
        return x.to(torch.float64)
    if x.dtype in (torch.float16, torch.bfloat16):
        return x.to(torch.float32)
    return x


def _dims(x, dim, nd_form):
    nd = x.dim()
    if dim is None:
        dim = list(range(nd)) if nd_form else -1
    dims = list(dim) if isinstance(dim, (list, tuple)) else [dim]
    out = []
    for d in dims:
        d = int(d)
        if not -nd <= d < nd:
            raise IndexError(f'Dimension out of range (expected to be in range of [{-nd}, {nd - 1}], but got {d})')
        out.append(d % nd)
    if len(set(out)) != len(out):
        raise ValueError('all dims must be unique')
    return out


def _run(kind, x, dim, norm, type, nd_form, inverse=False):
    norm = norm or 'backward'
    if type not in (1, 2, 3):
        raise ValueError(f'{"DST" if kind else "DCT"} only implemented for types 1, 2 and 3, got {type!r}')
    if norm not in _FLIPNORM:
        raise ValueError(f'invalid norm {norm!r}: expected "backward", "forward", "ortho" or "ortho_scipy"')
    if inverse:
        norm, type = _FLIPNORM[norm], _FLIPTYPE[type]
    if type == 1 and norm == 'ortho_scipy':
        norm = 'ortho'
    x = _promote(x)
    if x.dtype.is_complex:
        raise TypeError('real transforms take real tensors')
    dims = _dims(x, dim, nd_form)
    if needs_grad(x):
        from . import _autograd
        return _autograd.RealTransformFn.apply(x, kind, type, norm, tuple(dims), False)
    return _apply(x, dims, kind, type, norm, False)


def dct(x, dim=-1, norm='backward', type=2):
    """Discrete cosine transform along `dim` (`_impl/realtransforms.py:11-45`).

    norm : 'backward' (no scaling), 'forward' (1 / 2N; 1 / 2(N-1) for type 1), 'ortho' (orthogonal matrix),
        'ortho_scipy' (the same for a DCT); None means 'backward'.
    type : 1, 2 or 3 (ValueError otherwise).
    """
    return _run(_lib.RT_DCT, x, dim, norm, type, False)


def idct(x, dim=-1, norm='backward', type=2):
    """Inverse of `dct(x, dim, norm, type)` (`_impl/realtransforms.py:48-81`): the transform of the flipped type
    (2 <-> 3) under the flipped norm (forward <-> backward)."""
    return _run(_lib.RT_DCT, x, dim, norm, type, False, inverse=True)


def dst(x, dim=-1, norm='backward', type=2):
    """Discrete sine transform along `dim` (`_impl/realtransforms.py:84-124`).

    norm : as for `dct` (type 1 scales by N + 1).  'ortho' is orthogonal and equals scipy's; 'ortho_scipy' is
        the reference's own convention for types 2 and 3: the sqrt(2) correction sits on the first term
        instead of the last.
    """
    return _run(_lib.RT_DST, x, dim, norm, type, False)


def idst(x, dim=-1, norm='backward', type=2):
    """Inverse of `dst(x, dim, norm, type)` for 'backward', 'forward' and 'ortho'
    (`_impl/realtransforms.py:127-166`): flipped type under the flipped norm."""
    return _run(_lib.RT_DST, x, dim, norm, type, False, inverse=True)


def dctn(x, dim=None, norm='backward', type=2):
    """`dct` along every axis of `dim` (all axes when None), `_impl/realtransforms.py:169-204`."""
    return _run(_lib.RT_DCT, x, dim, norm, type, True)


def idctn(x, dim=None, norm='backward', type=2):
    """`idct` along every axis of `dim` (all axes when None), `_impl/realtransforms.py:207-241`."""
    return _run(_lib.RT_DCT, x, dim, norm, type, True, inverse=True)


def dstn(x, dim=None, norm='backward', type=2):
    """`dst` along every axis of `dim` (all axes when None), `_impl/realtransforms.py:244-285`."""
    return _run(_lib.RT_DST, x, dim, norm, type, True)


def idstn(x, dim=None, norm='backward', type=2):
    """`idst` along every axis of `dim` (all axes when None), `_impl/realtransforms.py:288-328`."""
    return _run(_lib.RT_DST, x, dim, norm, type, True, inverse=True)
