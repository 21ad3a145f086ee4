"""
Functions of data on the simplex (probabilities) on MI355X -- drop-in for `nitorch_fastmath.simplex`
(`simplex.py`): `softmax`, `log_softmax`, `logsumexp`, `logit` and `softmax_lse`, each with the reference's
"implicit" class: a class whose logit is fixed at zero and that need not be stored.

`implicit` is a bool or a pair `(the input has a hidden zero-logit class, the output drops that class)`;
one bool means both.  K = `input.shape[dim]` classes are stored, K' = K + 1 take part in the arithmetic when
the input is implicit.  The implicit class sits at `implicit_index` of the K'-long axis (negative values
count from its end; out of range raises IndexError).

One voxel per lane (`nfm_simplex.hip`): every input element is read once and every output element written
once, the hidden class is never built in memory and a dropped class is simply not written.  K' <= 17 (K <= 16
with a hidden class, K <= 17 without) keeps the classes in registers, K <= 48 sweeps the class axis, larger K
takes torch ops on the device.  Any `dim`
of a contiguous tensor (or of a dim-permuted view of one, e.g. the channel-last view of a channel-first field)
runs in place; other non-contiguous inputs take one `contiguous()`.  float32 and float64 GPU tensors.

Autograd: softmax, log_softmax and logsumexp have backward kernels and save one tensor each (the output,
the input, the input); `logit` runs its kernel forward and takes its gradient from a torch composition on the
saved input; the K > 48 route is torch ops, differentiated by torch.
"""
__all__ = ['logsumexp', 'softmax', 'log_softmax', 'logit', 'softmax_lse']
import torch
from . import _lib
from ._dispatch import call, dtype_code, needs_grad, require_gpu
from .utils import ensure_list

MAX_K = _lib.SX_MAX_K      # stored classes K served by the kernels (include/nfm_hip.h: NFM_SIMPLEX_MAX_K)
REGISTER_MAX_KP = 17       # ... with the classes in registers: K' = K + (implicit input) up to this


def _pair(implicit):
    imp = ensure_list(implicit, 2)
    if isinstance(implicit, (list, tuple)) and len(implicit) != 2:
        raise ValueError(f'implicit must be a bool or a pair of bools, got {implicit!r}')
    return bool(imp[0]), bool(imp[1])


def _index(implicit_index, kp):
    i = int(implicit_index)
    if not -kp <= i < kp:
        raise IndexError(f'implicit_index {implicit_index} is out of range for {kp} classes')
    return i % kp


def _prepare(input, dim):
    """checks + the contiguous tensor the kernels address: returns (x, d, restore) where `restore` maps a result
    computed on x back to the input's dim order"""
    input = torch.as_tensor(input)
    require_gpu(input)
    dtype_code(input.dtype)
    if isinstance(dim, (list, tuple)):
        raise TypeError('simplex functions take a single dim')
    scalar = input.dim() == 0
    if scalar:
        input = input.reshape(1)
    nd = input.dim()
    d = int(dim)
    if not -nd <= d < nd:
        raise IndexError(f'Dimension out of range (expected to be in range of [{-nd}, {nd - 1}], but got {dim})')
    d %= nd
    if input.shape[d] == 0:
        raise IndexError(f'simplex: expected dim {d} to have non-zero size (shape {tuple(input.shape)})')
    restore = (lambda r: r.reshape(())) if scalar else (lambda r: r)
    if not input.is_contiguous():
        st = input.stride()
        perm = sorted(range(nd), key=lambda k: (-st[k], k))
        xp = input.permute(perm)
        if xp.is_contiguous():          # a dim permutation of a contiguous tensor: run in place
            inv = [0] * nd
            for j, k in enumerate(perm):
                inv[k] = j
            return xp, inv[d], lambda r: r.permute(inv)
        input = input.contiguous()
    return input, d, restore


def _view(x, d):
    outer = 1
    for s in x.shape[:d]:
        outer *= int(s)
    inner = 1
    for s in x.shape[d + 1:]:
        inner *= int(s)
    return outer, int(x.shape[d]), inner


def _flags(imp_in, imp_out):
    return (_lib.SX_IMPLICIT_IN if imp_in else 0) | (_lib.SX_IMPLICIT_OUT if imp_out else 0)


def _with_class(t, extra, d, idx):
    return torch.cat([t.narrow(d, 0, idx), extra, t.narrow(d, idx, t.shape[d] - idx)], d)


def _without_class(t, d, idx):
    return torch.cat([t.narrow(d, 0, idx), t.narrow(d, idx + 1, t.shape[d] - idx - 1)], d)


def _torch_forward(op, x, d, imp_in, imp_out, idx):
    """the same functions from torch ops on the device (K above the kernels' range; differentiable)"""
    if op == _lib.SX_LOGIT:
        return _torch_logit(x, d, imp_in, imp_out, idx)
    z = _with_class(x, torch.zeros_like(x.narrow(d, 0, 1)), d, idx) if imp_in else x
    m = z.detach().max(d, keepdim=True)[0]
    lse = m + (z - m).exp().sum(d, keepdim=True).log()
    if op == _lib.SX_LOGSUMEXP:
        return None, lse
    out = (z - m).exp() / (z - m).exp().sum(d, keepdim=True) if op == _lib.SX_SOFTMAX else z - lse
    if imp_out:
        out = _without_class(out, d, idx)
    return out, lse


def _torch_logit(x, d, imp_in, imp_out, idx):
    if imp_in:
        extra = (1 - x.sum(d, keepdim=True)).clamp_min(1e-8).log()
        out = x.log() - extra
        if not imp_out:
            out = _with_class(out, torch.zeros_like(extra), d, idx)
        return out, None
    lg = x.log()
    ref = lg.narrow(d, idx, 1)
    return (_without_class(lg, d, idx) if imp_out else lg) - ref, None


def _forward(op, x, d, imp_in, imp_out, idx, want_lse=False):
    """(out, lse) of a contiguous x along d; lse keeps dim d with size 1 (no autograd)"""
    outer, K, inner = _view(x, d)
    ko = K + imp_in - imp_out
    only_lse = op == _lib.SX_LOGSUMEXP
    if K > MAX_K:
        with torch.no_grad():
            out, lse = _torch_forward(op, x, d, imp_in, imp_out, idx)
        return out, (lse if only_lse or want_lse else None)
    shape = list(x.shape)
    out = lse = None
    if not only_lse:
        out = torch.empty(shape[:d] + [ko] + shape[d + 1:], dtype=x.dtype, device=x.device)
    if only_lse or want_lse:
        lse = torch.empty(shape[:d] + [1] + shape[d + 1:], dtype=x.dtype, device=x.device)
    if outer * inner == 0:
        return out, lse
    if ko == 0:                         # the only class was dropped: nothing to write but the lse
        if lse is None:
            return out, lse
        op, imp_out, only_lse = _lib.SX_LOGSUMEXP, False, True
    call(_lib.lib().nfm_simplex_forward, x.device,
         dtype_code(x.dtype), op, _flags(imp_in, imp_out), idx, outer, K, inner, x.data_ptr(),
         None if only_lse else out.data_ptr(), None if lse is None else lse.data_ptr())
    return out, lse


def _backward(op, saved, g, d, K, imp_in, imp_out, idx):
    """grad_input (contiguous, K classes along d) from the saved tensor and grad_output"""
    g = g.to(saved.dtype).contiguous()
    shape = list(saved.shape)
    grad = torch.empty(shape[:d] + [K] + shape[d + 1:], dtype=saved.dtype, device=saved.device)
    outer, _, inner = _view(grad, d)
    if outer * inner == 0:
        return grad
    if K + imp_in - imp_out == 0:       # the output had no classes
        return grad.zero_()
    call(_lib.lib().nfm_simplex_backward, saved.device,
         dtype_code(saved.dtype), op, _flags(imp_in, imp_out), idx, outer, K, inner, saved.data_ptr(),
         g.data_ptr(), grad.data_ptr())
    return grad


def _run(op, input, dim, implicit, implicit_index):
    """softmax / log_softmax / logit: checks, layout, autograd route"""
    imp_in, imp_out = _pair(implicit)
    x, d, restore = _prepare(input, dim)
    K = x.shape[d]
    idx = _index(implicit_index, K + imp_in)
    if needs_grad(x):
        if K > MAX_K:
            return restore(_torch_forward(op, x, d, imp_in, imp_out, idx)[0])
        from . import _autograd
        fn = {_lib.SX_SOFTMAX: _autograd.SoftmaxFn, _lib.SX_LOG_SOFTMAX: _autograd.LogSoftmaxFn,
              _lib.SX_LOGIT: _autograd.LogitFn}[op]
        return restore(fn.apply(x, d, imp_in, imp_out, idx))
    return restore(_forward(op, x, d, imp_in, imp_out, idx)[0])


def logsumexp(input, dim=-1, keepdim=False, implicit=False):
    """Numerically stabilised log-sum-exp (`simplex.py:51-94`).

    implicit : bool; a hidden class with logit zero takes part in the sum (a pair, as the other functions
        take, is a TypeError here: there is no output class to drop).
    Returns the input's shape without `dim` (with size 1 there if `keepdim`).  Differentiable (backward
    kernel: softmax recomputed from the saved input and scaled, one pass).
    """
    if not isinstance(implicit, (bool, int)):
        raise TypeError(f'logsumexp: implicit must be a bool, got {implicit!r}')
    imp_in = bool(implicit)
    x, d, restore = _prepare(input, dim)
    K = x.shape[d]
    if needs_grad(x):
        if K > MAX_K:
            lse = _torch_forward(_lib.SX_LOGSUMEXP, x, d, imp_in, False, K if imp_in else 0)[1]
        else:
            from . import _autograd
            lse = _autograd.LogsumexpFn.apply(x, d, imp_in)
    else:
        lse = _forward(_lib.SX_LOGSUMEXP, x, d, imp_in, False, K if imp_in else 0)[1]
    lse = restore(lse)
    if keepdim or lse.dim() == 0:
        return lse
    nd = torch.as_tensor(input).dim()
    return lse.squeeze(int(dim) % nd)


def softmax(input, dim=-1, implicit=False, implicit_index=0):
    """SoftMax (`simplex.py:163-217`).

    implicit : `(in, out)`; `in`: a hidden class with logit zero exists; `out`: the implicit class is dropped
        from the output.  `(True, False)` returns K + 1 classes, the added one at `implicit_index`;
        `(False, True)` returns K - 1, class `implicit_index` left out.
    Differentiable: the backward kernel computes `p * (g - sum(g * p))` from the saved output, and is the
    derivative of this forward for every `implicit_index` (the reference's is not).
    """
    return _run(_lib.SX_SOFTMAX, input, dim, implicit, implicit_index)


def log_softmax(input, dim=-1, implicit=False, implicit_index=0):
    """log(softmax) (`simplex.py:326-366`); arguments as for `softmax`.  Differentiable (backward kernel:
    `g - softmax(x) * sum(g)` from the saved input)."""
    return _run(_lib.SX_LOG_SOFTMAX, input, dim, implicit, implicit_index)


def logit(input, dim=-1, implicit=False, implicit_index=0):
    """Multiclass logit, the inverse of softmax (`simplex.py:268-323`): `log(p_k) - log(p_ref)`.

    implicit : `(in, out)`; `in`: a hidden class holds the probability `1 - sum` (clamped at 1e-8 like the
        reference) and is the reference class; otherwise class `implicit_index` is.  `out`: the reference
        class (whose logit is zero) is dropped from the output.
    With or without `requires_grad` the forward is the kernel (same bits); the gradient comes from a torch
    composition on the saved input (no backward kernel: three elementwise ops and a sum).
    """
    return _run(_lib.SX_LOGIT, input, dim, implicit, implicit_index)


def softmax_lse(input, dim=-1, weights=None, implicit=False):
    """SoftMax and the log-sum-exp summed over all voxels (`simplex.py:369-431`), from one pass over `input`.

    weights : optional voxel weights of the log-sum-exp, broadcastable to the input with size 1 along `dim`.
    implicit : as for `softmax`; the implicit class is always the LAST one here (there is no `implicit_index`).
    Returns `(softmax, lse)`, lse a float64 scalar.
    """
    from . import reduce
    imp_in, imp_out = _pair(implicit)
    x, d, restore = _prepare(input, dim)
    K = x.shape[d]
    idx = K + imp_in - 1
    if needs_grad(x):
        p = softmax(input, dim, (imp_in, imp_out), -1)
        lse = logsumexp(input, dim, keepdim=True, implicit=imp_in)
    else:
        p, lse = _forward(_lib.SX_SOFTMAX, x, d, imp_in, imp_out, idx, want_lse=True)
        p, lse = restore(p), restore(lse)
    if weights is not None:
        weights = torch.as_tensor(weights, device=lse.device)
        lse = lse * weights.to(lse.dtype)
    return p, reduce.sum(lse, dtype=torch.float64)
