"""
Compact-storage symmetric matrices on MI355X -- drop-in for `nitorch_fastmath.sym`.

Same layout as the reference (`nitorch_fastmath/sym.py:7-14`): the flattened matrix
holds the diagonal first, then the rows of the upper triangle::

    [ a d e ]
    [ . b f ]   =>  [a b c d e f]
    [ . . c ]

Matrix-vector functions (`sym_matvec`, `sym_solve`, and the add/sub forms) also accept
and auto-detect compact diagonal / scaled-identity / full matrices, as the reference
documents (`sym.py:16-24`): for a vector `(*, N)` and a matrix `(*, NN)`, `NN` may be
`1` (scaled identity), `N` (diagonal), `N*(N+1)//2` (symmetric) or `N*N` (full).

Every function launches hand-written gfx950 kernels through the C ABI of
`libnfm_hip.so` on the current stream; tensors must live on the GPU.
"""
__all__ = [
    'sym_to_full', 'sym_diag', 'sym_outer', 'sym_det', 'sym_matmul',
    'sym_matvec',
    'sym_addmatvec', 'sym_addmatvec_',
    'sym_submatvec', 'sym_submatvec_',
    'sym_solve', 'sym_solve_',
    'sym_invert', 'sym_invert_',
    'sym_matmul_solve',      # extension: fused Gauss-Newton step (not in the reference)
    # extensions: spectral functions of compact symmetric matrices (not in the reference)
    'sym_funm', 'sym_expm', 'sym_logm', 'sym_sqrtm', 'sym_rsqrtm', 'sym_powm', 'sym_clampm',
    # extensions: sorted eigendecomposition of compact symmetric matrices (not in the reference)
    'sym_eigvals', 'sym_eigh',
    # extensions: spectral functions of two compact symmetric matrices (not in the reference)
    'sym_pencil_funm', 'sym_geodesic', 'sym_geomean', 'sym_logmap', 'sym_expmap', 'sym_geneigvals', 'sym_dist',
    'sym_karcher_mean',
    # extensions: Cholesky kernels of compact symmetric positive definite matrices (not in the reference)
    'sym_chol', 'sym_chol_apply', 'sym_logdet', 'sym_mahalanobis', 'sym_gauss_logpdf',
]
import ctypes
from math import sqrt
import torch
from . import _lib
from ._dispatch import Batch, broadcast_shapes, expand_batch, launch, max_order, needs_grad, prepare


def _nb_prm(K):
    M = int((sqrt(1 + 8 * K) - 1) // 2)
    if M * (M + 1) // 2 != K:
        raise ValueError(f'last dimension {K} is not M*(M+1)/2 for any integer M')
    return M


def _check_order(M):
    if not 1 <= M <= _lib.MAX_DIM:
        raise ValueError(f'matrix order {M} outside the supported range 1..{_lib.MAX_DIM}')


def _mat_kind(NN, N):
    """`sym.py:16-24`; ambiguous sizes (N = 1) resolve to the symmetric reading."""
    if NN == N * (N + 1) // 2:
        return _lib.MAT_SYM
    if NN == N:
        return _lib.MAT_DIAG
    if NN == 1:
        return _lib.MAT_SCAL
    if NN == N * N:
        return _lib.MAT_FULL
    raise ValueError(f'matrix with {NN} components does not match a vector of length {N}: '
                     f'expected 1, {N}, {N * (N + 1) // 2} or {N * N}')


# orders 9..16 of sym_solve / sym_invert: 'auto' = positive definite first, 'always' = pivoted at once
PIVOTING = 'auto'


def _pivoting(pivoting):
    mode = PIVOTING if pivoting is None else pivoting
    if mode not in ('auto', 'always'):
        raise ValueError(f"pivoting must be 'auto' or 'always', got {mode!r}")
    return mode == 'always'


def _eps_array(eps, N):
    """the `eps` argument of the C ABI: MAX_DIM doubles, the last given value repeated up to N (None: NULL)"""
    if eps is None:
        return None
    e = [float(x) for x in torch.as_tensor(eps, dtype=torch.float64).flatten().tolist()]
    if not e:
        raise ValueError('eps is empty')
    e = (e + [e[-1]] * N)[:N]
    return (ctypes.c_double * _lib.MAX_DIM)(*(e + [0.0] * (_lib.MAX_DIM - N)))


def _alloc_out(out, shape, dtype, device, like=None):
    if out is None:
        # a channel-first (component-major) operand of the output's shape hands its layout on:
        # the whole call then runs through the SoA tiles and downstream ops keep the field layout
        if (like is not None and tuple(like.shape) == tuple(shape) and like.dim() >= 2
                and like.stride(-1) != 1 and not like.is_contiguous()
                and like.numel() > 0 and 0 not in like.stride()):
            cand = torch.empty_like(like, dtype=dtype)      # preserve_format keeps dense strides
            if cand.stride() == like.stride():
                return cand, None
        return torch.empty(shape, dtype=dtype, device=device), None
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f'out has shape {tuple(out.shape)}, expected {tuple(shape)}')
    if out.dtype != dtype or out.device != device:
        raise ValueError('out must have the computation dtype and live on the same device')
    return out, None


def _full_view(mat, N, kind):
    """Full matrices come as (..., N*N) per `sym.py:24`; view them as (..., N, N)."""
    if kind == _lib.MAT_FULL:
        return mat.unflatten(-1, (N, N)), 2
    return mat, 1


def _matvec_impl(mode, inp, mat, vec, dtype, out):
    dev, dtype, (inp, mat, vec) = prepare(dtype, inp, mat, vec)
    N = vec.shape[-1]
    kind = _mat_kind(mat.shape[-1], N)
    if N > _lib.MAX_DIM:          # the reference's own large-order route, on the device (_bigorder.py)
        from . import _bigorder
        return _bigorder.sym_matvec(mode, inp, mat, vec, out, mat.shape[-1])
    matv, mat_nc = _full_view(mat, N, kind)
    shapes = [mat.shape[:-1], vec.shape[:-1]] + ([inp.shape[:-1]] if inp is not None else [])
    batch = broadcast_shapes(*shapes)
    if inp is not None and inp.shape[-1] != N:
        raise ValueError('inp and vec must have the same number of components')
    out, _ = _alloc_out(out, tuple(batch) + (N,), dtype, dev, like=vec if (N <= 8 or kind == _lib.MAT_SYM) else None)
    ops = [expand_batch(batch, matv, mat_nc), expand_batch(batch, vec, 1)]
    ncs = [mat_nc, 1]
    if inp is not None:
        ops.append(expand_batch(batch, inp, 1))
        ncs.append(1)
    ops.append(out)
    ncs.append(1)
    b = Batch(batch, ops, ncs, pack=N > 8 and kind == _lib.MAT_SYM)
    launch(_lib.lib().nfm_sym_matvec, dev, dtype, (N, kind, mode), b, (0, 1, None if inp is None else 2, -1))
    return out


def _cast(dtype, *tensors):
    """differentiable torch route of the orders > MAX_DIM: operands as tensors of the computation dtype"""
    ts = [None if t is None else torch.as_tensor(t) for t in tensors]
    if dtype is None:
        dtype = ts[0].dtype
        for t in ts[1:]:
            if t is not None:
                dtype = torch.promote_types(dtype, t.dtype)
    return [None if t is None else t.to(dtype) for t in ts]


def _matvec(mode, inp, mat, vec, dtype, out):
    from ._autograd import SymMatvecFn
    if needs_grad(inp, mat, vec):
        if out is not None:
            raise RuntimeError('out= is not supported for tensors that require grad')
        if torch.as_tensor(vec).shape[-1] > _lib.MAX_DIM:   # torch.linalg route: torch differentiates it (forward AND backward)
            from . import _bigorder
            mat_, vec_, inp_ = _cast(dtype, mat, vec, inp)
            return _bigorder.sym_matvec(mode, inp_, mat_, vec_, None, mat_.shape[-1])
        return SymMatvecFn.apply(mode, inp, torch.as_tensor(mat), torch.as_tensor(vec), dtype)
    return _matvec_impl(mode, inp, mat, vec, dtype, out)


def sym_matvec(mat, vec, dtype=None, out=None):
    r"""Matrix-vector product with a compact symmetric matrix: `mat @ vec`.

    Replaces `nitorch_fastmath.sym.sym_matvec` (in-repo: `_impl/sym.py:134-172`).

    Parameters
    ----------
    mat : `(..., NN) tensor`
        Compact matrix; `NN` in `{1, M, M*(M+1)//2, M*M}` (see module docstring).
    vec : `(..., M) tensor`
    dtype : `torch.dtype`, optional
        Computation (and output) dtype; default: promoted input dtype.
    out : `(..., M) tensor`, optional

    Returns
    -------
    matvec : `(..., M) tensor`
    """
    return _matvec(0, None, mat, vec, dtype, out)


def sym_addmatvec(inp, mat, vec, dtype=None, out=None):
    """`inp + mat @ vec` (reference name list `sym.py:31`)."""
    return _matvec(+1, inp, mat, vec, dtype, out)


def sym_addmatvec_(inp, mat, vec):
    """In-place `inp += mat @ vec`."""
    _require_inplace_ok(inp, broadcast_shapes(mat.shape[:-1], vec.shape[:-1]) + vec.shape[-1:])
    return _matvec_impl(+1, inp, mat, vec, inp.dtype, inp)


def sym_submatvec(inp, mat, vec, dtype=None, out=None):
    """`inp - mat @ vec` (reference name list `sym.py:32`)."""
    return _matvec(-1, inp, mat, vec, dtype, out)


def sym_submatvec_(inp, mat, vec):
    """In-place `inp -= mat @ vec`."""
    _require_inplace_ok(inp, broadcast_shapes(mat.shape[:-1], vec.shape[:-1]) + vec.shape[-1:])
    return _matvec_impl(-1, inp, mat, vec, inp.dtype, inp)


def _require_inplace_ok(t, shape):
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'in-place operand has shape {tuple(t.shape)} but the result has shape '
                         f'{tuple(shape)} (it cannot be broadcast)')


def sym_solve(mat, vec, eps=None, dtype=None, out=None, *, pivoting=None):
    r"""Left matrix division for compact symmetric matrices: `mat \ vec`.

    Replaces `nitorch_fastmath.sym.sym_solve` (in-repo: `_impl/sym.py:327-398`).
    Orders up to 4 use the reference's closed forms evaluated in its operation order
    (bit-identical to its CPU path); larger orders use LU with partial pivoting per
    lane, like the `torch.linalg.solve` branch of the reference.

    Parameters
    ----------
    mat : `(..., NN) tensor`
    vec : `(..., M) tensor`
    eps : `float or (M,) sequence[float]`, optional
        Smoothing term added to the diagonal of `mat` (last value repeated).
    dtype, out : optional
    pivoting : {'auto', 'always'}, keyword-only, default `sym.PIVOTING` = 'auto'
        Orders 9..16.  'auto': the unpivoted LDL^T first -- positive definite matrices, what Hessians are -- and the
        pivoted elimination for the groups of matrices that are not; 'always': the pivoted elimination at once (a
        batch of INDEFINITE matrices pays the attempt for nothing: up to 2x).  Same answers within rounding.

    Returns
    -------
    result : `(..., M) tensor`
    """
    from ._autograd import SymSolveFn
    piv = _pivoting(pivoting)
    if needs_grad(mat, vec):
        if out is not None:
            raise RuntimeError('out= is not supported for tensors that require grad')
        if torch.as_tensor(vec).shape[-1] > _lib.MAX_DIM:   # torch.linalg route: torch differentiates it
            from . import _bigorder
            mat_, vec_ = _cast(dtype, mat, vec)
            return _bigorder.sym_solve(mat_, vec_, eps, None, mat_.shape[-1])
        return SymSolveFn.apply(torch.as_tensor(mat), torch.as_tensor(vec), eps, dtype, 'always' if piv else 'auto')
    dev, dtype, (mat, vec) = prepare(dtype, mat, vec)
    N = vec.shape[-1]
    kind = _mat_kind(mat.shape[-1], N)
    if N > _lib.MAX_DIM:          # densify + torch.linalg.solve on the device, as `_impl/sym.py:392-396`
        from . import _bigorder
        return _bigorder.sym_solve(mat, vec, eps, out, mat.shape[-1])
    matv, mat_nc = _full_view(mat, N, kind)
    batch = broadcast_shapes(mat.shape[:-1], vec.shape[:-1])
    # (orders 9..16 of compact matrices take component-major fields as they are since round 3 -- `spd_strided_kernel`
    # -- so channel-first input gets channel-first output at every order; Batch packs what is strided along the batch)
    piv = _pivoting(pivoting)
    out, _ = _alloc_out(out, tuple(batch) + (N,), dtype, dev,
                        like=vec if (N <= 8 or (kind == _lib.MAT_SYM and not piv)) else None)
    b = Batch(batch, [expand_batch(batch, matv, mat_nc), expand_batch(batch, vec, 1), out], [mat_nc, 1, 1],
              pack=('all' if piv else True) if (N > 8 and kind == _lib.MAT_SYM) else False)
    launch(_lib.lib().nfm_sym_solve, dev, dtype, (N, kind | (_lib.MAT_PIVOTED if piv else 0)), b,
           tail=(_eps_array(eps, N),))
    return out


def sym_solve_(mat, vec, eps=None):
    """In-place `sym_solve`: overwrites `vec` with `mat \\ vec` (`sym.py:33`)."""
    _require_inplace_ok(vec, broadcast_shapes(mat.shape[:-1], vec.shape[:-1]) + vec.shape[-1:])
    return sym_solve(mat, vec, eps=eps, dtype=vec.dtype, out=vec)


def sym_invert(mat, diag=False, dtype=None, out=None, *, pivoting=None):
    r"""Inverse of compact symmetric matrices, returned in compact storage.

    Replaces `nitorch_fastmath.sym.sym_invert` (in-repo: `_impl/sym.py:455-493`,
    which runs M full solves; here one factorisation per matrix).

    Parameters
    ----------
    mat : `(..., M*(M+1)//2) tensor`
    diag : `bool`, default=False
        If True, only return the diagonal of the inverse, shape `(..., M)`.
    pivoting : {'auto', 'always'}, keyword-only: see `sym_solve`.
    """
    from ._autograd import SymInvertFn
    piv = _pivoting(pivoting)
    if needs_grad(mat):
        if out is not None:
            raise RuntimeError('out= is not supported for tensors that require grad')
        if _nb_prm(torch.as_tensor(mat).shape[-1]) > _lib.MAX_DIM:
            from . import _bigorder
            (mat_,) = _cast(dtype, mat)
            return _bigorder.sym_invert(mat_, _nb_prm(mat_.shape[-1]), bool(diag), None)
        return SymInvertFn.apply(torch.as_tensor(mat), bool(diag), dtype, 'always' if piv else 'auto')
    dev, dtype, (mat,) = prepare(dtype, mat)
    M = _nb_prm(mat.shape[-1])
    if M > _lib.MAX_DIM:
        from . import _bigorder
        return _bigorder.sym_invert(mat, M, bool(diag), out)
    batch = mat.shape[:-1]
    uncovered = piv          # (the pivoted kernels of orders 9..16 want contiguous records: everything is packed for them)
    out, _ = _alloc_out(out, tuple(batch) + ((M,) if diag else (mat.shape[-1],)), dtype, dev, like=None if uncovered else mat)
    b = Batch(batch, [mat, out], [1, 1], pack=('all' if uncovered else True) if (M > 8 and not diag) else False)
    launch(_lib.lib().nfm_sym_invert, dev, dtype, (M, int(bool(diag)) | (_lib.INVERT_PIVOTED if piv else 0)), b)
    return out


def sym_invert_(mat):
    """In-place `sym_invert`: overwrites `mat` with its compact inverse (`sym.py:34`)."""
    return sym_invert(mat, dtype=mat.dtype, out=mat)


def sym_det(mat, dtype=None, out=None):
    r"""Determinant of compact symmetric matrices (`_impl/sym.py:401-452`).

    The reference derives M from a batch dimension by mistake (quirk Q2); this
    implementation uses the compact dimension, as documented.
    """
    from ._autograd import SymDetFn
    if needs_grad(mat):
        if out is not None:
            raise RuntimeError('out= is not supported for tensors that require grad')
        if _nb_prm(torch.as_tensor(mat).shape[-1]) > _lib.MAX_DIM:
            from . import _bigorder
            (mat_,) = _cast(dtype, mat)
            return _bigorder.sym_det(mat_, _nb_prm(mat_.shape[-1]), None)
        return SymDetFn.apply(torch.as_tensor(mat), dtype)
    dev, dtype, (mat,) = prepare(dtype, mat)
    M = _nb_prm(mat.shape[-1])
    if M > _lib.MAX_DIM:
        from . import _bigorder
        return _bigorder.sym_det(mat, M, out)
    batch = mat.shape[:-1]
    out, _ = _alloc_out(out, tuple(batch), dtype, dev)
    b = Batch(batch, [mat, out], [1, 0], pack=M > 8)
    launch(_lib.lib().nfm_sym_det, dev, dtype, (M,), b)
    return out


def _grad_guard(out):
    if out is not None:
        raise RuntimeError('out= is not supported for tensors that require grad')


def sym_to_full(mat, dtype=None, out=None):
    r"""Compact symmetric `(..., M*(M+1)//2)` -> full `(..., M, M)` (`_impl/sym.py:16-60`)."""
    from ._autograd import SymToFullFn
    if needs_grad(mat):
        _grad_guard(out)
        return SymToFullFn.apply(torch.as_tensor(mat), dtype)
    dev, dtype, (mat,) = prepare(dtype, mat)
    M = _nb_prm(mat.shape[-1])
    if M > _lib.MAX_DIM:
        from . import _bigorder
        return _bigorder._deliver(_bigorder.to_full(mat, M), out)
    batch = mat.shape[:-1]
    out, _ = _alloc_out(out, tuple(batch) + (M, M), dtype, dev)
    b = Batch(batch, [mat, out], [1, 2])
    launch(_lib.lib().nfm_sym_to_full, dev, dtype, (M,), b)
    return out


def sym_diag(mat):
    r"""View into the main diagonal of a compact symmetric matrix, shape `(..., M)`
    (`_impl/sym.py:63-84`; a pure view, no kernel)."""
    mat = torch.as_tensor(mat)
    return mat[..., :_nb_prm(mat.shape[-1])]


def sym_outer(x, dtype=None, out=None):
    r"""Symmetric outer product `x x^T` in compact storage (`_impl/sym.py:496-528`)."""
    from ._autograd import SymOuterFn
    if needs_grad(x):
        _grad_guard(out)
        return SymOuterFn.apply(torch.as_tensor(x), dtype)
    dev, dtype, (x,) = prepare(dtype, x)
    M = x.shape[-1]
    _check_order(M)
    batch = x.shape[:-1]
    out, _ = _alloc_out(out, tuple(batch) + (M * (M + 1) // 2,), dtype, dev)
    b = Batch(batch, [x, out], [1, 1])
    launch(_lib.lib().nfm_sym_outer, dev, dtype, (M,), b)
    return out


def sym_matmul(j, h, dtype=None, out=None):
    r"""Symmetric product `J^T H J` with compact `H`, returned compact (`_impl/sym.py:637-670`).

    j : `(..., k, d)`, h : `(..., k*(k+1)//2)` (or `(..., k)` diagonal) -> `(..., d*(d+1)//2)`.
    For `k == d` in `{2, 3}` the reference's specialised kernels evaluate `J H J^T`
    (quirk Q16); this function returns what the reference returns.
    """
    from ._autograd import SymMatmulFn
    if needs_grad(j, h):
        _grad_guard(out)
        return SymMatmulFn.apply(torch.as_tensor(j), torch.as_tensor(h), dtype)
    dev, dtype, (j, h) = prepare(dtype, j, h)
    k, d = j.shape[-2:]
    _check_order(k)
    _check_order(d)
    if h.shape[-1] == k * (k + 1) // 2:
        hk = _lib.MAT_SYM
    elif h.shape[-1] == k:
        hk = _lib.MAT_DIAG
    else:
        raise ValueError(f'hessian with {h.shape[-1]} components does not match k={k}')
    batch = broadcast_shapes(j.shape[:-2], h.shape[:-1])
    out, _ = _alloc_out(out, tuple(batch) + (d * (d + 1) // 2,), dtype, dev)
    b = Batch(batch, [expand_batch(batch, j, 2), expand_batch(batch, h, 1), out], [2, 1, 1])
    launch(_lib.lib().nfm_sym_matmul, dev, dtype, (k, d, hk), b)
    return out


def sym_matmul_solve(j, h, g, eps=None, dtype=None, out=None):
    r"""EXTENSION (not in the reference): `sym_solve(sym_matmul(j, h), g, eps)` in ONE kernel.

    The Gauss-Newton step of a Hessian field pushed through a Jacobian field,
    `x = (J^T H J + diag(eps))^{-1} g`, without writing the compact `(d x d)` product to HBM and
    reading it back: for k = d = 3 fp32, 84 B per element instead of 132 B.
    Same arithmetic as the two calls, so the result is bit-identical to the chain (including the
    reference's `J H J^T` quirk for k = d in {2, 3}).  Sizes beyond 4 fall back to the chain.

    j : `(..., k, d)`, h : `(..., k*(k+1)//2)` or `(..., k)`, g : `(..., d)` -> `(..., d)`.
    """
    k, d = torch.as_tensor(j).shape[-2:]
    if needs_grad(j, h, g) or k > 4 or d > 4:
        return sym_solve(sym_matmul(j, h, dtype=dtype), g, eps=eps, dtype=dtype, out=out)
    dev, dtype, (j, h, g) = prepare(dtype, j, h, g)
    if h.shape[-1] == k * (k + 1) // 2:
        hk = _lib.MAT_SYM
    elif h.shape[-1] == k:
        hk = _lib.MAT_DIAG
    else:
        raise ValueError(f'hessian with {h.shape[-1]} components does not match k={k}')
    if g.shape[-1] != d:
        raise ValueError(f'gradient with {g.shape[-1]} components does not match d={d}')
    batch = broadcast_shapes(j.shape[:-2], h.shape[:-1], g.shape[:-1])
    out, _ = _alloc_out(out, tuple(batch) + (d,), dtype, dev, like=g)
    b = Batch(batch, [expand_batch(batch, j, 2), expand_batch(batch, h, 1), expand_batch(batch, g, 1), out],
              [2, 1, 1, 1])
    launch(_lib.lib().nfm_sym_matmul_solve, dev, dtype, (k, d, hk), b, tail=(_eps_array(eps, d),))
    return out


# ---------------------------------------------------------------- spectral functions (extension)
def _funm_cap(dtype, backward):
    """largest order with a kernel: the compiled table of the library (`nfm_sym_funm_max_order`)"""
    return max_order('nfm_sym_funm_max_order', dtype, bool(backward))


def _funm_args(fn, p, min):
    from math import isfinite
    if fn not in _lib.FUN:
        raise ValueError(f"fn must be one of {sorted(_lib.FUN)}, got {fn!r}")
    if fn == 'pow':
        if p is None:
            raise ValueError("fn='pow' needs the exponent p")
        p = float(p)
        if not isfinite(p):
            raise ValueError('p must be finite')
    else:
        p = 0.0
    if min is None:
        if fn == 'clamp':
            raise ValueError("fn='clamp' needs min")
    else:
        min = float(min)
        if not isfinite(min):
            raise ValueError('min must be finite')
    return _lib.FUN[fn], p, min


def _deliver(res, out):
    if out is None:
        return res
    if tuple(out.shape) != tuple(res.shape) or out.dtype != res.dtype or out.device != res.device:
        raise ValueError('out must have the shape, the computation dtype and the device of the result')
    return out.copy_(res)


def _funm_forward(mat, code, p, vmin, dtype, out):
    dev, dtype, (mat,) = prepare(dtype, mat)
    M = _nb_prm(mat.shape[-1])
    if M > _funm_cap(dtype, False):          # no kernel at this order: torch.linalg.eigh on the device (_symfun.py)
        from . import _symfun
        return _deliver(_symfun.forward(mat, code, p, vmin), out)
    batch = mat.shape[:-1]
    out, _ = _alloc_out(out, tuple(mat.shape), dtype, dev, like=mat)
    b = Batch(batch, [mat, out], [1, 1])
    launch(_lib.lib().nfm_sym_funm, dev, dtype, (M, code, p, int(vmin is not None), 0.0 if vmin is None else vmin), b)
    return out


def _funm_backward(mat, gout, code, p, vmin, dtype):
    dev, dtype, (mat, gout) = prepare(dtype, mat, gout)
    M = _nb_prm(mat.shape[-1])
    if M > _funm_cap(dtype, True):
        from . import _symfun
        return _symfun.backward(mat, gout, code, p, vmin)
    batch = mat.shape[:-1]
    gmat, _ = _alloc_out(None, tuple(mat.shape), dtype, dev, like=mat)
    b = Batch(batch, [mat, expand_batch(batch, gout, 1), gmat], [1, 1, 1])
    launch(_lib.lib().nfm_sym_funm_backward, dev, dtype,
           (M, code, p, int(vmin is not None), 0.0 if vmin is None else vmin), b)
    return gmat


def sym_funm(mat, fn, p=None, min=None, dtype=None, out=None):
    r"""EXTENSION (not in the reference): `f(A)` of compact symmetric matrices, compact in and compact out.

    `A = V diag(l) V^T` per matrix, in the registers of one lane (the fast arithmetic of `qr.eig_sym`); the result is
    `V diag(f(max(l, min))) V^T`.  One read of the `K = M(M+1)/2` values and one write, instead of
    `sym_to_full` -> `eig_sym(compute_u=True)` -> dense products -> repack.

    Parameters
    ----------
    mat : `(..., M*(M+1)//2) tensor`
    fn : {'exp', 'log', 'sqrt', 'rsqrt', 'pow', 'clamp'}
    p : `float`, the exponent of 'pow' (required there, ignored otherwise)
    min : `float`, optional (required by 'clamp')
        The eigenvalues are replaced by `max(l, min)` before `f`: `sym_clampm` is the projection onto
        `{A >= min I}`, and `sym_logm(x, min=1e-6)` a safe logarithm of a nearly singular field.
    dtype, out : as `sym_det`; `out=mat` (in place) is allowed.

    Domains, judged after the clamp: 'exp' and 'clamp' take any eigenvalue; 'log', 'rsqrt' and 'pow' with `p < 0`
    need `l > 0`; 'sqrt' and 'pow' with `p >= 0` need `l >= 0`.  A matrix with an eigenvalue outside the domain, or
    with an entry that is not finite, gives NaN in every component of its result and of its gradient; its neighbours
    are untouched.  No exception, no host synchronisation: a call (forward and backward) can be captured in a graph.

    Differentiable once with respect to `mat`.  The gradient is the Daleckii-Krein form
    `V [(V^T G V) o F] V^T` with closed-form divided differences `F`, regular at repeated and clustered
    eigenvalues, in the compact convention of the module (what autograd gives for `pack(f(sym_to_full(x)))`).
    Orders above the compiled caps (8; 7 for the float64 gradient) run `torch.linalg.eigh` on the device.
    """
    code, p, vmin = _funm_args(fn, p, min)
    _nb_prm(torch.as_tensor(mat).shape[-1])
    if needs_grad(mat):
        _grad_guard(out)
        from ._autograd import SymFunmFn
        return SymFunmFn.apply(torch.as_tensor(mat), code, p, vmin, dtype)
    return _funm_forward(mat, code, p, vmin, dtype, out)


def sym_expm(mat, min=None, dtype=None, out=None):
    """EXTENSION: matrix exponential of compact symmetric matrices (`sym_funm(mat, 'exp')`)."""
    return sym_funm(mat, 'exp', min=min, dtype=dtype, out=out)


def sym_logm(mat, min=None, dtype=None, out=None):
    """EXTENSION: matrix logarithm of compact SPD matrices (`sym_funm(mat, 'log')`)."""
    return sym_funm(mat, 'log', min=min, dtype=dtype, out=out)


def sym_sqrtm(mat, min=None, dtype=None, out=None):
    """EXTENSION: `A^(1/2)` of compact positive semi-definite matrices (`sym_funm(mat, 'sqrt')`)."""
    return sym_funm(mat, 'sqrt', min=min, dtype=dtype, out=out)


def sym_rsqrtm(mat, min=None, dtype=None, out=None):
    """EXTENSION: `A^(-1/2)` of compact SPD matrices (`sym_funm(mat, 'rsqrt')`)."""
    return sym_funm(mat, 'rsqrt', min=min, dtype=dtype, out=out)


def sym_powm(mat, p, min=None, dtype=None, out=None):
    """EXTENSION: `A^p` of compact positive (semi-)definite matrices (`sym_funm(mat, 'pow', p)`)."""
    return sym_funm(mat, 'pow', p=p, min=min, dtype=dtype, out=out)


def sym_clampm(mat, min, dtype=None, out=None):
    """EXTENSION: projection onto `{A >= min I}`: the eigenvalues clamped from below (`sym_funm(mat, 'clamp')`)."""
    return sym_funm(mat, 'clamp', min=min, dtype=dtype, out=out)


# ---------------------------------------------------------------- sorted eigendecomposition (extension)
def _eigh_cap(dtype, op):
    """largest order with a kernel for `op`: the compiled table of the library (`nfm_sym_eigh_max_order`)"""
    return max_order('nfm_sym_eigh_max_order', dtype, op)


def _eigh_order(order):
    if order not in _lib.EIGH_ORDER:
        raise ValueError(f"order must be one of {sorted(_lib.EIGH_ORDER)}, got {order!r}")
    return _lib.EIGH_ORDER[order]


def _alloc_field(out, shape, dtype, device, like):
    """`_alloc_out` for a result with the batch of `like` and another number of components: a channel-first
    (component-major) `like` hands its dim order on, as `_alloc_out` does for a result of its own shape"""
    if (out is None and tuple(like.shape) != tuple(shape) and tuple(like.shape[:-1]) == tuple(shape[:-1])
            and like.dim() >= 2 and like.stride(-1) != 1 and like.numel() > 0 and 0 not in like.stride()
            and torch.empty_like(like, device='meta').stride() == like.stride()):
        perm = sorted(range(like.dim()), key=lambda d: (-like.stride(d), d))
        inv = [perm.index(d) for d in range(like.dim())]
        return torch.empty([shape[d] for d in perm], dtype=dtype, device=device).permute(inv), None
    return _alloc_out(out, shape, dtype, device, like=like)


def _eigh_forward(mat, order, vectors, dtype, out):
    """values `(..., M)`, or with `vectors` the pair (values, vectors): two views of one packed `(..., M + M*M)`"""
    dev, dtype, (mat,) = prepare(dtype, mat)
    M = _nb_prm(mat.shape[-1])
    if M > _eigh_cap(dtype, _lib.EIGH_OP_VECTORS if vectors else _lib.EIGH_OP_VALUES):
        from . import _symeig          # no kernel at this order: torch.linalg.eigh on the device
        res = _symeig.forward(mat, order, vectors)
        return res if vectors else _deliver(res, out)
    batch = mat.shape[:-1]
    if vectors:
        packed = torch.empty(tuple(batch) + (M + M * M,), dtype=dtype, device=dev)
        b = Batch(batch, [mat, packed], [1, 1])
        launch(_lib.lib().nfm_sym_eigh, dev, dtype, (M, order | _lib.EIGH_VECTORS), b)
        return packed[..., :M], packed[..., M:].unflatten(-1, (M, M))
    out, _ = _alloc_field(out, tuple(batch) + (M,), dtype, dev, mat)
    b = Batch(batch, [mat, out], [1, 1])
    launch(_lib.lib().nfm_sym_eigh, dev, dtype, (M, order), b)
    return out


def _eigh_backward(mat, glam, gvec, order, dtype):
    """the compact gradient for the cotangents of the values and / or of the vectors (either may be None)"""
    dev, dtype, (mat, glam, gvec) = prepare(dtype, mat, glam, gvec)
    M = _nb_prm(mat.shape[-1])
    if M > _eigh_cap(dtype, _lib.EIGH_OP_VALUES_BACKWARD if gvec is None else _lib.EIGH_OP_BACKWARD):
        from . import _symeig
        if M > _eigh_cap(dtype, _lib.EIGH_OP_VECTORS):
            return _symeig.backward(mat, glam, gvec, order)
        # the split route: the forward kernel recomputes the decomposition (its order and its signs, which another
        # solver does not reproduce where a sign is decided by a tie) and torch applies the formula
        lam, V = _eigh_forward(mat, order, True, dtype, None)
        return _symeig.backward_from(lam, V, ~torch.isfinite(mat).all(-1), glam, gvec)
    batch = mat.shape[:-1]
    gmat, _ = _alloc_out(None, tuple(mat.shape), dtype, dev, like=mat)
    if glam is None:               # a stride-0 record of zeros
        glam = torch.zeros(M, dtype=dtype, device=dev)
    glam = expand_batch(batch, glam, 1)
    if gvec is None:
        b = Batch(batch, [mat, glam, gmat], [1, 1, 1])
        launch(_lib.lib().nfm_sym_eigh_backward, dev, dtype, (M, order), b, slots=(0, 1, None, 2))
    else:
        # one row-major record of M * M values (a view unless the two matrix dims cannot be merged)
        gvec = expand_batch(batch, gvec, 2).reshape(tuple(batch) + (M * M,))
        b = Batch(batch, [mat, glam, gvec, gmat], [1, 1, 1, 1])
        launch(_lib.lib().nfm_sym_eigh_backward, dev, dtype, (M, order | _lib.EIGH_VECTORS), b)
    return gmat


def sym_eigvals(mat, order='ascending', dtype=None, out=None):
    r"""EXTENSION (not in the reference): the eigenvalues of compact symmetric matrices, sorted.

    One read of the `K = M(M+1)/2` values and one write of `M`, the decomposition in the registers of one lane (the
    fast arithmetic of `qr.eig_sym`, which scales: every finite matrix is in range), instead of
    `sym_to_full` -> `eig_sym` -> a sort in torch.

    Parameters
    ----------
    mat : `(..., M*(M+1)//2) tensor`
    order : {'ascending', 'descending', 'abs'}
        'ascending' is the order of `torch.linalg.eigh`; 'abs' sorts ascending by `|l|`, ties by the value ascending
        (`|l1| <= |l2| <= |l3|`, the Frangi / Sato convention of Hessian filters).
    dtype, out : as `sym_det`.  A channel-first field hands its layout on to the values and to the gradient.

    Returns `(..., M)`.  A matrix with an entry that is not finite gives NaN in all its values and in its gradient;
    its neighbours are untouched.  No exception, no host synchronisation: forward and backward can be captured in a
    graph.

    Differentiable once with respect to `mat` (only `mat` is saved; the backward pass recomputes the decomposition):
    the gradient is `V diag(g) V^T` in the compact convention of the module, what autograd gives through
    `sym_to_full`.  See `sym_eigh` for the gap rule of the eigenvectors' gradient.
    Orders above the compiled caps (8) run `torch.linalg.eigh` on the device.
    """
    code = _eigh_order(order)
    _nb_prm(torch.as_tensor(mat).shape[-1])
    if needs_grad(mat):
        _grad_guard(out)
        from ._autograd import SymEighFn
        return SymEighFn.apply(torch.as_tensor(mat), code, False, dtype)
    return _eigh_forward(mat, code, False, dtype, out)


def sym_eigh(mat, order='ascending', dtype=None):
    r"""EXTENSION (not in the reference): eigenvalues `(..., M)` and eigenvectors `(..., M, M)` of compact symmetric
    matrices, sorted as `sym_eigvals`; column `k` of the vectors belongs to value `k`.

    Signs: the component of largest magnitude of each returned eigenvector is positive (the first such component
    among exact ties); the rule is applied after the sort.  Bad records, range and graph capture as `sym_eigvals`
    (NaN in the values, the vectors and the gradient).  The two results are views of one packed tensor.

    Differentiable once with respect to `mat`; the backward pass recomputes the decomposition with the same code, so
    with the same order and signs.  For the cotangents `gl` and `gV` (either may be absent): `B = V^T gV`,
    `W_kk = gl_k`, `W_kl = (B_kl - B_lk) / (2 (l_l - l_k))`, `S = V W V^T`, returned as `S_ii` and `2 S_ij`.

    THE GAP RULE: a pair of eigenvalues with `|l_k - l_l| <= 16 M eps max_i |l_i|` gets `W_kl = 0`.  `16 M eps` is the
    bar the sweeps are held to; closer pairs are numerically one eigenspace.  The gradient is therefore finite for
    every finite matrix, isotropic and repeated ones included, and exact for any loss that does not depend on the
    choice of basis inside an eigenspace.

    Orders above the compiled caps (8) run `torch.linalg.eigh` on the device with the same sort, sign rule and
    gradient formula.  An order with a forward kernel and no backward kernel (8 for the float64 gradient with `gV`)
    recomputes the decomposition with the forward kernel and applies the formula in torch.
    """
    code = _eigh_order(order)
    _nb_prm(torch.as_tensor(mat).shape[-1])
    if needs_grad(mat):
        from ._autograd import SymEighFn
        return SymEighFn.apply(torch.as_tensor(mat), code, True, dtype)
    return _eigh_forward(mat, code, True, dtype, None)


# ---------------------------------------------------------------- Cholesky kernels (extension)
def _chol_cap(dtype, cls):
    """largest order with a kernel for the class: the compiled table of the library (`nfm_sym_chol_max_order`)"""
    return max_order('nfm_sym_chol_max_order', dtype, cls)


def _chol_shapes(mat, vec):
    """(M, K) of the compact matrix, checked against the vector"""
    K = torch.as_tensor(mat).shape[-1]
    M = _nb_prm(K)
    if vec is not None and torch.as_tensor(vec).shape[-1] != M:
        raise ValueError(f'vec has {torch.as_tensor(vec).shape[-1]} components, a matrix of {K} compact values '
                         f'is of order {M}')
    return M, K


def _chol_route(name, dtype, mat, vec=None, **kw):
    """the torch composition (`_symchol.py`) on the device: orders without a kernel, forward or backward, and the second
    derivatives of the factor"""
    from . import _symchol
    _, _, ts = prepare(dtype, mat, vec, grad_ok=True)
    return getattr(_symchol, name)(*[t for t in ts if t is not None], **kw)


_CHOL_ROUTE = {_lib.CHOL_FACTOR: ('chol', {}), _lib.CHOL_LOGDET: ('logdet', {}),
               _lib.CHOL_MAHA: ('mahalanobis', {'squared': True}), _lib.CHOL_MAHA_SQRT: ('mahalanobis', {'squared': False}),
               _lib.CHOL_LOGPDF: ('gauss_logpdf', {})}


def _chol_forward(op, cls, mat, vec, dtype, out, route):
    """one forward launch of `nfm_sym_chol`: the factor `(..., K)`, an applied vector `(..., M)` or a scalar `(...)`"""
    dev, dtype, (mat, vec) = prepare(dtype, mat, vec)
    M, K = _chol_shapes(mat, vec)
    if M > _chol_cap(dtype, cls):                # no kernel at this order: the torch composition (_symchol.py)
        name, kw = route
        from . import _symchol
        return _deliver(getattr(_symchol, name)(*([mat] if vec is None else [mat, vec]), **kw), out)
    batch = mat.shape[:-1] if vec is None else broadcast_shapes(mat.shape[:-1], vec.shape[:-1])
    if cls == _lib.CHOL_CLASS_FACTOR:
        out, _ = _alloc_out(out, tuple(mat.shape), dtype, dev, like=mat)
        nco = 1
    elif cls == _lib.CHOL_CLASS_APPLY:
        out, _ = _alloc_field(out, tuple(batch) + (M,), dtype, dev, vec)
        nco = 1
    else:
        out, _ = _alloc_out(out, tuple(batch), dtype, dev)
        nco = 0
    if vec is None:
        b = Batch(batch, [mat, out], [1, nco])
        launch(_lib.lib().nfm_sym_chol, dev, dtype, (M, op), b, slots=(0, None, 1))
    else:
        b = Batch(batch, [expand_batch(batch, mat, 1), expand_batch(batch, vec, 1), out], [1, 1, nco])
        launch(_lib.lib().nfm_sym_chol, dev, dtype, (M, op), b)
    return out


def _chol_backward(op, mat, vec, gout, dtype):
    """the packed gradient `(..., K + M)` (`sym_logdet`: `(..., K)`) of a scalar op for the cotangent `gout`"""
    dev, dtype, (mat, vec, gout) = prepare(dtype, mat, vec, gout)
    M, K = _chol_shapes(mat, vec)
    batch = tuple(gout.shape)
    packed = torch.empty(batch + (K + (0 if vec is None else M),), dtype=dtype, device=dev)
    gout = gout.contiguous()
    if vec is None:
        b = Batch(batch, [expand_batch(batch, mat, 1), gout, packed], [1, 0, 1])
        launch(_lib.lib().nfm_sym_chol_backward, dev, dtype, (M, op), b, slots=(0, None, 1, 2))
    else:
        b = Batch(batch, [expand_batch(batch, mat, 1), expand_batch(batch, vec, 1), gout, packed], [1, 1, 0, 1])
        launch(_lib.lib().nfm_sym_chol_backward, dev, dtype, (M, op), b)
    return packed


def _chol_scalar(op, mat, vec, dtype, out):
    M, _ = _chol_shapes(mat, vec)
    route = _CHOL_ROUTE[op]
    if needs_grad(mat, vec):
        _grad_guard(out)
        _, cdt, _ = prepare(dtype, mat, vec, grad_ok=True)
        if M > min(_chol_cap(cdt, _lib.CHOL_CLASS_SCALAR), _chol_cap(cdt, _lib.CHOL_CLASS_BACKWARD)):
            return _chol_route(route[0], dtype, mat, vec, **route[1])     # torch differentiates the composition
        from ._autograd import SymCholFn
        return SymCholFn.apply(torch.as_tensor(mat), None if vec is None else torch.as_tensor(vec), op, dtype)
    return _chol_forward(op, _lib.CHOL_CLASS_SCALAR, mat, vec, dtype, out, route)


def _chol_grad_cap(dtype, cls):
    """largest order with a backward kernel for the factor (`CHOL_CLASS_FACTOR`) or an apply op (`CHOL_CLASS_APPLY`)"""
    return max_order('nfm_sym_chol_grad_max_order', dtype, cls)


def _chol_grad_fits(dtype, mat, vec, cls):
    """the order has a forward and a backward kernel for the class in the computing dtype"""
    M, _ = _chol_shapes(mat, vec)
    _, cdt, _ = prepare(dtype, mat, vec, grad_ok=True)
    return M <= min(_chol_cap(cdt, cls), _chol_grad_cap(cdt, cls))


def _chol_grad(op, mat, vec, gout, dtype):
    """one launch of `nfm_sym_chol_grad`: the packed gradient `(..., K)` of the factor, or `(..., K + M)` of an apply op,
    for the cotangent `gout` (of the broadcast batch shape)"""
    dev, dtype, (mat, vec, gout) = prepare(dtype, mat, vec, gout)
    M, K = _chol_shapes(mat, vec)
    batch = tuple(gout.shape[:-1])
    packed = torch.empty(batch + (K + (0 if vec is None else M),), dtype=dtype, device=dev)
    gout = gout.contiguous()
    if vec is None:
        b = Batch(batch, [expand_batch(batch, mat, 1), gout, packed], [1, 1, 1])
        launch(_lib.lib().nfm_sym_chol_grad, dev, dtype, (M, op), b, slots=(0, None, 1, 2))
    else:
        b = Batch(batch, [expand_batch(batch, mat, 1), expand_batch(batch, vec, 1), gout, packed], [1, 1, 1, 1])
        launch(_lib.lib().nfm_sym_chol_grad, dev, dtype, (M, op), b)
    return packed


def sym_chol(mat, dtype=None, out=None):
    r"""EXTENSION (not in the reference): the Cholesky factor of compact symmetric positive definite matrices.

    Returns `(..., K)`, `K = M(M+1)/2`: the lower factor `L` with `A = L L^T`, `L_ij` (`i >= j`) stored where the
    compact layout stores `(i, j)`, so `sym_diag` of the result is the diagonal of `L`.  One read of the `K` values and
    one write, the factorisation in the registers of one lane.

    BAD RECORDS (all the Cholesky functions): a matrix (or vector) with an entry that is not finite, or with a pivot
    `d_j = a_jj - sum_k l_jk^2` that is not `> 0` (NaN, zero and negative included), gives NaN in every value of its
    result and of its gradient; its neighbours are untouched.  No exception, no host synchronisation: a call can be
    captured in a graph.  Nothing is scaled: `sym_chol(s^2 A) == s * sym_chol(A)` bit for bit for a power of two `s`.

    dtype, out : as `sym_det`; `out=mat` (in place) is allowed.

    Differentiable: with `requires_grad` the same forward kernel runs (the same bits) and one backward kernel pulls the
    cotangent `G` of the factor (compact, one value per stored `L_ij`) back to
    `S = L^-T (P + P^T) L^-1 / 2`, `P` = the lower triangle of `L^T G` with a halved diagonal, returned as `S_ii`,
    `2 S_ij`.  Nothing is saved but `mat`: the backward kernel factors again in registers, which costs no memory traffic
    (the C entry also takes the factor itself, `NFM_CHOL_FACTORED`).  A record with a cotangent entry that is not finite
    is NaN in its gradient.  A second derivative
    (`create_graph=True`) differentiates the torch composition on the device (`torch.linalg.cholesky_ex`), which is
    also what orders above the compiled cap (8) run, forward and backward.
    """
    _chol_shapes(mat, None)
    if needs_grad(mat):
        _grad_guard(out)
        if not _chol_grad_fits(dtype, mat, None, _lib.CHOL_CLASS_FACTOR):
            return _chol_route('chol', dtype, mat)
        from ._autograd import SymCholFactorFn
        return SymCholFactorFn.apply(torch.as_tensor(mat), dtype)
    return _chol_forward(_lib.CHOL_FACTOR, _lib.CHOL_CLASS_FACTOR, mat, None, dtype, out, _CHOL_ROUTE[_lib.CHOL_FACTOR])


def sym_chol_apply(mat, vec, op, factored=False, dtype=None, out=None):
    r"""EXTENSION: apply the Cholesky factor of compact SPD matrices `(..., K)` to vectors `(..., M)`.

    op : 'L' for `L v` (colouring a white sample), 'LT' for `L^T v`, 'Linv' for `L^-1 v` (whitening), 'LTinv' for
        `L^-T v`.
    factored : `mat` already is the result of `sym_chol`, so one factorisation serves many vectors (same bits).
    Either operand may be broadcast, as in `sym_matvec`.  Bad records, `dtype`, `out` as `sym_chol`.

    Differentiable in `mat` and `vec`: the forward kernel (the same bits as without `requires_grad`), and one backward
    kernel that saves nothing but the two inputs and recomputes the factor and the result.  With the cotangent `g` and
    the result `y`: 'L' `g_v = L^T g`, `G = tril(g v^T)`; 'LT' `g_v = L g`, `G = tril(v g^T)`; 'Linv' `g_v = L^-T g`,
    `G = -tril(g_v y^T)`; 'LTinv' `g_v = L^-1 g`, `G = -tril(y g_v^T)`.  With `factored` the gradient of `mat` is `G`
    itself (one value per stored entry of the factor); without, `G` is pulled back to `A` in the same lane as in
    `sym_chol`.  The gradient of a broadcast operand is summed to its shape.  Second derivatives and orders above 8 as
    `sym_chol`.
    """
    if op not in _lib.CHOL_APPLY:
        raise ValueError(f"op must be one of {sorted(_lib.CHOL_APPLY)}, got {op!r}")
    _chol_shapes(mat, vec)
    code = _lib.CHOL_APPLY[op] | (_lib.CHOL_FACTORED if factored else 0)
    if needs_grad(mat, vec):
        _grad_guard(out)
        if not _chol_grad_fits(dtype, mat, vec, _lib.CHOL_CLASS_APPLY):
            return _chol_route('chol_apply', dtype, mat, vec, op=op, factored=bool(factored))
        from ._autograd import SymCholApplyFn
        return SymCholApplyFn.apply(torch.as_tensor(mat), torch.as_tensor(vec), op, bool(factored), dtype)
    return _chol_forward(code, _lib.CHOL_CLASS_APPLY, mat, vec, dtype, out,
                         ('chol_apply', {'op': op, 'factored': bool(factored)}))


def sym_logdet(mat, dtype=None, out=None):
    r"""EXTENSION: `log det A = 2 sum_i log L_ii` of compact SPD matrices, `(...)`.  Finite wherever `A` and its root
    are (the determinant itself overflows float32 at 8x8 with entries of 1e6); NaN, not `-inf`, for a singular record.

    Differentiable once (one backward kernel, nothing but `mat` saved): `S = g A^-1`, returned as `S_ii`, `2 S_ij`.
    Bad records, `dtype`, `out` and orders above the cap as `sym_chol`.
    """
    return _chol_scalar(_lib.CHOL_LOGDET, mat, None, dtype, out)


def sym_mahalanobis(mat, vec, squared=True, dtype=None, out=None):
    r"""EXTENSION: `v^T A^-1 v = |L^-1 v|^2` of compact SPD matrices and vectors, `(...)`, or its root with
    `squared=False`.  One pass: `K + M` values read, one written.  Either operand may be broadcast.

    Differentiable once in `mat` and `vec`: with `w = A^-1 v`, `S = -g w w^T` and `g_v = 2 g w`; for the root the same
    with `g / (2 d)`, exactly zero where `d = 0` (finite at `v = 0`).  Bad records, `dtype`, `out` as `sym_chol`.
    """
    return _chol_scalar(_lib.CHOL_MAHA if squared else _lib.CHOL_MAHA_SQRT, mat, vec, dtype, out)


def sym_gauss_logpdf(mat, resid, dtype=None, out=None):
    r"""EXTENSION: the Gaussian log-density `-(M log 2 pi + log det A + r^T A^-1 r) / 2` of residuals `(..., M)` under
    compact covariances `(..., K)`, `(...)`.  One pass: `K + M` values read, one written.

    Differentiable once in `mat` and `resid`: `S = -g (A^-1 - w w^T) / 2`, `g_r = -g w`, `w = A^-1 r`.  Bad records,
    `dtype`, `out` as `sym_chol`.
    """
    return _chol_scalar(_lib.CHOL_LOGPDF, mat, resid, dtype, out)


# ---------------------------------------------------------------- two-matrix spectral functions (extension)
_PENCIL_FUNS = ('exp', 'log', 'sqrt', 'rsqrt', 'pow')


def _pencil_cap(dtype, op):
    """largest order with a kernel: the compiled table of the library (`nfm_sym_pencil_max_order`)"""
    return max_order('nfm_sym_pencil_max_order', dtype, op)


def _pencil_order(base, mat):
    base, mat = torch.as_tensor(base), torch.as_tensor(mat)
    if base.shape[-1] != mat.shape[-1]:
        raise ValueError(f'the two matrices have {base.shape[-1]} and {mat.shape[-1]} components: not the same order')
    return _nb_prm(mat.shape[-1])


def _pencil_args(fn, p, min=None, clamp=None):
    if min is not None or clamp is not None:
        raise ValueError('a pencil function takes no min / clamp: clamp the operands with sym_clampm first')
    if fn not in _PENCIL_FUNS:
        raise ValueError(f"fn must be one of {sorted(_PENCIL_FUNS)}, got {fn!r}")
    code, p, _ = _funm_args(fn, p, None)
    return code, p


def _pencil_batch(base, mat, *more):
    batch = broadcast_shapes(base.shape[:-1], mat.shape[:-1], *[m.shape[:-1] for m in more])
    like = mat if tuple(mat.shape[:-1]) == tuple(batch) else base
    return batch, like


def _pencil_forward(base, mat, code, p, dtype, out):
    dev, dtype, (base, mat) = prepare(dtype, base, mat)
    M = _pencil_order(base, mat)
    if M > _pencil_cap(dtype, _lib.PENCIL_OP_FUNM):      # no kernel at this order: the composition (_sympencil.py)
        from . import _sympencil
        return _deliver(_sympencil.pencil_funm(base, mat, code, p), out)
    batch, like = _pencil_batch(base, mat)
    out, _ = _alloc_out(out, tuple(batch) + (mat.shape[-1],), dtype, dev, like=like)
    b = Batch(batch, [expand_batch(batch, base, 1), expand_batch(batch, mat, 1), out], [1, 1, 1])
    launch(_lib.lib().nfm_sym_pencil_funm, dev, dtype, (M, code, p, 0, 0.0), b)
    return out


def _pencil_backward(base, mat, gout, code, p, dtype):
    """gradient with respect to `mat`, of the broadcast batch shape (the composition above the cap: of `mat`'s own
    shape; the caller sums to the input's shape either way)"""
    dev, dtype, (base, mat, gout) = prepare(dtype, base, mat, gout)
    M = _pencil_order(base, mat)
    if M > _pencil_cap(dtype, _lib.PENCIL_OP_FUNM_BACKWARD):
        return _pencil_grad_composed(base, mat, gout, code, p, 1)
    batch, like = _pencil_batch(base, mat, gout)
    gmat, _ = _alloc_out(None, tuple(batch) + (mat.shape[-1],), dtype, dev, like=like)
    b = Batch(batch, [expand_batch(batch, base, 1), expand_batch(batch, mat, 1), expand_batch(batch, gout, 1), gmat],
              [1, 1, 1, 1])
    launch(_lib.lib().nfm_sym_pencil_funm_backward, dev, dtype, (M, code, p, 0, 0.0), b)
    return gmat


def _pencil_grad_composed(base, mat, gout, code, p, which):
    """gradient of the composition (_sympencil.py) with respect to base (which = 0) or mat (1), input-shaped"""
    from . import _sympencil
    with torch.enable_grad():
        ops = [base.detach(), mat.detach()]
        ops[which] = ops[which].requires_grad_(True)
        y = _sympencil.pencil_funm(ops[0], ops[1], code, p)
        (g,) = torch.autograd.grad(y, ops[which], gout.expand(y.shape))
    return g


def _pencil_eig(base, mat, mode, dtype, out=None):
    dev, dtype, (base, mat) = prepare(dtype, base, mat)
    M = _pencil_order(base, mat)
    if M > _pencil_cap(dtype, _lib.PENCIL_OP_EIG):
        from . import _sympencil
        res = (_sympencil.geneigvals(base, mat) if mode == _lib.PENCIL_EIG
               else _sympencil.dist(base, mat, squared=mode == _lib.PENCIL_DIST2))
        return _deliver(res, out)
    batch, _ = _pencil_batch(base, mat)
    if mode == _lib.PENCIL_EIG:
        out, _ = _alloc_out(out, tuple(batch) + (M,), dtype, dev)
        rec = out
    else:
        out, _ = _alloc_out(out, tuple(batch), dtype, dev)
        rec = out.unsqueeze(-1)
    b = Batch(batch, [expand_batch(batch, base, 1), expand_batch(batch, mat, 1), rec], [1, 1, 1])
    launch(_lib.lib().nfm_sym_pencil_eig, dev, dtype, (M, mode), b)
    return out


def _pencil_dist_backward(base, mat, gout, mode, dtype):
    """(gradient with respect to base, with respect to mat) of the distance, both of the broadcast batch shape: two
    views of one (..., 2, K) tensor (the composition above the cap: each of its input's own shape, already summed over
    the broadcast dims; the caller sums to the input's shape either way, a no-op there)"""
    dev, dtype, (base, mat, gout) = prepare(dtype, base, mat, gout)
    M = _pencil_order(base, mat)
    batch, _ = _pencil_batch(base, mat)
    if M > _pencil_cap(dtype, _lib.PENCIL_OP_DIST_BACKWARD):
        from . import _sympencil
        with torch.enable_grad():
            a, b = base.detach().requires_grad_(True), mat.detach().requires_grad_(True)
            d = _sympencil.dist(a, b, squared=mode == _lib.PENCIL_DIST2)
            ga, gb = torch.autograd.grad(d, (a, b), gout.expand(d.shape))
        return ga, gb
    K = mat.shape[-1]
    grads = torch.empty(tuple(batch) + (2, K), dtype=dtype, device=dev)
    b = Batch(batch, [expand_batch(batch, base, 1), expand_batch(batch, mat, 1),
                      expand_batch(batch, gout.unsqueeze(-1), 1), grads.view(tuple(batch) + (2 * K,))], [1, 1, 1, 1])
    launch(_lib.lib().nfm_sym_pencil_dist_backward, dev, dtype, (M, mode), b)
    return grads[..., 0, :], grads[..., 1, :]


def sym_pencil_funm(base, mat, fn, p=None, dtype=None, out=None, min=None, clamp=None):
    r"""EXTENSION (not in the reference): `A^{1/2} f(A^{-1/2} B A^{-1/2}) A^{1/2}` for compact `A = base` (symmetric
    positive definite) and compact symmetric `B = mat`, compact out, in ONE kernel.

    `A = V L V^T`, `W = V L^{-1/2}`, `W^T B W = Q M Q^T`: the `mu_i` are the generalised eigenvalues of
    `B x = mu A x`, and the result is `Z f(M) Z^T` with `Z = V L^{1/2} Q`.  Both decompositions stay in the registers
    of one lane: each record is read once and the result written once, instead of the chain
    `sym_rsqrtm -> sym_to_full -> sym_matmul -> sym_funm -> sym_matmul` and its three decompositions.

    Parameters
    ----------
    base, mat : `(..., M*(M+1)//2) tensor`; the batch dims broadcast without a copy
    fn : {'exp', 'log', 'sqrt', 'rsqrt', 'pow'}; `p` : the exponent of 'pow'
        'pow' with exponent t is the point `A #_t B` of the geodesic, 'log' / 'exp' the Riemannian log / exp map at A.
        There is no `min` / `clamp` here (a `ValueError`).
    dtype, out : as `sym_funm`; `out=mat` is allowed.

    A record with an entry that is not finite, a base that is not positive definite, or a `mu` outside the domain
    of `f` gives NaN in every component of its result and gradients; its neighbours are untouched.  No exception, no
    host synchronisation: a call (forward and backward) can be captured in a graph.

    Differentiable once.  With respect to `mat`: `X [(Z^T G Z) o F] X^T`, `X = Z^{-T}`, with the closed-form divided
    differences of `sym_funm`, regular at repeated `mu`.  With respect to `base` for 'pow' / 'sqrt' / 'rsqrt': the
    same kernel through `A #_t B = B #_{1-t} A` (which needs `mat` positive definite as well); for 'log' / 'exp':
    autograd through the composition of `sym_funm` calls.  Orders above the compiled caps
    (`nfm_sym_pencil_max_order`) run that composition throughout.
    """
    code, p = _pencil_args(fn, p, min, clamp)
    _pencil_order(base, mat)
    if needs_grad(base, mat):
        _grad_guard(out)
        from ._autograd import SymPencilFunmFn
        return SymPencilFunmFn.apply(torch.as_tensor(base), torch.as_tensor(mat), code, p, dtype)
    return _pencil_forward(base, mat, code, p, dtype, out)


def sym_geodesic(a, b, t, dtype=None, out=None):
    """EXTENSION: the point `a #_t b = a^{1/2} (a^{-1/2} b a^{-1/2})^t a^{1/2}` of the affine-invariant geodesic from
    `a` (t = 0) to `b` (t = 1), compact SPD in and out (`sym_pencil_funm(a, b, 'pow', t)`)."""
    return sym_pencil_funm(a, b, 'pow', p=t, dtype=dtype, out=out)


def sym_geomean(a, b, dtype=None, out=None):
    """EXTENSION: the geometric mean `a # b` of two compact SPD matrices (`sym_geodesic(a, b, 1/2)`)."""
    return sym_pencil_funm(a, b, 'sqrt', dtype=dtype, out=out)


def sym_logmap(base, mat, dtype=None, out=None):
    """EXTENSION: the Riemannian log map `Log_base(mat)` of the affine-invariant metric: the compact symmetric
    tangent vector at `base` that points to `mat` (`sym_pencil_funm(base, mat, 'log')`)."""
    return sym_pencil_funm(base, mat, 'log', dtype=dtype, out=out)


def sym_expmap(base, tangent, dtype=None, out=None):
    """EXTENSION: the Riemannian exp map `Exp_base(tangent)`, the inverse of `sym_logmap`; `tangent` is any compact
    symmetric matrix (`sym_pencil_funm(base, tangent, 'exp')`)."""
    return sym_pencil_funm(base, tangent, 'exp', dtype=dtype, out=out)


def sym_geneigvals(mat, base, dtype=None, out=None):
    """EXTENSION: the generalised eigenvalues of `mat x = mu base x`, ascending, `(..., M)`: compact symmetric `mat`,
    compact SPD `base` (the argument order of `scipy.linalg.eigh(a, b)`).  NaN records as `sym_pencil_funm`.
    With an operand that requires grad the composition of `sym_funm` calls and `torch.linalg.eigvalsh` runs."""
    _pencil_order(base, mat)
    if needs_grad(mat, base):
        _grad_guard(out)
        from . import _sympencil
        dev, dtype, (base, mat) = prepare(dtype, base, mat, grad_ok=True)
        return _sympencil.geneigvals(base, mat)
    return _pencil_eig(base, mat, _lib.PENCIL_EIG, dtype, out)


def sym_dist(a, b, squared=False, dtype=None, out=None):
    r"""EXTENSION: the affine-invariant distance `d(a, b) = ||log(a^{-1/2} b a^{-1/2})||_F` of compact SPD matrices
    (`squared=True`: `d^2 = sum_i log^2 mu_i`), `(...)`.

    Differentiable once with respect to both, by closed forms with no divided difference:
    `d d^2 / d b = X diag(2 log mu / mu) X^T`, `d d^2 / d a = -X diag(2 log mu) X^T`: finite, and exactly zero, at
    `a = b`.  The gradient of `d` itself carries the factor `1 / (2 d)` and is DEFINED as 0 at `d = 0` (a
    subgradient: `d` has a kink there); minimise `squared=True`.  NaN records as `sym_pencil_funm`.
    """
    _pencil_order(a, b)
    mode = _lib.PENCIL_DIST2 if squared else _lib.PENCIL_DIST
    if needs_grad(a, b):
        _grad_guard(out)
        from ._autograd import SymDistFn
        return SymDistFn.apply(torch.as_tensor(a), torch.as_tensor(b), mode, dtype)
    return _pencil_eig(a, b, mode, dtype, out)


def sym_karcher_mean(mats, dim=0, weights=None, max_iter=8):
    r"""EXTENSION: the Karcher (Frechet) mean of compact SPD matrices along `dim` under the affine-invariant metric.

    Starts at the log-Euclidean mean `M = sym_expm(sum_i w_i sym_logm(A_i))` and repeats
    `M <- sym_expmap(M, sum_i w_i sym_logmap(M, A_i))` `max_iter` times; `M` is broadcast along `dim` with stride 0,
    so it is read in place.  A fixed number of iterations and no host synchronisation: capturable in a graph.
    Not differentiable.  The step-one iteration converges linearly, by a factor that grows with the squared geodesic
    diameter of the set: 8 steps reach the rounding level for matrices within about 0.5 of each other (`sym_dist`);
    widely dispersed sets want a larger `max_iter` (32 for distances around 2).

    mats : `(..., n, ..., K)` with the n matrices of a set along `dim` (not the last); weights : `(n,)`, optional
    (normalised to sum 1; default uniform) -> the input shape without `dim`.
    """
    mats = torch.as_tensor(mats)
    nd = mats.dim()
    dim = dim + nd if dim < 0 else dim
    if not 0 <= dim < nd - 1:
        raise ValueError(f'dim {dim} is not a batch dimension of a tensor with {nd} dimensions')
    n = mats.shape[dim]
    with torch.no_grad():
        mats = mats.detach()
        if weights is None:
            w = torch.full((n,), 1.0 / n, dtype=mats.dtype, device=mats.device)
        else:
            w = torch.as_tensor(weights, dtype=mats.dtype, device=mats.device)
            if w.shape != (n,):
                raise ValueError(f'weights must have shape ({n},), got {tuple(w.shape)}')
            w = w / w.sum()
        w = w.reshape((n,) + (1,) * (nd - 1 - dim))
        mean = sym_expm((w * sym_logm(mats)).sum(dim))
        for _ in range(int(max_iter)):
            step = (w * sym_logmap(mean.unsqueeze(dim).expand(mats.shape), mats)).sum(dim)
            mean = sym_expmap(mean, step)
    return mean
