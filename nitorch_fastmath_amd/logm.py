"""
Principal matrix logarithm of small matrices and the exponential barycentre on MI355X -- replaces
`nitorch_fastmath.lie.logm` (`_impl/logm.py:102`, scipy on the CPU, one matrix at a time) and
`nitorch_fastmath.lie.meanm` (`lie.py:13-93`).

One matrix per lane (`nfm_logm.hip`): inverse scaling and squaring with Denman-Beavers square roots and
the atanh series (quirk Q20 in DESIGN.md section 2).  Kernels: `logm` and `logm(M^-1 A)` at float32
orders 1..8 and float64 orders 1..7, the Frechet derivative of the logarithm at orders 1..5.  Every
other order runs the same algorithm in batched torch operations on the device (`_logm_torch`).

Deviations from the reference (Q21, Q22): the output has the input's dtype (the reference returns
float64); a matrix without a real principal logarithm (non-finite entry, singular, eigenvalue on the
closed negative real axis) gives NaN in every entry, where the reference returns the real part of a
complex result.
"""
__all__ = ['logm', 'meanm']
import warnings
import torch
from . import _lib
from ._dispatch import Batch, broadcast_shapes, expand_batch, launch, needs_grad, prepare

FORWARD_MAX = {torch.float32: 8, torch.float64: 7}   # orders with a logm / logm_solve kernel (include/nfm_hip.h)
FRECHET_MAX = 5                                       # orders with a Frechet kernel
THETA = 0.25                                          # square roots until ||A - I||_1 <= THETA
MAX_ITER = 40                                         # Denman-Beavers steps per square root
MAX_ROOTS = 64


def _square(M):
    if M.dim() < 2 or M.shape[-2] != M.shape[-1]:
        raise ValueError(f'expected square matrices, got {tuple(M.shape[-2:])}')
    return M.shape[-1]


def _dist1(X, eye):
    return (X - eye).abs().sum(-2).amax(-1)


def _tree_sum(x):
    """sum over the last dim by halving with elementwise adds: the order of the additions depends on that
    dim's length only, never on the batch around it (meanm's batched form is bit-identical to the loop)"""
    while x.shape[-1] > 1:
        n = x.shape[-1]
        h = n // 2
        y = x[..., :h] + x[..., h:2 * h]
        x = y if n == 2 * h else torch.cat([y, x[..., 2 * h:]], -1)
    return x[..., 0]


def _logm_torch(A):
    """The kernel's algorithm (Q20) in batched torch operations: the batch runs its largest number of square
    roots, steps and series terms, each matrix its own under per-matrix masks.  Differentiable by autograd (the
    roots end on the Frechet kernel's stop test, which waits for the derivative of M as well); same NaN policy.
    One host read per Denman-Beavers step (the loop ends when every matrix has converged) and one for the largest
    degree.  The arithmetic of a matrix does not involve its batch mates, but the library routines
    behind `matmul` / `inv_ex` may pick other kernels for another batch size: bit-for-bit independence of the
    batch is a property of the HIP kernels' orders only."""
    D = _square(A)
    fi = torch.finfo(A.dtype)
    eye = torch.eye(D, dtype=A.dtype, device=A.device)
    sqrt_eps = fi.eps ** 0.5

    def sel(mask, a, b):
        return torch.where(mask[..., None, None], a, b)

    bad = ~torch.isfinite(A).all(-1).all(-1)
    Y = sel(bad, eye, A)
    s = torch.zeros(A.shape[:-2], dtype=torch.int32, device=A.device)
    for _ in range(MAX_ROOTS):
        active = ~bad & (_dist1(Y.detach(), eye) > THETA)
        if not bool(active.any()):
            break
        M = sel(active, Y, eye)
        R = M
        conv = ~active
        was_near = torch.zeros_like(conv)
        for _ in range(MAX_ITER):
            e_prev = _dist1(M.detach(), eye)
            Mi = torch.linalg.inv_ex(M).inverse
            Rn = 0.5 * (R + R @ Mi)
            Mn = 0.5 * (eye + 0.5 * (M + Mi))
            fin = torch.isfinite(Mn.detach()).all(-1).all(-1)
            upd = ~conv
            bad = bad | (upd & ~fin)
            conv = conv | (upd & ~fin)
            upd = upd & fin
            R = sel(upd, Rn, R)
            M = sel(upd, Mn, sel(bad, eye, M))
            # the stop test of the kernel that carries the derivative (autograd or jvp may be differentiating these
            # steps): the second step in a row that started within sqrt(eps) ends the root, so that the derivative
            # of M, which lags M by a step and is of order one where M reaches I at once (unipotent A), is consumed
            near = e_prev <= sqrt_eps
            conv = conv | (upd & near & was_near)
            was_near = near
            if bool(conv.all()):
                break
        bad = bad | ~conv
        ok = active & ~bad
        Y = sel(ok, R, Y)
        s = s + ok.to(s.dtype)
    bad = bad | ~(_dist1(Y.detach(), eye) <= THETA)
    Y = sel(bad, eye, Y)
    Z = (Y - eye) @ torch.linalg.inv_ex(Y + eye).inverse
    # the degree of the series, per matrix: a coefficient mask, so that a matrix takes its own degree (as in the
    # kernel) whatever its batch mates need; one host read for the largest
    zn = Z.detach().abs().sum(-2).amax(-1)
    deg = torch.zeros_like(s)
    alive = torch.ones_like(bad)
    pw = zn
    for k in range(16):
        alive = alive & (pw > fi.eps * 0.125 * (2 * k + 1))
        deg = deg + alive.to(deg.dtype)
        pw = pw * zn * zn
    top = int(deg.max()) if deg.numel() else 0
    W = Z @ Z
    P = torch.zeros_like(Z)
    for k in range(top, -1, -1):
        P = (deg >= k).to(A.dtype)[..., None, None] * (eye / (2 * k + 1)) + W @ P
    out = torch.ldexp(Z @ P, (s + 1)[..., None, None])
    return sel(bad, torch.full_like(out, float('nan')), out)


def _logm(A, M=None):
    """logm(A), or logm(M^-1 A) with M broadcast over A's batch (no autograd): the kernel, or the torch route"""
    D = _square(A)
    if D > FORWARD_MAX[A.dtype]:
        return _logm_torch(A if M is None else torch.linalg.solve(M, A))
    dev = A.device
    ops = [A] if M is None else [M, A]
    batch = broadcast_shapes(*[t.shape[:-2] for t in ops])
    out = torch.empty(tuple(batch) + (D, D), dtype=A.dtype, device=dev)
    b = Batch(batch, [expand_batch(batch, t, 2) for t in ops] + [out], [2] * (len(ops) + 1))
    L = _lib.lib()
    launch(L.nfm_lie_logm if M is None else L.nfm_lie_logm_solve, dev, A.dtype, (D,), b)
    return out


def _frechet(X, G):
    """L_log(X, G), the Frechet derivative of the logarithm at X along G (no autograd; orders 1..FRECHET_MAX)"""
    D = _square(X)
    dev = X.device
    batch = broadcast_shapes(X.shape[:-2], G.shape[:-2])
    out = torch.empty(tuple(batch) + (D, D), dtype=X.dtype, device=dev)
    b = Batch(batch, [expand_batch(batch, X, 2), expand_batch(batch, G, 2), out], [2, 2, 2])
    launch(_lib.lib().nfm_lie_logm_frechet, dev, X.dtype, (D,), b)
    return out


def logm(mat):
    """Batched principal matrix logarithm.  Replaces `_impl/logm.py:102` (same signature).

    mat : `(..., N, N)` float32 / float64 GPU tensor (strided and broadcast views are read in place).
    Returns `(..., N, N)`, contiguous, in the input's dtype (Q21).  A matrix without a real principal
    logarithm gives NaN in every entry (Q22).  Differentiable: the backward is L_log(X^T, G), the Frechet
    kernel at orders 1..5 and autograd through the torch route above them.

    Accuracy (Q20; m = max(1, cond_log(X)), cond_log = ||L_log(X)||_2 ||X||_F / ||log X||_F): the relative
    Frobenius error is within 128 eps m for scales to 2^+-60, graded spectra, rotations up to pi - 0.1, unipotent
    and triangular matrices; within 0.03 rad of pi it grows like eps cond_log^2, and a strongly non-normal matrix
    (off-diagonals of 10..100 around a spectrum in [0.5, 2], rotated) may lose a few thousand eps m or come
    back NaN.  kappa_1(X) does not bound the error.
    """
    from ._autograd import LogmFn
    _, _, (mat,) = prepare(None, mat, grad_ok=True)
    D = _square(mat)
    if needs_grad(mat):
        if D > FRECHET_MAX:
            return _logm_torch(mat).contiguous()
        return LogmFn.apply(mat)
    return _logm(mat)


def meanm(mats, max_iter=1024, tol=1e-20):
    """Exponential barycentre of a set of matrices.  Replaces `lie.py:13-93` (same signature and iteration:
    float64 arithmetic, mean <- mean expm(mean_n logm(mean^-1 A_n)) until the sum of squares of the mean
    logarithm is <= tol).

    mats : `(N, M, M)` tensor or a list of `(M, M)` tensors; also `(..., N, M, M)` for many sets at once,
        each with its own stop test.
    Returns `(M, M)` (or `(..., M, M)`) in the input's dtype.  One `logm(mean^-1 A)` launch per iteration with
    the mean at stride 0 along the set.  A logarithm that comes back NaN (Q22) warns and stops that barycentre.
    """
    return _meanm(mats, max_iter, tol)[0]


def _meanm(mats, max_iter, tol):
    """meanm, returning (mean, number of iterations run)"""
    from .lie import _expm
    if not torch.is_tensor(mats):
        mats = torch.stack(list(mats))
    prepare(None, mats, grad_ok=True)
    D = _square(mats)
    if mats.dim() < 3:
        raise ValueError(f'expected (..., N, M, M) matrices, got {tuple(mats.shape)}')
    dtype = mats.dtype
    mats = mats.detach().double()
    batch = mats.shape[:-3]
    mean = torch.eye(D, dtype=torch.float64, device=mats.device).expand(tuple(batch) + (D, D)).contiguous()
    active = torch.ones(tuple(batch), dtype=torch.bool, device=mats.device)
    failed = False
    n_iter = 0
    for _ in range(int(max_iter)):
        n_iter += 1
        logs = _logm(mats, mean.unsqueeze(-3))
        mean_log = _tree_sum(logs.movedim(-3, -1)) / logs.shape[-3]
        sos = _tree_sum(mean_log.square().flatten(-2))
        nan = torch.isnan(sos)
        step = active & ~nan
        E = _expm(mean_log, 10000, 1e-32)
        new = mean[..., :, 0, None] * E[..., 0, None, :]
        for k in range(1, D):
            new = new + mean[..., :, k, None] * E[..., k, None, :]
        mean = torch.where(step[..., None, None], new, mean)
        active = step & ~(sos <= tol)
        # the one host read of the iteration: 0 = all done, 1 = go on, +2 = a logarithm failed
        code = int(active.any().to(torch.int32) + 2 * nan.any().to(torch.int32))
        failed = failed or code >= 2
        if not code & 1:
            break
    if failed:
        warnings.warn('`meanm` failed to converge (`logm` -> complex)', RuntimeWarning)
    return mean.to(dtype), n_iter
