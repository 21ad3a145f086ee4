r'''
Stochastic estimators on MI355X -- drop-in for `nitorch_fastmath.stochastic` (`stochastic.py:1`):
`trapprox` (Hutchinson / Hutch++ trace and moment estimation), `maxeig_power` (power iteration) and
`vbald` (variational Bayesian approximation of log-determinants), same positional signatures.

The operator (`matvec`) belongs to the caller and runs as the caller wrote it.  What the reference does
around it is streaming work over whole fields, and that is HIP here (csrc/nfm_stochastic.hip):

- probes: one counter-based fill (Philox4x32-10) per stack of samples instead of three passes and a
  broadcast per probe (`stochastic.py:84-92`); element e of a call's probe stream depends on
  (seed, e) alone, sample i uses elements [i numel, (i + 1) numel);
- inner products: `gram` reads each vector once and sums in float64, whatever the working dtype
  (`flatten().dot()` accumulates in the working dtype, :141), straight into a float64 device tensor;
- Hutch++: the m^2 dots, m^2 host-indexed scalar writes and m^2 `addcmul_` passes of :105-123 are one
  `gram(m, m)` + one `combine(m, m)`; `torch.qr` of the n x m matrix (:127) is classical Gram-Schmidt
  applied twice on the same two kernels, with a drop rule for dependent columns;
- power iteration: a step is the operator, one `gram` into a device history and one `combine` that
  reads its scale from that history; the host looks at the history every `check_every` steps.

Nothing between the operator calls synchronises with the host.  Extensions (keyword-only):
`generator=` (the torch CPU generator the call's seed is drawn from; default: the global one, so
`torch.manual_seed` makes a call reproducible) and `check_every=` of `maxeig_power`.
'''
__all__ = ['trapprox', 'vbald', 'maxeig_power']
import ctypes
from math import ceil, log
import torch
from . import _lib
from ._dispatch import dtype_code, on_device, stream_ptr

_KINDS = {'r': _lib.STOCH_RADEMACHER, 'g': _lib.STOCH_GAUSSIAN}
_BLOCK = _lib.STOCH_MAX_VECS


# ---------------------------------------------------------------------------------------- kernels
def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _check_vecs(tensors, dtype, n):
    for t in tensors:
        if t.dtype != dtype or t.numel() != n or not t.is_contiguous():
            raise ValueError(f'expected contiguous {dtype} vectors of {n} elements, got {t.dtype} {tuple(t.shape)}')


def _run(dev, fn, *args):
    with on_device(dev):
        _lib.check(fn(*args, stream_ptr(dev)))


def _fill(out, kind, seed, offset=0):
    """out (contiguous, any shape) <- elements [offset, offset + out.numel()) of the probe stream of `seed`"""
    assert out.is_contiguous()
    _run(out.device, _lib.lib().nfm_stoch_fill, dtype_code(out.dtype), kind, seed, offset, out.numel(), out.data_ptr())
    return out


def _gram(xs, ys, out, accumulate=False):
    """out[j * len(ys) + k] (+)= <xs[j], ys[k]>; `out`: a contiguous float64 device tensor (or view) of p q elements"""
    p, q = len(xs), len(ys)
    dtype, n, dev = xs[0].dtype, xs[0].numel(), xs[0].device
    _check_vecs(list(xs) + list(ys), dtype, n)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == p * q
    L = _lib.lib()
    nbytes = L.nfm_stoch_gram_workspace_bytes(p, q)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    _run(dev, L.nfm_stoch_gram, dtype_code(dtype), p, q, n, _ptrs(xs), _ptrs(ys), ws.data_ptr(), nbytes,
         out.data_ptr(), int(bool(accumulate)))
    return out


def _combine(xs, c, ys, zs, scale_op=_lib.STOCH_SCALE_NONE, s_ref=None, s=None):
    """zs[k] = sigma (ys[k] - sum_j xs[j] c[j, k]); c, s_ref, s: float64 device tensors (views); zs[k] may be ys[k]"""
    p, q = len(xs), len(ys)
    dtype, n, dev = ys[0].dtype, ys[0].numel(), ys[0].device
    _check_vecs(list(xs) + list(ys) + list(zs), dtype, n)
    for t in (c, s_ref, s):
        assert t is None or (t.dtype == torch.float64 and t.is_contiguous())
    assert p == 0 or c.numel() == p * q
    _run(dev, _lib.lib().nfm_stoch_combine, dtype_code(dtype), p, q, n, _ptrs(xs) if p else None,
         c.data_ptr() if p else None, _ptrs(ys), _ptrs(zs), scale_op,
         None if s_ref is None else s_ref.data_ptr(), None if s is None else s.data_ptr())


def _blocks(m):
    return [range(a, min(a + _BLOCK, m)) for a in range(0, m, _BLOCK)]


def _orth(y):
    """Orthonormalise the rows of the stack `y` (m, ...) in place: classical Gram-Schmidt applied twice
    (Giraud, Langou, Rozloznik, van den Eshof 2005: orthogonal to a small multiple of eps whenever the
    columns are numerically independent).  A row that the projections reduce below 64 eps of its
    length -- a numerically dependent one -- is zeroed.  Returns the (m, 2) float64 device record
    [squared length before, squared length after the projections]."""
    m = y.shape[0]
    rows = [y[j] for j in range(m)]
    norms = torch.zeros(m, 2, dtype=torch.float64, device=y.device)
    c = torch.empty(_BLOCK, dtype=torch.float64, device=y.device)
    for j in range(m):
        _gram([rows[j]], [rows[j]], norms[j, 0:1])
        for _ in range(2 if j else 0):
            for blk in _blocks(j):          # more than 8 earlier rows: 8 at a time
                qs = [rows[i] for i in blk]
                _gram(qs, [rows[j]], c[:len(qs)])
                _combine(qs, c[:len(qs)], [rows[j]], [rows[j]])
        _gram([rows[j]], [rows[j]], norms[j, 1:2])
        _combine([], None, [rows[j]], [rows[j]], _lib.STOCH_SCALE_RSQRT_OR_DROP, norms[j, 0:1], norms[j, 1:2])
    return norms


def _deflate(q, g):
    """g -= q (q^T g) over stacks of m fields (rows of `q` orthonormal or zero): `outerpp` + `mmpp`"""
    m = q.shape[0]
    qr, gr = [q[j] for j in range(m)], [g[j] for j in range(m)]
    for gb in _blocks(m):
        gs = [gr[k] for k in gb]
        cs = []
        for qb in _blocks(m):       # every coefficient from the g that came in
            qs = [qr[j] for j in qb]
            cs.append(_gram(qs, gs, torch.empty(len(qs) * len(gs), dtype=torch.float64, device=q.device)))
        for qb, c in zip(_blocks(m), cs):
            _combine([qr[j] for j in qb], c, gs, gs)


# ---------------------------------------------------------------------------------------- plumbing
def _setup(matvec, shape, backend, fname):
    """(matvec, shape, dtype, device) with the reference's defaults (`stochastic.py:72-80`), GPU only"""
    backend = dict(backend)
    if torch.is_tensor(matvec):
        mat = matvec
        if mat.dim() != 2:
            # the reference's `shape = [*batch, N]` does not go through `mat.matmul` for batched input
            raise ValueError(f'{fname}: a tensor `matvec` is one 2-d matrix (dense or sparse), got {mat.dim()} dims')
        if not mat.is_cuda:
            raise RuntimeError(f'nitorch_fastmath_amd runs on MI355X (HIP) tensors only; got a matrix on {mat.device}. '
                               'There is no CPU fallback: move the data with .cuda().')

        def matvec(x):
            return mat.matmul(x)
        backend.setdefault('dtype', mat.dtype)
        backend.setdefault('device', mat.device)
        shape = [mat.shape[-1]]
    else:
        if not callable(matvec):
            raise TypeError(f'{fname}: `matvec` is a tensor or a callable')
        if shape is None:
            raise ValueError(f'{fname}: a callable `matvec` needs the vector `shape`')
        backend.setdefault('dtype', torch.get_default_dtype())
        if backend.get('device') is None:
            raise RuntimeError(f"{fname}: the reference builds its probes on the CPU unless told otherwise; "
                               "nitorch_fastmath_amd runs on MI355X (HIP) tensors only. There is no CPU fallback: "
                               "pass device='cuda'.")
    unknown = set(backend) - {'dtype', 'device'}
    if unknown:
        raise TypeError(f'{fname}: unexpected keyword arguments {sorted(unknown)}')
    dtype = backend['dtype']
    dtype_code(dtype)
    device = torch.device(backend['device'])
    if device.type != 'cuda':
        raise RuntimeError(f'nitorch_fastmath_amd runs on MI355X (HIP) tensors only; got device={device}. '
                           "There is no CPU fallback: pass device='cuda'.")
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    shape = [int(s) for s in (shape if isinstance(shape, (list, tuple, torch.Size)) else [shape])]
    return matvec, shape, dtype, device


def _seed(generator):
    """the call's 62-bit seed: one draw on the CPU (no device sync; `torch.manual_seed` reproduces it)"""
    return int(torch.randint(0, 2 ** 62, (1,), generator=generator))


def _kind(method):
    try:
        return _KINDS[method[0].lower()]
    except (KeyError, IndexError, TypeError):
        raise ValueError(f"method is 'rademacher' or 'gaussian', got {method!r}") from None


def _apply(matvec, x, dtype):
    """the caller's operator on one field; the result as a contiguous tensor of the working dtype"""
    y = matvec(x)
    if y.dtype != dtype or y.device != x.device or y.numel() != x.numel():
        raise ValueError(f'matvec returned {y.dtype} {tuple(y.shape)} on {y.device} for a {dtype} {tuple(x.shape)} '
                         f'field on {x.device}')
    return y.contiguous()


def _apply_stack(matvec, x, dtype):
    return torch.stack([_apply(matvec, x[j], dtype).reshape(x.shape[1:]) for j in range(x.shape[0])])


def _moments(matvec, shape, moments, samples, kind, hutchpp, dtype, device, seed):
    """the float64 device tensor (moments,) of trace estimates"""
    numel = 1
    for s in shape:
        numel *= s
    if hutchpp:
        m = int(ceil(samples / 3))
        # one fill for both stacks: q takes samples 0..m-1 of the call's stream, g takes m..2m-1
        probes = _fill(torch.empty([2 * m, *shape], dtype=dtype, device=device), kind, seed)
        q = _apply_stack(matvec, probes[:m], dtype)
        g = probes[m:]
        _orth(q)                      # q <- orth(A S), dependent columns zeroed
        _deflate(q, g)                # g <- (I - q q^T) g
        t2 = torch.zeros(moments, 2, dtype=torch.float64, device=device)
        mq, mg = q, g
        for j in range(moments):
            mq = _apply_stack(matvec, mq, dtype)
            mg = _apply_stack(matvec, mg, dtype)
            _gram([q], [mq], t2[j, 0:1])
            _gram([g], [mg], t2[j, 1:2])
        return t2[:, 0] + t2[:, 1] / m
    t = torch.zeros(moments, dtype=torch.float64, device=device)
    probes = _fill(torch.empty([samples, *shape], dtype=dtype, device=device), kind, seed)
    for i in range(samples):
        v = mv = probes[i]
        for j in range(moments):
            mv = _apply(matvec, mv, dtype)
            _gram([mv], [v], t[j:j + 1], accumulate=True)
    return t / samples


# ---------------------------------------------------------------------------------------- public
def trapprox(matvec, shape=None, moments=None, samples=10, method='rademacher', hutchpp=False, *,
             generator=None, **backend):
    r"""Stochastic trace approximation (Hutchinson's estimator), `stochastic.py:9-146`

    Parameters
    ----------
    matvec : `(N, N) tensor (dense or sparse) or callable(tensor) -> tensor`
        Function that computes the matrix-vector product
    shape : `sequence[int]`
        "vector" shape (callable `matvec` only)
    moments : `int`, default=1
        Number of moments: tr(A), tr(A^2), ...
    samples : `int`, default=10
        Number of samples
    method : `{'rademacher', 'gaussian'}`, default='rademacher'
        Sampling method
    hutchpp : `bool`, default=False
        Use Hutch++ (Meyer, Musco, Musco, Woodruff 2021) instead of Hutchinson (1989):
        ceil(samples / 3) deflation vectors + as many probes.  Uses more memory.
    generator : `torch.Generator` (CPU), keyword-only extension
        Where the call's seed is drawn from; default: torch's global CPU generator.
    dtype, device : backend; a callable `matvec` needs `device='cuda'` (there is no CPU path).

    Returns
    -------
    trace : `([moments],) tensor`

    Sums are accumulated in float64 on the device and nothing synchronises with the host: with a
    capturable `matvec` the whole call can be captured in a graph (a replay reuses the captured seed).
    """
    matvec, shape, dtype, device = _setup(matvec, shape, backend, 'trapprox')
    no_moments = moments is None
    moments = moments or 1
    samples = int(samples)
    if samples < 1:
        raise ValueError('samples must be at least 1')
    t = _moments(matvec, shape, moments, samples, _kind(method), hutchpp, dtype, device, _seed(generator)).to(dtype)
    return t[0] if no_moments else t


def maxeig_power(matvec, shape=None, max_iter=512, tol=1e-6, *, check_every=8, generator=None, **backend):
    """Estimate the maximum eigenvalue of a matrix by power iteration, `stochastic.py:316-362`

    Parameters
    ----------
    matvec : `(N, N) tensor (dense or sparse) or callable(tensor) -> tensor`
        Function that computes the matrix-vector product
    shape : `sequence[int]`
        "vector" shape (callable `matvec` only)
    max_iter : `int`, default=512
    tol : `float`, default=1e-6
    check_every : `int`, default=8, keyword-only extension
        The iteration keeps (<w, A w>, |A w|^2) of every step on the device and the host reads that history
        every `check_every` steps -- one sync instead of one per step.  The estimate returned is the one of
        the FIRST step that met `tol`, so it has the same bits for every `check_every` (1 = the reference's
        schedule); up to `check_every - 1` operator calls are spent past that step.
    generator : `torch.Generator` (CPU), keyword-only extension

    Returns
    -------
    maxeig : `scalar tensor`
        Largest eigenvalue
    """
    matvec, shape, dtype, device = _setup(matvec, shape, backend, 'maxeig_power')
    max_iter, check_every = int(max_iter), max(int(check_every), 1)
    if max_iter < 1:
        raise ValueError('max_iter must be at least 1')
    cur = _fill(torch.empty(shape, dtype=dtype, device=device), _lib.STOCH_RADEMACHER, _seed(generator))
    other = torch.empty_like(cur)
    hist = torch.zeros(max_iter, 2, dtype=torch.float64, device=device)
    mu0, scanned, found = float('inf'), 0, None
    for it in range(max_iter):
        w = cur
        v = _apply(matvec, w, dtype)
        _gram([w, v], [v], hist[it])                # (<w, v>, <v, v>)
        _combine([], None, [v], [other], _lib.STOCH_SCALE_RSQRT, None, hist[it, 1:2])
        cur, other = other, cur
        if (it + 1) % check_every == 0 or it + 1 == max_iter:
            mus = hist[scanned:it + 1, 0].tolist()      # the one sync of this stretch
            for k, mu in enumerate(mus):
                if abs(mu - mu0) < tol:
                    found = scanned + k
                    break
                mu0 = mu
            scanned = it + 1
            if found is not None:
                break
    return hist[max_iter - 1 if found is None else found, 0].to(dtype)


def vbald(matvec, shape=None, upper=None, moments=5, samples=5, mc_samples=64, method='rademacher', *,
          generator=None, **backend):
    """Variational Bayesian Approximation of Log Determinants (Granziol et al. 2018), `stochastic.py:149-228`

    Parameters
    ----------
    matvec : `(N, N) tensor (dense or sparse) or callable(tensor) -> tensor`
        Function that computes the matrix-vector product
    shape : `sequence[int]`
        "vector" shape (callable `matvec` only)
    upper : `float`
        Upper bound on eigenvalues (default: `maxeig_power`, with the caller's backend)
    moments : `int`, default=5
        Number of moments
    samples : `int`, default=5
        Number of samples for moment estimation
    mc_samples : `int`, default=64
        Number of samples for Monte Carlo integration
    method : `{'rademacher', 'gaussian'}`, default='rademacher'
        Sampling method
    generator : `torch.Generator` (CPU), keyword-only extension (seeds of the probes)

    Returns
    -------
    logdet : `scalar tensor`

    The moments are estimated on the device; the maximum-entropy fit (a 5 x 5 Newton system per
    iteration) runs on the host in float64, as the reference's does on its CPU tensors.
    """
    matvec, shape, dtype, device = _setup(matvec, shape, backend, 'vbald')
    numel = 1
    for s in shape:
        numel *= s
    if not upper:
        upper = maxeig_power(matvec, shape, generator=generator, dtype=dtype, device=device)
    upper = float(upper)

    def matvec2(x):
        return matvec(x).div(upper)
    mom = _moments(matvec2, shape, int(moments), int(samples), _kind(method), False, dtype, device, _seed(generator))
    mom = mom.cpu() / numel
    logdet = numel * (_vbald_fit(mom, int(mc_samples)) + log(upper))
    return logdet.to(dtype).to(device)


# --------------------------------------------------------- the reference's maximum-entropy fit (host)
def _vbald_fit(mom, mc_samples):
    """E[log(lam)] under the maximum-entropy density with moments `mom` (float64 CPU tensor), by the
    reference's algorithm (`stochastic.py:214-313`): Beta prior from the first two moments (Uniform when
    they give no valid one), Gauss-Newton with Armijo halving on Monte-Carlo integrals over `mc_samples`
    prior nodes, redrawn at every evaluation as the reference does; the node loops are vectorised."""
    mom = mom.detach().to('cpu', torch.float64)
    alpha = mom[0] * (mom[0] - mom[1]) / (mom[1] - mom[0] ** 2)
    beta = alpha * (1 / mom[0] - 1)
    if alpha > 0 and beta > 0:
        prior = torch.distributions.Beta(torch.tensor(alpha.item(), dtype=torch.float64),
                                         torch.tensor(beta.item(), dtype=torch.float64))
    else:
        prior = torch.distributions.Uniform(torch.tensor(1e-8, dtype=torch.float64),
                                            torch.tensor(1., dtype=torch.float64))
    coeff = _vbald_gn(mom, mc_samples, prior)
    lam = prior.sample([mc_samples])
    return (lam.log() * _vbald_factexp(lam, coeff)).mean()


def _vbald_factexp(lam, coeff):
    """exp(-1 - sum_i coeff[i] lam^(i+1)) at every node"""
    powers = lam[:, None] ** torch.arange(1, len(coeff) + 1, dtype=lam.dtype)
    return (-1 - powers @ coeff).exp()


def _vbald_mc(coeff, samples, prior, derivatives=False):
    """Monte-Carlo integrals of lam^j exp(-1 - sum coeff[i] lam^i), j = 0 (.. 2 len(coeff))"""
    lam = prior.sample([samples])
    q = _vbald_factexp(lam, coeff)
    if not derivatives:
        return q.mean()
    k = len(coeff)
    s = (q[:, None] * lam[:, None] ** torch.arange(0, 2 * k + 1, dtype=lam.dtype)).mean(0)
    idx = torch.arange(k)
    return s[0], s[1:k + 1], s[1 + idx[:, None] + idx[None, :]].clone()


def _vbald_gn(mom, samples, prior, tol=1e-6, max_iter=512):
    coeff = torch.zeros_like(mom)
    for _ in range(max_iter):
        loss, grad, hess = _vbald_mc(coeff, samples, prior, derivatives=True)
        loss = loss + coeff.dot(mom)
        grad = mom - grad
        diag = hess.diagonal(0, -1, -2)
        diag += 1e-3 * diag.abs().max() * torch.rand_like(diag)
        try:
            delta = torch.linalg.solve(hess, grad)
        except RuntimeError:        # a singular sample of the Hessian: keep what we have
            return coeff
        if not bool(torch.isfinite(delta).all()):
            return coeff
        success, armijo, loss0, coeff0 = False, 1., loss, coeff
        for _ in range(12):
            coeff = coeff0 - armijo * delta
            loss = _vbald_mc(coeff, samples, prior) + coeff.dot(mom)
            if loss < loss0:
                success = True
                break
            armijo /= 2
        if not success:
            return coeff0
        if abs(loss - loss0) < tol:
            break
    return coeff
