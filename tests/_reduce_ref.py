"""Inputs, high-precision truths and per-slice bounds of the moment and gradient tests of `reduce` (shared by
test_reduce_ref_host.py, test_gpu_reduce.py and test_gpu_autograd.py).

Truth: numpy on the input converted exactly to numpy.longdouble (64-bit mantissa, asserted by `hp_ok`), two passes
per output slice -- the mean, then the centred squares -- NaN omitted or propagated as asked.

Bounds, per output element.  n is the number of counted values of the slice, R = max - min of its finite values,
u = 2^-53 and eps_out the machine epsilon of the output dtype:

    variance   |v - v_ref| <= eps_out |v_ref| + 8 n u R^2 n / (n - ddof)
    std        |s - s_ref| <= eps_out |s_ref| + (8 n u R^2 n / (n - ddof)) / (2 s_ref)    (s_ref > 0; else exactly 0)
    mean       |m - m_ref| <= eps_out |m_ref| + 2 n u R

Derivation.  The kernels accumulate n, s = sum(x - K) and q = sum (x - K)^2 in double with a shift K that is one of
the slice's own values, so |x - K| <= R whatever value was picked.  A double sum of n terms, in any order, is off by
at most n u sum|terms|: n u . n R for s and n u . n R^2 for q.  Two partial sums with shifts K1, K2 are merged by
re-centring one on the other (s2 + n2 d, q2 + 2 d s2 + n2 d^2 with d = K2 - K1, |d| <= R): terms of the same form and
size.  The sum of squares about the mean, q - s^2 / n, inherits n u n R^2 from q and as much again from s^2 / n and
from the re-centring; 8 is twice the sum of these contributions, and the division by n - ddof scales all of it.  The
mean K + s / n carries n u n R / n = n u R from s, doubled for the re-centring.  d sqrt(v) = dv / (2 sqrt(v)) gives
the std.  eps_out |ref| is the final rounding to the output dtype (and the last operations in double).

Nothing in the bound depends on WHICH value of the slice the kernel takes as its shift; an unshifted formula
(K = 0 on data far from 0) is off by n u n offset^2 and misses it by orders of magnitude.  A constant slice has
R = 0: its variance and std must be exactly 0, its mean exact to eps_out.

Verdicts: every output slice gets one.  Where the truth is NaN or infinite (count <= ddof, an inf among the values,
a NaN without omitnan) the result must show exactly that; everywhere else it must be finite and within the bound.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
KINDS = ('mean', 'var', 'std')
# offsets of the data, per dtype: offset + N(0, 1) rounded to the dtype
OFFSETS = {'f32': (0.0, 3e4, 1e6), 'f64': (0.0, 1e8)}
VARIANTS = ('clean', 'nan5', 'border')
DT = {'f32': np.float32, 'f64': np.float64}
N_SPECIAL = 6


def hp_ok():
    return np.finfo(LD).eps <= 2.0 ** -63


# ------------------------------------------------------------------------------------------ slices
def _axes(ndim, axis):
    if axis is None:
        return tuple(range(ndim))
    ax = (axis,) if np.isscalar(axis) else tuple(axis)
    return tuple(sorted(a % ndim for a in ax))


def to_slices(x, axis):
    """(nout, red) view/copy of x: one row per output element, the reduced dims (ascending) in C order"""
    ax = _axes(x.ndim, axis)
    kept = [d for d in range(x.ndim) if d not in ax]
    xt = np.transpose(x, kept + list(ax))
    return xt.reshape(int(np.prod([x.shape[d] for d in kept], dtype=np.int64)), -1), [x.shape[d] for d in kept]


def from_slices(rows, shape, axis):
    """inverse of `to_slices`: the array of `shape` whose slices over `axis` are the rows"""
    ax = _axes(len(shape), axis)
    kept = [d for d in range(len(shape)) if d not in ax]
    order = kept + list(ax)
    xt = rows.reshape([shape[d] for d in order])
    return np.ascontiguousarray(np.transpose(xt, np.argsort(order)))


# ------------------------------------------------------------------------------------------ inputs
def make_rows(nout, red, dn, offset, variant, seed, specials=True):
    """(nout, red) rows of offset + N(0, 1) in the dtype, with the NaN variant applied and, if the batch has room,
    the six special slices in its first rows (a batch of fewer than seven rows carries as many as it has rows but
    one: `make_batches` spreads the rest over further batches).  `specials` may be a tuple of the ones to plant."""
    rng = np.random.default_rng(seed)
    x = (offset + rng.standard_normal((nout, red))).astype(DT[dn])
    if variant == 'nan5':
        x[rng.random((nout, red)) < 0.05] = np.nan
    elif variant == 'border':
        # the first 8..40 positions of EVERY slice (at most half of a short one)
        b = np.minimum(rng.integers(8, 41, size=nout), max(red // 2, 1))
        x[np.arange(red)[None, :] < b[:, None]] = np.nan
    elif variant != 'clean':
        raise ValueError(variant)
    which = tuple(range(N_SPECIAL)) if specials is True else tuple(specials or ())
    border = min(int(rng.integers(8, 41)), max(red // 2, 1))
    for row, sp in enumerate(which):
        if row >= nout:
            break
        r = x[row]
        if sp == 0:                                   # all NaN
            r[:] = np.nan
        elif sp == 1:                                 # a single counted value
            keep = r[red // 2] if np.isfinite(r[red // 2]) else DT[dn](offset + 0.25)
            r[:] = np.nan
            r[red // 2] = keep
        elif sp == 2 and red >= 2:                    # exactly two
            r[:] = np.nan
            r[red // 3] = DT[dn](offset + 0.75)
            r[red - 1] = DT[dn](offset - 1.25)
        elif sp == 3:                                 # constant behind a NaN border
            r[:] = DT[dn](offset + 0.5)
            r[:border] = np.nan
        elif sp == 4:                                 # holds an inf
            r[red // 2] = np.inf
        elif sp == 5:                                 # the first counted value is an outlier
            ok = np.flatnonzero(np.isfinite(r))
            if ok.size:
                r[ok[0]] = DT[dn](offset + 1e3)
    return x


def make_batches(shape, axis, dn, offset, variant, seed):
    """arrays of `shape` whose slices over `axis` come from `make_rows`; together they carry every special slice
    and at least one ordinary slice"""
    ax = _axes(len(shape), axis)
    red = int(np.prod([shape[d] for d in ax], dtype=np.int64))
    nout = int(np.prod(shape, dtype=np.int64)) // red
    if nout > N_SPECIAL:
        plans = [True]
    else:                                             # few outputs: the specials take turns, then a batch without
        sp = list(range(N_SPECIAL))
        plans = [tuple(sp[i:i + nout]) for i in range(0, N_SPECIAL, nout)] + [()]
    return [from_slices(make_rows(nout, red, dn, offset, variant, seed + 101 * i, p), shape, axis)
            for i, p in enumerate(plans)]


# ------------------------------------------------------------------------------------------ truth
class Truth:
    """two-pass longdouble moments of every slice of x over axis"""

    def __init__(self, x, axis):
        rows, kept = to_slices(np.asarray(x), axis)
        self.kept = kept
        self.red = rows.shape[1]
        xl = rows.astype(LD)
        nan = np.isnan(xl)
        fin = np.isfinite(xl)
        self.anynan = nan.any(1)
        self.n = (~nan).sum(1)
        with np.errstate(all='ignore'):
            nl = self.n.astype(LD)
            self.mean = np.where(nan, LD(0), xl).sum(1) / nl                     # 0 / 0 = NaN for an empty slice
            c = np.where(nan, LD(0), xl - self.mean[:, None])
            self.m2 = (c * c).sum(1)                                             # NaN when an inf is counted
            self.m2 = np.where(self.n == 0, LD(np.nan), self.m2)
            hi = np.where(fin, xl, -np.inf).max(1, initial=-np.inf)
            lo = np.where(fin, xl, np.inf).min(1, initial=np.inf)
            self.R = np.where(fin.any(1), hi - lo, LD(0))
        self.rows = rows

    def expect(self, kind, ddof=0, omitnan=True, out_dtype=np.float64):
        """(ref, bound) per slice; ref non-finite where the result must be exactly that"""
        eps = LD(np.finfo(out_dtype).eps)
        nl = self.n.astype(LD)
        with np.errstate(all='ignore'):
            if kind == 'mean':
                ref = self.mean.copy()
                bound = eps * np.abs(ref) + 2 * nl * U * self.R
            else:
                den = nl - ddof
                ref = np.where(den > 0, self.m2 / den, LD(np.nan))
                vterm = 8 * nl * U * self.R * self.R * nl / den
                if kind == 'var':
                    bound = eps * np.abs(ref) + vterm
                else:
                    ref = np.sqrt(ref)
                    bound = np.where(ref > 0, eps * ref + vterm / (2 * ref), LD(0))
            if not omitnan:
                ref = np.where(self.anynan, LD(np.nan), ref)
        return ref, bound

    def judge(self, got, kind, ddof=0, omitnan=True, out_dtype=np.float64, what='', strict=True):
        """assert the verdict of EVERY slice; returns the worst error / bound ratio of the finite ones
        (0 for an exact result against a zero bound).  strict=False (measuring scripts): a failing slice
        makes the ratio inf instead of raising."""
        ref, bound = self.expect(kind, ddof, omitnan, out_dtype)
        got = np.asarray(got)
        assert got.dtype == np.dtype(out_dtype), (what, got.dtype)
        assert list(got.shape) == list(self.kept), (what, got.shape, self.kept)
        ratio, bad = verdicts(got.reshape(-1).astype(LD), ref, bound)
        if not strict:
            return np.inf if bad.any() else ratio
        assert not bad.any(), (f'{what} {kind} ddof={ddof} omitnan={omitnan}: {int(bad.sum())} of {bad.size} slices fail; first '
                               f'{int(np.flatnonzero(bad)[0])}: got {got.reshape(-1)[bad][0]!r} ref {ref[bad][0]!r} '
                               f'bound {bound[bad][0]!r} n {self.n[bad][0]} R {self.R[bad][0]!r}; worst ratio {ratio:.3g}')
        return ratio


def verdicts(got, ref, bound):
    """(worst ratio over the finite slices, mask of failing slices).  NaN must meet NaN, an infinity the same
    infinity, a finite truth a finite result within its bound (a zero bound: equality)."""
    with np.errstate(all='ignore'):
        isn, isi = np.isnan(ref), np.isinf(ref)
        fin = ~(isn | isi)
        err = np.abs(got - ref)
        ok = np.where(isn, np.isnan(got), np.where(isi, got == ref, np.isfinite(got) & (err <= bound)))
        r = np.where(fin & (err > 0), err / np.where(bound > 0, bound, np.finfo(LD).tiny), LD(0))
    worst = float(np.max(np.where(fin, r, 0), initial=0.0))
    return worst, ~ok.astype(bool)


def judge_moments(tr, n, s, q, k, what='', strict=True):
    """raw moments [count, sum(x - K), sum (x - K)^2, K] of `reduce._moments`: the count is exact, K + s / n is held
    to the mean's bound and q - s^2 / n to n times the biased variance's"""
    n, s, q, k = (np.asarray(a).reshape(-1).astype(LD) for a in (n, s, q, k))
    assert np.array_equal(n, tr.n.astype(LD)), (what, 'counts')
    empty = tr.n == 0
    assert (s[empty] == 0).all() and (q[empty] == 0).all(), (what, 'empty slices')
    with np.errstate(all='ignore'):
        mean = k + s / n
        m2 = q - s * s / n
        ref_m, b_m = tr.expect('mean', 0, True, np.float64)
        ref_v, b_v = tr.expect('var', 0, True, np.float64)
        r1, bad1 = verdicts(mean, ref_m, b_m)
        r2, bad2 = verdicts(m2, ref_v * n, b_v * n)
    if not strict:
        return np.inf if (bad1.any() or bad2.any()) else max(r1, r2)
    assert not bad1.any(), (what, 'K + s/n', int(bad1.sum()), r1)
    assert not bad2.any(), (what, 'q - s^2/n', int(bad2.sum()), r2)
    return max(r1, r2)


# ------------------------------------------------------------------------------------------ host restatement
def restate(rows, kind, ddof, shift, lanes=8, vec=4):
    """The kernels' arithmetic in numpy float64, per row: `lanes` lanes take the vectors of `vec` elements in turn,
    each accumulates n, sum(x - K), sum (x - K)^2 with its own shift K, the lanes are merged pairwise by the
    re-centring formula of MomAcc::merge, and the statistic is finished as in MomAcc::finish.
    shift = 'first': K = the lane's first finite value (0 for a lane without one, which then counts nothing
    finite); shift = 'vector': K = the first finite value of the lane's FIRST VECTOR, else 0 (a lane whose first
    vector is all NaN folds the rest of its share unshifted); shift = 'zero': K = 0, the unshifted formula."""
    nout, red = rows.shape
    per = -(-red // (lanes * vec)) * vec                        # elements per lane, padded with NaN
    pad = np.full((nout, per * lanes), np.nan)
    pad[:, :red] = rows.astype(np.float64)
    # element e of the row sits in vector e // vec, which belongs to lane (e // vec) % lanes
    x = pad.reshape(nout, per // vec, lanes, vec).transpose(0, 2, 1, 3).reshape(nout, lanes, per)
    cnt = ~np.isnan(x)
    if shift == 'first':
        fin = np.isfinite(x)
        first = np.where(fin.any(2), fin.argmax(2), 0)
        k = np.where(fin.any(2), np.take_along_axis(x, first[..., None], 2)[..., 0], 0.0)
    elif shift == 'vector':
        fin = np.isfinite(x[..., :vec])
        first = np.where(fin.any(2), fin.argmax(2), 0)
        k = np.where(fin.any(2), np.take_along_axis(x, first[..., None], 2)[..., 0], 0.0)
    elif shift == 'zero':
        k = np.zeros((nout, lanes))
    else:
        raise ValueError(shift)
    with np.errstate(all='ignore'):
        d = np.where(cnt, x - k[..., None], 0.0)
        n, s, q = cnt.sum(2).astype(np.float64), d.sum(2), (d * d).sum(2)
        w = lanes
        while w > 1:                                            # xor-shuffle tree
            h = w // 2
            n1, s1, q1, k1 = n[:, :h], s[:, :h], q[:, :h], k[:, :h]
            n2, s2, q2, k2 = n[:, h:w], s[:, h:w], q[:, h:w], k[:, h:w]
            kk = np.where(n1 == 0, k2, k1)
            dk = k2 - kk
            s = s1 + s2 + n2 * dk
            q = q1 + q2 + (2.0 * dk) * s2 + n2 * dk * dk
            n, k, w = n1 + n2, kk, h
        n, s, q, k = n[:, 0], s[:, 0], q[:, 0], k[:, 0]
        if kind == 'mean':
            return k + s / n
        ss = q - s * (s / n)
        den = n - ddof
        v = np.where(ss < 0, 0.0, ss) / den
        v = np.where(den <= 0, np.nan, v)
        return np.sqrt(v) if kind == 'std' else v


# ------------------------------------------------------------------------------------------ gradients
def grad_truth(x, axis, fn, g, ddof=0, omitnan=True, tr=None):
    """closed-form gradient of sum(g * fn(x, axis)) in longdouble, and its bound, both shaped like x.
    g: cotangent with one entry per output slice (C order of the kept dims).

        sum    g on the counted elements, 0 at omitted NaNs
        mean   g / n
        var    2 (x - mean) g / (n - ddof)
        std    var's gradient / (2 std)

    Bound: eps |ref| (eps of the leaf's dtype: the gradient is rounded to it) plus the error of the forward
    quantities the backward pass reads, propagated to first order with the bounds of this module:
        var    2 |g| / (n - ddof) . b_mean
        std    that / (2 std) + |ref| b_std / std
    A propagating var / std with a NaN in the slice has a NaN gradient on the whole slice; the propagating sum and
    mean have the gradient g (g over the slice's length) whatever the values."""
    x = np.asarray(x)
    tr = tr or Truth(x, axis)                         # (a caller with several functions of one input shares it)
    rows = tr.rows.astype(LD)
    nan = np.isnan(rows)
    g = np.asarray(g).reshape(-1).astype(LD)[:, None]
    nl = tr.n.astype(LD)[:, None]
    eps = LD(np.finfo(x.dtype).eps)
    with np.errstate(all='ignore'):
        if fn == 'sum':
            ref = np.broadcast_to(g, rows.shape).copy()
            extra = np.zeros_like(ref)
        elif fn == 'mean':
            ref = np.broadcast_to(g / nl, rows.shape).copy()
            extra = np.zeros_like(ref)
        else:
            _, b_mean = tr.expect('mean', 0, True, np.float64)
            den = nl - ddof
            ref = 2 * (rows - tr.mean[:, None]) * g / den
            extra = 2 * np.abs(g) / np.abs(den) * b_mean[:, None]
            if fn == 'std':
                sd, b_sd = tr.expect('std', ddof, True, np.float64)
                sd, b_sd = sd[:, None], b_sd[:, None]
                ref = ref / (2 * sd)
                extra = extra / (2 * sd) + np.abs(ref) * b_sd / sd
        if omitnan:
            ref = np.where(nan, LD(0), ref)
            extra = np.where(nan, LD(0), extra)
        elif fn in ('sum', 'mean'):                   # does not depend on x: g, or g over the slice's length
            ref = np.broadcast_to(g / (tr.red if fn == 'mean' else 1), rows.shape).copy()
        else:
            ref = np.where(tr.anynan[:, None], LD(np.nan), ref)
        bound = eps * np.abs(ref) + extra
    return (from_slices(ref, x.shape, axis), from_slices(bound, x.shape, axis))


def judge_grad(got, ref, bound, what=''):
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio, bad = verdicts(got.reshape(-1).astype(LD), ref.reshape(-1), bound.reshape(-1))
    assert not bad.any(), (f'{what}: {int(bad.sum())} of {bad.size} gradient entries fail; first got '
                           f'{got.reshape(-1)[bad][0]!r} ref {ref.reshape(-1)[bad][0]!r} bound {bound.reshape(-1)[bad][0]!r}; '
                           f'worst ratio {ratio:.3g}')
    return ratio


def pick_truth(x, axis, which, g, omitnan):
    """gradient of sum(g * max/min(x, axis)): the whole cotangent at the FIRST occurrence of the extremum (numpy's
    argmax / argmin over the slice, reduced dims ascending in C order) -- after NaN -> -inf / +inf for the omitting
    forms, where an all-NaN slice gets no gradient at all; at the first NaN for the propagating forms."""
    x = np.asarray(x)
    rows, _ = to_slices(x, axis)
    nan = np.isnan(rows)
    fill = -np.inf if which == 'max' else np.inf
    arg = (np.argmax if which == 'max' else np.argmin)(np.where(nan, fill, rows), 1)
    if not omitnan:
        arg = np.where(nan.any(1), nan.argmax(1), arg)
    out = np.zeros(rows.shape, LD)
    out[np.arange(rows.shape[0]), arg] = np.asarray(g).reshape(-1).astype(LD)
    if omitnan:
        out[nan] = 0
    return from_slices(out, x.shape, axis), arg
