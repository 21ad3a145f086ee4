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

Sums, extrema and indices have hard slices, an exact (fsum) truth and verdicts of their own in the last section of
this module (`make_hard_batches`, `SumPickTruth`); the sum bound is derived there.
"""
import math
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


def verdicts_each(got, ref, bound):
    """(error / bound of every slice with a finite truth, 0 elsewhere; mask of failing slices).  NaN must meet NaN,
    an infinity the same infinity, a finite truth a finite result within its bound (a zero bound: equality)."""
    with np.errstate(all='ignore'):
        isn, isi = np.isnan(ref), np.isinf(ref)
        fin = ~(isn | isi)
        err = np.abs(got - ref)
        ok = np.where(isn, np.isnan(got), np.where(isi, got == ref, np.isfinite(got) & (err <= bound)))
        r = np.where(fin & (err > 0), err / np.where(bound > 0, bound, np.finfo(LD).tiny), LD(0))
        return np.where(fin, r, 0).astype(np.float64), ~ok.astype(bool)


def verdicts(got, ref, bound):
    """(worst ratio over the finite slices, mask of failing slices) of `verdicts_each`"""
    r, bad = verdicts_each(got, ref, bound)
    return float(np.max(r, initial=0.0)), bad


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


def pick_arg(rows, which, omitnan):
    """position of the extremum of every row by the convention of `pick_truth`"""
    nan = np.isnan(rows)
    fill = -np.inf if which == 'max' else np.inf
    arg = (np.argmax if which == 'max' else np.argmin)(np.where(nan, fill, rows), 1)
    if not omitnan:
        arg = np.where(nan.any(1), nan.argmax(1), arg)
    return arg


def pick_truth(x, axis, which, g, omitnan):
    """gradient of sum(g * max/min(x, axis)): the whole cotangent at the FIRST occurrence of the extremum (numpy's
    argmax / argmin over the slice, reduced dims ascending in C order) -- after NaN -> -inf / +inf for the omitting
    forms, where an all-NaN slice gets no gradient at all; at the first NaN for the propagating forms."""
    x = np.asarray(x)
    rows, _ = to_slices(x, axis)
    nan = np.isnan(rows)
    arg = pick_arg(rows, which, omitnan)
    out = np.zeros(rows.shape, LD)
    out[np.arange(rows.shape[0]), arg] = np.asarray(g).reshape(-1).astype(LD)
    if omitnan:
        out[nan] = 0
    return from_slices(out, x.shape, axis), arg


# ------------------------------------------------------------------------------------------ sums and picks
# Hard slices for sum / nansum / max / min / nanmax / nanmin (+ indices), their truths and verdicts.
#
# Sum bound, per output slice.  n counted values, S = fsum of them (exact, as doubles), A = fsum of their absolute
# values, eps_out the machine epsilon of the OUTPUT dtype, u = 2^-53:
#
#     |s - S| <= eps_out |S| + n u A + (smallest subnormal of the output dtype)
#
# Derivation.  The contract is double accumulation and ONE rounding to the output dtype.  A double sum of n terms in
# any order -- lanes, chunks, the fold kernels, the float64 partial sums of the staged route -- is off by at most
# (n - 1) u A to first order (Higham, Accuracy and Stability, (4.4)): n u A.  The conversion of the double to the
# output dtype costs eps_out |S| while S is a normal number of that dtype and at most one smallest subnormal below
# that.  For float64 INPUT the n u A term is far above what a correct kernel does (errors of random sign grow like
# sqrt(n) u A, and `cancel` makes A / |S| only about n): there is no wider accumulator to compare a double sum with,
# so for float64 the sum verdict mostly guards the NaN / inf / overflow outcomes and gross errors, and the sharp
# check of the accumulation is float32 input, where a float32 accumulator misses the bound (test_reduce_ref_host).
# Where the truth is NaN or an infinity (IEEE: a counted +inf and -inf give NaN, one of them that infinity, a NaN
# without omitnan NaN) the result must be exactly that; where |S| is at least twice the output dtype's largest
# number (`overflow`) it must be that infinity, and no slice may have |S| between half and twice that number.
#
# Extrema: `==` with the truth (NaN meets NaN; the sign of a zero is not judged; a subnormal is not zero).  Indices:
# the first position by `pick_arg`, which is what the reference's `_reduce_index` gives (NaN -> -inf / +inf, then
# torch.max / torch.min over the flattened reduced dims); the element there, seen as the reduction sees it (NaN
# replaced for the omitting forms), equals the value unless that is NaN; and the value that comes with the indices
# (PickAcc) equals the one that comes without (ValAcc).
def hard_entries(dn):
    """(kind, variant) of the hard slices of a dtype, in the order they are planted"""
    e = [('graded', 0), ('cancel', 0), ('huge', 0)]
    if dn == 'f32':
        e.append(('overflow', 0))
    e += [('ints', 0), ('constant', 0), ('constant', 1)]
    e += [('tie_pair', k) for k in range(4)]
    e += [(k, 0) for k in ('late_nan', 'zeros', 'denormal', 'pinf', 'ninf', 'both_inf', 'all_ninf', 'nan_then_ninf',
                           'all_nan')]
    return tuple(e)


def hard_kinds(dn):
    return tuple(dict.fromkeys(k for k, _ in hard_entries(dn)))


def _border(rng, red):
    return min(int(rng.integers(8, 41)), max(red // 2, 1))


def _cancel_row(rng, red, a, odd):
    """a, -a shuffled (+ `odd` when red is odd), a_0 brought to element 0 and replaced by |a_0| 2^-20: the sum is
    -a_0 to a relative 2^-20, all other terms cancel in pairs"""
    parts = [a, -a] + ([np.array([odd], a.dtype)] if red % 2 else [])
    vals = np.concatenate(parts)
    order = rng.permutation(vals.size)
    r = vals[order]
    if a.size:
        j = int(np.flatnonzero(order == 0)[0])
        r[j] = r[0]
        r[0] = abs(a[0]) * a.dtype.type(2.0 ** -20)
    return r


def _cancel_half(rng, h, f):
    """the half `a` of a `cancel` slice: N(0, 1), with two of its elements -- never a_0, which becomes the sum --
    2^20 times larger.  Why the two large pairs: an accumulator of precision e that holds one of them absorbs
    the small terms it meets, an error of up to e 2^20 |a| / 2 per addition, whereas the n u A term of the sum
    bound only grows by their share of A = 0.8 |a| (n + 4 . 2^20).  With e = 2^-24 one such addition costs up to
    2^-5 |a|, against eps_out |S| + n u A <= 1.2e-7 |a_0| + 4.9e-4 |a| up to n = 2^20 + 77, and every order of
    summation makes dozens of them, so a float32 accumulator fails at every length; with e = 2^-53 they cost
    2^-34 |a| each and stay inside the bound, as any double sum does.  With N(0, 1) alone, A = 0.8 n |a| lets the
    bound grow like n^2 while the error of a float32 pairwise sum grows like sqrt(n log n): at n = 2^20 such a
    sum stayed at 0.19 of the bound and the slice could not tell it from a double one."""
    a = rng.standard_normal(h).astype(f)
    if h >= 3:
        a[1 + rng.choice(h - 1, 2, replace=False)] *= f(2.0 ** 20)
    return a


def _tie_positions(rng, red, variant, few):
    """(p1, p2) of the planted maximum and (q1, q2) of the planted minimum: four distinct positions"""
    if red < 4:
        raise ValueError('tie_pair needs four positions')
    cyc = ((0, red - 1), (red // 2, red // 2 + 1), (red - 2, red - 1), (red // 3, 2 * red // 3))
    if not few:
        p = rng.choice(red, 4, replace=False)
        return tuple(sorted(p[:2])), tuple(sorted(p[2:]))
    hi, lo = cyc[variant % 4], cyc[(variant + 1) % 4]
    if len(set(hi + lo)) < 4:                                   # a short slice: the minimum goes where there is room
        free = [j for j in range(red) if j not in hi]
        lo = tuple(sorted(rng.choice(free, 2, replace=False)))
    return hi, lo


def hard_rows(nout, red, dn, seed, entries=True, few=None):
    """(x, kinds): (nout, red) rows of N(0, 1) in the dtype with one hard slice per entry of `entries` (True: all of
    `hard_entries`) in the first rows, and the kind of every row ('normal' for the ordinary ones).  few: tie_pair
    cycles through fixed positions (default: the batch has no room for all entries at once)."""
    f = DT[dn]
    fi = np.finfo(f)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nout, red)).astype(f)
    which = hard_entries(dn) if entries is True else tuple(entries or ())
    if few is None:
        few = nout <= len(hard_entries(dn))
    kinds = ['normal'] * nout
    for row, (kind, variant) in enumerate(which):
        if row >= nout:
            break
        kinds[row] = kind
        r = x[row]
        if kind == 'graded':
            e = rng.integers(-60, 61, red) if dn == 'f32' else rng.integers(-500, 501, red)
            r[:] = np.ldexp(rng.standard_normal(red), e).astype(f)
        elif kind == 'cancel':
            a = _cancel_half(rng, red // 2, f)
            r[:] = _cancel_row(rng, red, a, f(1e-6 * rng.standard_normal())) * f(2.0 ** int(rng.integers(-20, 21)))
        elif kind == 'huge':
            lo = 2.0 ** 126 if dn == 'f32' else 2.0 ** 999 / red
            mag = np.minimum(rng.uniform(lo, 2 * lo, red // 2).astype(f), np.nextafter(f(2 * lo), f(0)))
            a = mag * rng.choice(np.array([-1, 1], f), red // 2)
            r[:] = _cancel_row(rng, red, a, f(1e-6 * lo * rng.standard_normal()))
            assert abs(math.fsum(r.astype(np.float64).tolist())) <= float(fi.max) / 2     # the true sum is small
        elif kind == 'overflow':
            assert dn == 'f32' and red >= 4
            r[:] = 0
            r[rng.choice(red, 4, replace=False)] = f(2.0 ** 127)
        elif kind == 'ints':
            r[:] = rng.integers(-3, 4, red).astype(f)
        elif kind == 'constant':
            r[:] = r[red // 2] if r[red // 2] != 0 else f(0.25)
            if variant:
                r[:_border(rng, red)] = np.nan
        elif kind == 'tie_pair':
            hi, lo = _tie_positions(rng, red, variant, few)
            top, bot = r.max() + f(1), r.min() - f(1)
            r[list(hi)] = top
            r[list(lo)] = bot
        elif kind == 'late_nan':
            r[red - 1 - int(rng.integers(0, max(red // 10, 1)))] = np.nan
        elif kind == 'zeros':
            r[0::2] = 0.0
            r[1::2] = -0.0
        elif kind == 'denormal':
            r[:] = rng.integers(-50, 51, red).astype(f) * fi.smallest_subnormal
        elif kind in ('pinf', 'ninf', 'both_inf'):
            p = rng.choice(red, 2, replace=False)
            if kind != 'ninf':
                r[p[0]] = np.inf
            if kind != 'pinf':
                r[p[1]] = -np.inf
        elif kind == 'all_ninf':
            r[:] = -np.inf
        elif kind == 'nan_then_ninf':
            r[:] = -np.inf
            r[:_border(rng, red)] = np.nan
        elif kind == 'all_nan':
            r[:] = np.nan
        else:
            raise ValueError(kind)
    # only `overflow` may come near the top of the format (`huge` was checked above: its sum needs fsum)
    rest = np.array([k not in ('huge', 'overflow') for k in kinds])
    with np.errstate(invalid='ignore'):
        mass = np.where(np.isfinite(x[rest]), np.abs(x[rest].astype(np.float64)), 0.0).sum(1)
    assert (mass <= float(fi.max) / 2).all()
    return x, kinds


def make_hard_batches(shape, axis, dn, seed):
    """[(array of `shape`, kinds of its slices over `axis`)]: together the arrays carry every entry of
    `hard_entries`, and every array an ordinary slice too.  A batch with fewer output slices than entries takes
    the entries in turn, all of its slices but one at a time -- and a batch of a single slice (the full reduction)
    one entry at a time, the ordinary slice in an array of its own."""
    ax = _axes(len(shape), axis)
    red = int(np.prod([shape[d] for d in ax], dtype=np.int64))
    nout = int(np.prod(shape, dtype=np.int64)) // red
    ents = hard_entries(dn)
    if nout > len(ents):
        plans, few = [ents], False
    else:
        per = max(nout - 1, 1)
        plans, few = [ents[i:i + per] for i in range(0, len(ents), per)] + ([()] if nout == 1 else []), True
    out = []
    for i, p in enumerate(plans):
        rows, kinds = hard_rows(nout, red, dn, seed + 101 * i, p, few)
        out.append((from_slices(rows, shape, axis), kinds))
    return out


def _same(a, b):
    """numerically equal, NaN meeting NaN"""
    with np.errstate(invalid='ignore'):
        return (a == b) | (np.isnan(a) & np.isnan(b))


class SumPickTruth:
    """per slice of x over axis: the exact sum S, the sum of absolute values A and the count n of the counted
    values, the IEEE outcome where a NaN or an infinity decides it, and the extrema with their first positions"""

    def __init__(self, x, axis):
        x = np.asarray(x)
        rows, kept = to_slices(x, axis)
        self.rows, self.kept, self.red = rows, kept, rows.shape[1]
        self.redshape = [x.shape[d] for d in _axes(x.ndim, axis)]
        r64 = rows.astype(np.float64)
        nan = np.isnan(r64)
        self.anynan = nan.any(1)
        pinf, ninf = (r64 == np.inf).any(1), (r64 == -np.inf).any(1)
        nout = rows.shape[0]
        self.S, self.A = np.zeros(nout, LD), np.zeros(nout, LD)
        for i in range(nout):
            if pinf[i] or ninf[i]:
                self.S[i] = np.nan if pinf[i] and ninf[i] else (np.inf if pinf[i] else -np.inf)
                self.A[i] = np.inf
            else:
                v = (r64[i][~nan[i]] if self.anynan[i] else r64[i]).tolist()
                self.S[i] = LD(math.fsum(v))
                self.A[i] = LD(math.fsum(map(abs, v)))
        self.n_omit = (~nan).sum(1)
        self._pick = {}

    # -------------------------------------------------------------------- sums
    def sum_expect(self, omitnan, out_dtype):
        """(ref, bound) per slice; ref non-finite where the result must be exactly that"""
        fi = np.finfo(out_dtype)
        top = LD(fi.max)
        S = self.S if omitnan else np.where(self.anynan, LD(np.nan), self.S)
        n = (self.n_omit if omitnan else np.full(self.n_omit.shape, self.red)).astype(LD)
        with np.errstate(all='ignore'):
            fin = np.isfinite(S)
            assert not (fin & (np.abs(S) > top / 2) & (np.abs(S) < 2 * top)).any(), 'a sum near the top of the format'
            ref = np.where(fin & (np.abs(S) >= 2 * top), np.sign(S) * LD(np.inf), S)
            bound = LD(fi.eps) * np.abs(S) + n * U * self.A + LD(fi.smallest_subnormal)
        return ref, bound

    def sum_each(self, got, omitnan, out_dtype, what=''):
        """(error / bound per slice, mask of failing slices)"""
        got = np.asarray(got)
        assert got.dtype == np.dtype(out_dtype), (what, got.dtype)
        assert list(got.shape) == list(self.kept), (what, got.shape, self.kept)
        ref, bound = self.sum_expect(omitnan, out_dtype)
        return verdicts_each(got.reshape(-1).astype(LD), ref, bound)

    def judge_sum(self, got, omitnan, out_dtype, what=''):
        """assert the verdict of EVERY slice; returns the worst error / bound ratio"""
        ratio, bad = self.sum_each(got, omitnan, out_dtype, what)
        if bad.any():
            ref, bound = self.sum_expect(omitnan, out_dtype)
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(f'{what} sum omitnan={omitnan} -> {np.dtype(out_dtype).name}: {int(bad.sum())} of '
                                 f'{bad.size} slices fail; first {i}: got {np.asarray(got).reshape(-1)[i]!r} ref '
                                 f'{ref[i]!r} bound {bound[i]!r} ratio {ratio[i]:.3g}')
        return float(ratio.max(initial=0.0))

    # -------------------------------------------------------------------- extrema
    def pick_expect(self, which, omitnan):
        """(value, first position, rows as the reduction sees them) per slice"""
        key = (which, omitnan)
        if key not in self._pick:
            seen = self.rows
            if omitnan:
                seen = np.where(np.isnan(seen), seen.dtype.type(-np.inf if which == 'max' else np.inf), seen)
            arg = pick_arg(self.rows, which, omitnan)
            self._pick[key] = (seen[np.arange(seen.shape[0]), arg], arg, seen)
        return self._pick[key]

    def value_bad(self, got, which, omitnan, what=''):
        got = np.asarray(got)
        assert got.dtype == self.rows.dtype, (what, got.dtype)
        assert list(got.shape) == list(self.kept), (what, got.shape, self.kept)
        return ~_same(got.reshape(-1), self.pick_expect(which, omitnan)[0])

    def flat_index(self, idx, what=''):
        """sub-indices (..., len(dims)) or positions (...) along a single dim -> positions in the slice"""
        idx = np.asarray(idx)
        if idx.ndim == len(self.kept) + 1:
            assert idx.shape[-1] == len(self.redshape), (what, idx.shape)
            sub = np.moveaxis(idx, -1, 0).reshape(len(self.redshape), -1)
            assert all(((s >= 0) & (s < m)).all() for s, m in zip(sub, self.redshape)), (what, 'sub-index out of range')
            idx = np.ravel_multi_index(tuple(sub), self.redshape)
        else:
            assert len(self.redshape) == 1, (what, idx.shape)
        idx = idx.reshape(-1)
        assert idx.shape[0] == self.rows.shape[0], (what, idx.shape)
        assert ((idx >= 0) & (idx < self.red)).all(), (what, 'index out of range')
        return idx

    def judge_value(self, got, which, omitnan, what=''):
        bad = self.value_bad(got, which, omitnan, what)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(f'{what} {which} omitnan={omitnan}: {int(bad.sum())} of {bad.size} values fail; first '
                                 f'{i}: got {np.asarray(got).reshape(-1)[i]!r} ref {self.pick_expect(which, omitnan)[0][i]!r}')
        return bad.size

    def pair_bad(self, got_val, got_idx, plain_val, which, omitnan, what=''):
        """mask of slices whose (value, index) pair fails: the value is wrong, the index is not the first position,
        the element there (as the reduction sees it) is not the value although that is no NaN, or the value
        differs from the one returned without indices"""
        ref, arg, seen = self.pick_expect(which, omitnan)
        idx = self.flat_index(got_idx, what)
        v = np.asarray(got_val).reshape(-1)
        bad = self.value_bad(got_val, which, omitnan, what) | (idx != arg)
        at = seen[np.arange(seen.shape[0]), idx]
        with np.errstate(invalid='ignore'):
            bad |= ~np.isnan(v) & ~(at == v)
        bad |= ~_same(v, np.asarray(plain_val).reshape(-1))
        return bad

    def judge_pair(self, got_val, got_idx, plain_val, which, omitnan, what=''):
        bad = self.pair_bad(got_val, got_idx, plain_val, which, omitnan, what)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            ref, arg, _ = self.pick_expect(which, omitnan)
            raise AssertionError(f'{what} {which} omitnan={omitnan} with indices: {int(bad.sum())} of {bad.size} slices '
                                 f'fail; first {i}: got {np.asarray(got_val).reshape(-1)[i]!r} at '
                                 f'{self.flat_index(got_idx)[i]} (without indices '
                                 f'{np.asarray(plain_val).reshape(-1)[i]!r}), ref {ref[i]!r} at {arg[i]}')
        return bad.size
