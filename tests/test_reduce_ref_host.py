"""The helpers of tests/_reduce_ref.py, and proof that their bars discriminate (second half: sums, extrema and
indices on hard slices).

The moment tests of test_gpu_reduce.py can see a wrong shift: on their own inputs, a numpy restatement of the
kernels' arithmetic (tests/_reduce_ref.py::restate, float64) passes the bounds with K = the first finite value an
accumulator folds, and fails them with K = 0 where the data sit far from 0.  Runs without a GPU.

Measured here (worst error / bound over all cases below): K = first value 0.50 with float32 results and 0.34 with
float64 results -- the final rounding to the output dtype itself, half an ulp against eps_out |ref|; the accumulation
terms stay below 0.3 of theirs.  K = 0 misses the bounds by a factor 1.0e+4 at float32 offset 1e6 and by more at
float64 offset 1e8 (variances off by O(1), a constant slice's exact 0 missed).
"""
import numpy as np
import pytest
import _reduce_ref as RR

pytestmark = pytest.mark.skipif(not RR.hp_ok(), reason='numpy.longdouble has no 64-bit mantissa here')

# (shape, axis) of test_gpu_reduce.py::MOMENT_ROUTES that differ as ROWS (the restatement knows no layouts):
# a short slice, one of several vectors per lane, a long one, a very long one, and the full reduction
HOST_SHAPES = (((1000, 8), 1), ((300, 100), 1), ((33, 2000), 1), ((3, 100_001), 1), ((1000,), None))
CASES = [(dn, off) for dn in ('f32', 'f64') for off in RR.OFFSETS[dn]]
STATS = (('mean', 0), ('var', 1), ('var', 0), ('std', 1), ('std', 0))


def _worst(dn, offset, shift, out_dtype, raise_on_fail):
    """worst ratio to the bound of the restatement over the shapes, NaN variants, batches and statistics;
    inf if some slice gets a failing verdict"""
    worst = 0.0
    for si, (shape, axis) in enumerate(HOST_SHAPES):
        for vi, variant in enumerate(RR.VARIANTS):
            for x in RR.make_batches(shape, axis, dn, offset, variant, 1000 * si + 10 * vi):
                tr = RR.Truth(x, axis)
                for kind, ddof in STATS:
                    got = RR.restate(tr.rows, kind, ddof, shift).astype(out_dtype).reshape(tr.kept)
                    if raise_on_fail:
                        worst = max(worst, tr.judge(got, kind, ddof, True, out_dtype, (shape, variant)))
                    else:
                        ref, bound = tr.expect(kind, ddof, True, out_dtype)
                        ratio, bad = RR.verdicts(got.reshape(-1).astype(RR.LD), ref, bound)
                        worst = max(worst, np.inf if bad.any() else ratio)
    return worst


@pytest.mark.parametrize('dn,offset', CASES)
def test_first_value_shift_meets_the_bounds(dn, offset):
    """every slice of every input, special slices included, in the input's dtype and in float64"""
    assert _worst(dn, offset, 'first', RR.DT[dn], True) <= 1.0
    if dn == 'f32':
        assert _worst(dn, offset, 'first', np.float64, True) <= 1.0


@pytest.mark.parametrize('dn,offset', [('f64', 1e8), ('f32', 1e6)])
def test_unshifted_formula_fails_the_bounds(dn, offset):
    assert not _worst(dn, offset, 'zero', RR.DT[dn], False) <= 1.0


@pytest.mark.parametrize('dn,offset', [('f64', 1e8), ('f32', 1e6)])
def test_shift_from_the_first_vector_only_fails_behind_nans(dn, offset):
    """the rule the kernels had: a lane whose first vector holds no finite value keeps K = 0 for the rest of its
    share.  Harmless without NaNs, wrong behind a NaN border and at a 5 % NaN rate (float64: 2-wide vectors)."""
    for variant, fails in (('clean', False), ('nan5', dn == 'f64'), ('border', True)):
        worst = 0.0
        for red in (100, 2000, 20_001):
            x = RR.make_rows(64, red, dn, offset, variant, red, specials=())       # ordinary slices only
            tr = RR.Truth(x, 1)
            got = RR.restate(tr.rows, 'var', 1, 'vector', vec=2 if dn == 'f64' else 4).astype(RR.DT[dn])
            ref, bound = tr.expect('var', 1, True, RR.DT[dn])
            ratio, bad = RR.verdicts(got.astype(RR.LD), ref, bound)
            worst = max(worst, np.inf if bad.any() else ratio)
        assert (worst > 1.0) == fails, (variant, worst)


def test_verdicts_cover_every_slice():
    """NaN meets NaN, inf the same inf, a zero bound means equality, and nothing is left out"""
    LD = RR.LD
    ref = np.array([np.nan, np.inf, -np.inf, 1.0, 0.0, 2.0], LD)
    bound = np.array([0, 0, 0, 0.5, 0.0, 0.5], LD)
    ok = np.array([np.nan, np.inf, -np.inf, 1.25, 0.0, 1.5], LD)
    ratio, bad = RR.verdicts(ok, ref, bound)
    assert not bad.any() and ratio == 1.0
    wrong = np.array([0.0, np.nan, np.inf, 1.75, 1e-300, np.nan], LD)
    _, bad = RR.verdicts(wrong, ref, bound)
    assert bad.all()
    # a constant slice behind a NaN border: R = 0, so the bound of var and std is exactly 0
    x = RR.make_rows(8, 100, 'f64', 1e8, 'border', 3)
    tr = RR.Truth(x, 1)
    for kind in ('var', 'std'):
        ref, bound = tr.expect(kind, 1)
        assert ref[3] == 0 and bound[3] == 0
    assert np.isnan(tr.expect('mean')[0][0]) and tr.n[1] == 1 and tr.n[2] == 2
    assert np.isnan(tr.expect('var', 1)[0][1]) and np.isfinite(tr.expect('var', 0)[0][1])
    assert np.isinf(tr.expect('mean')[0][4]) and np.isnan(tr.expect('var')[0][4])
    assert tr.R[5] > 900


# ---------------------------------------------------------------------------------------------------------------
# Sums, extrema and indices on the hard slices of _reduce_ref.make_hard_batches: the contract restated in numpy
# passes every verdict, and restatements that break it in one point fail where they should.
#
# (shape, axis) of every input of test_gpu_reduce.py::test_sums_and_picks_on_hard_slices (MOMENT_ROUTES, the
# staged and permuted-view dims, the full sizes and the two adjacent middle dims); as rows they give red =
# 4 .. 2^20 + 77 with many and with few output slices.
HARD_ROUTES = ([(s, 1) for s in ((1000, 8), (300, 100), (600, 4, 4), (4, 60, 4), (33, 2000), (3, 100_001), (5, 700, 2),
                                 (7, 300, 8), (3, 400, 5), (2, 300, 1000), (3, 50, 1001), (1, 3000, 260))] +
               [((3, 4, 9, 11, 5), (0, 2, 3, 4)), ((3, 4, 9, 11, 5), (1, 3)), ((2, 7, 9, 5, 6), -1),
                ((2, 7, 9, 5, 6), (1, 2)), ((9,), None), ((1000,), None), (((1 << 20) + 77,), None),
                ((5, 70, 6, 33), (1, 2))])
PICKS = [(w, o) for w in ('max', 'min') for o in (False, True)]


def _sum64(rows, omitnan, order, out_dtype):
    """the contract: double accumulation, pairwise or sequential, one rounding to the output dtype"""
    r = rows.astype(np.float64)
    if omitnan:
        r = np.where(np.isnan(r), 0.0, r)
    with np.errstate(all='ignore'):
        s = r.sum(1) if order == 'pairwise' else np.cumsum(r, axis=1)[:, -1]
        return s.astype(out_dtype)


def _sum32(rows, omitnan, order):
    """a float32 accumulator on float32 input"""
    assert rows.dtype == np.float32
    r = np.where(np.isnan(rows), np.float32(0), rows) if omitnan else rows
    with np.errstate(all='ignore'):
        return r.sum(1, dtype=np.float32) if order == 'pairwise' else np.cumsum(r, axis=1, dtype=np.float32)[:, -1]


def _pick(rows, which, omitnan, rule='first'):
    """(values, positions).  rule 'first': the contract; 'last': the last occurrence of the extremum;
    'skip': NaNs are passed over instead of being replaced by -inf / +inf (the omitting forms)"""
    nan = np.isnan(rows)
    fill = rows.dtype.type(-np.inf if which == 'max' else np.inf)
    seen = np.where(nan, fill, rows)
    red = rows.shape[1]
    arg_of = np.argmax if which == 'max' else np.argmin
    if rule == 'last':
        arg = red - 1 - arg_of(seen[:, ::-1], 1)
    else:
        arg = arg_of(seen, 1)
    if rule == 'skip' and omitnan:
        ext = seen[np.arange(len(seen)), arg]
        hit = ~nan & (seen == ext[:, None])
        arg = np.where(hit.any(1), hit.argmax(1), 0)
    if not omitnan:
        arg = np.where(nan.any(1), nan.argmax(1), arg)
        seen = rows
    return seen[np.arange(len(seen)), arg], arg


def _hard_inputs(dn, routes=HARD_ROUTES):
    for ri, (shape, axis) in enumerate(routes):
        for x, kinds in RR.make_hard_batches(shape, axis, dn, 1000 * ri + 7):
            yield shape, axis, x, np.array(kinds), RR.SumPickTruth(x, axis)


def _sub(tr, arg):
    """positions in the slice -> what the functions return: (..., len(dims)) sub-indices, or positions along one dim"""
    if len(tr.redshape) == 1:
        return arg.reshape(tr.kept)
    return np.stack(np.unravel_index(arg, tr.redshape), -1).reshape(tr.kept + [len(tr.redshape)])


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_double_accumulation_and_first_occurrence_pass_every_verdict(dn):
    """(a) every slice of every kind on every route shape, the sums pairwise and sequential, in the input dtype and
    in float64.  Worst error / bound measured here: 0.5 (the final rounding) for float32 input, 0.33 for float64."""
    worst, judged, met = 0.0, 0, set()
    for shape, axis, x, kinds, tr in _hard_inputs(dn):
        met.update((shape, str(axis), k) for k in kinds)
        for out_dtype in {RR.DT[dn], np.float64}:
            for omitnan in (False, True):
                for order in ('pairwise', 'sequential'):
                    got = _sum64(tr.rows, omitnan, order, out_dtype).reshape(tr.kept)
                    worst = max(worst, tr.judge_sum(got, omitnan, out_dtype, (shape, axis, order)))
        for which, omitnan in PICKS:
            val, arg = _pick(tr.rows, which, omitnan)
            judged += tr.judge_value(val.reshape(tr.kept), which, omitnan, (shape, axis))
            tr.judge_pair(val.reshape(tr.kept), _sub(tr, arg), val, which, omitnan, (shape, axis))
    print(f'HARD host {dn}: {judged} extremum verdicts, worst sum error / bound {worst:.3g}')
    assert worst <= 1.0 and judged > 40_000
    for shape, axis in HARD_ROUTES:
        assert {k for s, a, k in met if (s, a) == (shape, str(axis))} == set(RR.hard_kinds(dn)) | {'normal'}, (shape, axis)


@pytest.mark.parametrize('red', [100, 2000, 100_001, (1 << 20) + 77])
@pytest.mark.parametrize('order', ['pairwise', 'sequential'])
@pytest.mark.parametrize('kind', ['cancel', 'huge'])
def test_float32_accumulation_fails_the_sum_verdict(kind, red, order):
    """(b) on `cancel` and `huge` a float32 accumulator has to miss the bound at every length from 100 up (`huge`:
    a partial sum overflows; `cancel`: the rounding errors of partial sums of size sqrt(m) |a| against a sum of
    size |a|).  At red = 8 it may pass; nothing is asserted there.

    Measured error / bound: 1.6e3 .. 1.0e6 in the eight `cancel` cases (pairwise at 2^20 + 77: 1.6e3), inf / NaN
    results in all eight `huge` cases.  The two large pairs of `_reduce_ref._cancel_half` are what makes `cancel`
    tell at every length: with a half of plain N(0, 1) the float32 pairwise sum at 2^20 + 77 stayed at 0.19 of the
    bound, whose n u A term then grows like n^2 (the derivation is in that function's docstring)."""
    nout = 3 if red > 100_000 else 17
    shape, axis = ((red,), None) if red > (1 << 20) else ((nout, red), 1)
    seen = 0
    for x, kinds in RR.make_hard_batches(shape, axis, 'f32', red):
        sel = np.array(kinds) == kind
        if not sel.any():
            continue
        tr = RR.SumPickTruth(x, axis)
        for omitnan in (False, True):
            got = _sum32(tr.rows, omitnan, order).reshape(tr.kept)
            ratio, bad = tr.sum_each(got, omitnan, np.float32)
            seen += int(sel.sum())
            assert bad[sel].all(), (kind, omitnan, ratio[sel])
    assert seen == 2


@pytest.mark.parametrize('dn', ['f32', 'f64'])
def test_broken_conventions_fail_their_verdicts(dn):
    """(c) the last occurrence fails on `tie_pair` and `constant`, passing over NaNs instead of replacing them on
    `nan_then_ninf`, a sum that drops the infinities on `both_inf` -- on every slice of these kinds, on a route
    with many outputs, one with few and the full reduction"""
    routes = [HARD_ROUTES[1], HARD_ROUTES[5], HARD_ROUTES[17]]
    seen = set()
    for shape, axis, x, kinds, tr in _hard_inputs(dn, routes):
        for which, omitnan in PICKS:
            good = _pick(tr.rows, which, omitnan)[0]
            val, arg = _pick(tr.rows, which, omitnan, 'last')
            bad = tr.pair_bad(val.reshape(tr.kept), _sub(tr, arg), good, which, omitnan)
            ties = (kinds == 'tie_pair') | ((kinds == 'constant') & (omitnan | ~tr.anynan))
            assert bad[ties].all(), (shape, which, omitnan)
            if omitnan:
                val, arg = _pick(tr.rows, which, True, 'skip')
                bad = tr.pair_bad(val.reshape(tr.kept), _sub(tr, arg), good, which, True)
                sel = kinds == ('nan_then_ninf' if which == 'max' else 'none')
                assert bad[sel].all() and not bad[kinds == 'normal'].any(), (shape, which)
        for omitnan in (False, True):
            r = np.where(np.isinf(tr.rows), 0, tr.rows).astype(np.float64)
            got = (np.where(np.isnan(r), 0.0, r) if omitnan else r).sum(1).astype(RR.DT[dn]).reshape(tr.kept)
            _, bad = tr.sum_each(got, omitnan, RR.DT[dn])
            assert bad[kinds == 'both_inf'].all() and not bad[kinds == 'normal'].any(), (shape, omitnan)
        seen.update(kinds)
    assert {'tie_pair', 'constant', 'nan_then_ninf', 'both_inf'} <= seen


def test_sum_pick_truth_on_small_slices():
    """the truth itself, on rows small enough to check by hand"""
    inf, nan = np.inf, np.nan
    x = np.array([[1.0, 2.0, -4.0, 2.0], [nan, 3.0, 3.0, 1.0], [inf, 1.0, -inf, 0.0], [inf, nan, 1.0, inf],
                  [nan, nan, nan, nan], [-0.0, 0.0, -0.0, 0.0], [nan, nan, -inf, -inf]], np.float32)
    tr = RR.SumPickTruth(x, 1)
    ref, bound = tr.sum_expect(True, np.float32)
    assert ref[0] == 1 and ref[1] == 7 and np.isnan(ref[2]) and ref[3] == inf and ref[4] == 0 and ref[6] == -inf
    assert tr.A[0] == 9 and list(tr.n_omit) == [4, 3, 4, 3, 0, 4, 2]
    assert 0 < bound[0] <= 2.0 ** -23 + 4 * 2.0 ** -53 * 9 + 2e-45
    ref, _ = tr.sum_expect(False, np.float64)
    assert ref[0] == 1 and ref[5] == 0 and np.isnan(ref[[1, 2, 3, 4, 6]]).all()
    val, arg, _ = tr.pick_expect('max', True)
    assert list(arg) == [1, 1, 0, 0, 0, 0, 0] and list(val[:4]) == [2, 3, inf, inf] and val[4] == -inf and val[6] == -inf
    val, arg, _ = tr.pick_expect('max', False)
    assert list(arg) == [1, 0, 0, 1, 0, 0, 0] and np.isnan(val[[1, 3, 4, 6]]).all()
    val, arg, _ = tr.pick_expect('min', True)
    assert list(arg) == [2, 3, 2, 2, 0, 0, 2] and val[4] == inf and val[6] == -inf
    # a float32 sum of 4 x 2^127 is +inf, exactly 2^129 in float64
    big = np.zeros((1, 8), np.float32)
    big[0, ::2] = 2.0 ** 127
    tb = RR.SumPickTruth(big, 1)
    assert tb.sum_expect(True, np.float32)[0][0] == inf and tb.sum_expect(True, np.float64)[0][0] == 2.0 ** 129
    assert tb.sum_each(np.array([inf], np.float32), True, np.float32)[1].sum() == 0
    assert tb.sum_each(np.array([np.finfo(np.float32).max], np.float32), True, np.float32)[1].all()
    # the value with the index must be the element there, the first one, and the value without
    v, i = np.array([2, 3, inf, inf, -inf, 0, -inf], np.float32), np.array([1, 1, 0, 0, 0, 0, 0])
    assert not tr.pair_bad(v, i, v, 'max', True).any()
    assert list(tr.pair_bad(v, np.array([3, 2, 0, 3, 1, 1, 2]), v, 'max', True)) == [True, True, False, True, True, True, True]
    w = v.copy()
    w[5] = -0.0                                                 # the sign of a zero is not judged
    w[0] = 1.0
    assert list(tr.pair_bad(v, i, w, 'max', True)) == [True] + [False] * 6
    d = np.full((1, 5), np.finfo(np.float32).smallest_subnormal, np.float32)
    td = RR.SumPickTruth(d, 1)
    assert td.value_bad(np.zeros(1, np.float32), 'max', False).all() and not td.value_bad(d[:, 0], 'max', False).any()


def test_gradient_truth_matches_finite_differences():
    """the closed forms of `grad_truth` against central differences in longdouble"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 7, 2))
    x[0, 2, 1] = np.nan
    g = rng.standard_normal((3, 2))
    for fn, ddof in (('sum', 0), ('mean', 0), ('var', 1), ('var', 0), ('std', 1)):
        ref, _ = RR.grad_truth(x, 1, fn, g, ddof)

        def f(xx):
            tr = RR.Truth(xx, 1)
            if fn == 'sum':
                v = tr.mean * tr.n
            else:
                v = tr.expect(fn, ddof)[0]
            return (v * g.reshape(-1).astype(RR.LD)).sum()

        h = RR.LD(1e-6)
        for idx in ((0, 0, 0), (1, 3, 1), (2, 6, 0), (0, 5, 1)):
            xp, xm = x.astype(RR.LD), x.astype(RR.LD)
            xp[idx] += h
            xm[idx] -= h
            fd = (f(xp) - f(xm)) / (2 * h)
            assert abs(fd - ref[idx]) <= 1e-8 * (1 + abs(ref[idx])), (fn, idx)
        assert ref[0, 2, 1] == 0
