"""The moment tests of test_gpu_reduce.py can see a wrong shift: on their own inputs, a numpy restatement of the
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
