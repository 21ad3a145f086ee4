"""Exact model of `reduce.quantile`, written from its definition, for the quantile tests.

Per row: count = elements (omitnan: non-NaN elements); a NaN with omitnan=False, or count == 0 -> NaN;
p = fl64(q * (count - 1)), lo = floor(p), hi = ceil(p), w = p - lo; v_lo, v_hi = order statistics of the sorted
float64 copy; 'lower' v_lo, 'higher' v_hi, 'nearest' rank rint(p) half to even, 'midpoint' linear with w = 0.5,
'linear' v_lo when v_lo == v_hi, else v_lo + w (v_hi - v_lo) -- evaluated in fractions.Fraction, so exact.
An infinite v_lo or v_hi (unequal) has no exact value: the float64 formula of the definition is evaluated under
IEEE rules, which are exact on infinities (inf - inf = NaN).
"""
import math
from fractions import Fraction
import numpy as np

INTERPS = ('linear', 'lower', 'higher', 'nearest', 'midpoint')


def plan(q, count, interp):
    """(lo, hi, w) for count >= 1: the ranks selected and the weight of the upper one"""
    p = float(q) * float(count - 1)          # one double multiplication (count - 1 < 2^53 is exact)
    lo, hi = math.floor(p), math.ceil(p)
    w = p - float(lo)                        # exact
    if interp == 'lower':
        return lo, lo, 0.0
    if interp == 'higher':
        return hi, hi, 0.0
    if interp == 'nearest':
        r = round(p)                         # Python rounds a float half to even
        return r, r, 0.0
    if interp == 'midpoint':
        return lo, hi, 0.5
    assert interp == 'linear', interp
    return lo, hi, w


def combine(a, b, w):
    """exact value of the interpolation between the float64 numbers a <= b: a Fraction, or a float where the
    definition leaves no arithmetic (a == b) or IEEE rules apply (an infinity)"""
    a, b = float(a), float(b)
    if a == b:
        return a
    if not (math.isfinite(a) and math.isfinite(b)):
        with np.errstate(invalid='ignore'):
            a64, b64, w64 = np.float64(a), np.float64(b), np.float64(w)
            d = b64 - a64
            return float(a64 + w64 * d if w < 0.5 else b64 - d * (np.float64(1.0) - w64))
    return Fraction(a) + Fraction(w) * (Fraction(b) - Fraction(a))


def row_quantiles(row, qs, omitnan):
    """{interp: [(exact, v_lo, v_hi) per q]} of one 1-d array; exact is a Fraction or a float (NaN included)"""
    x = np.asarray(row, dtype=np.float64)
    nan = np.isnan(x)
    none = {m: [(float('nan'), float('nan'), float('nan'))] * len(qs) for m in INTERPS}
    if omitnan:
        x = x[~nan]
    elif nan.any():
        return none
    if x.size == 0:
        return none
    s = np.sort(x)
    out = {}
    for m in INTERPS:
        res = []
        for q in qs:
            lo, hi, w = plan(q, s.size, m)
            a, b = float(s[lo]), float(s[hi])
            res.append((combine(a, b, w), a, b))
        out[m] = res
    return out


def quantiles(x2d, qs, omitnan):
    """{interp: (exact[Q][rows], v_lo (Q, rows) float64, v_hi (Q, rows) float64)} of a (rows, red) array"""
    x2d = np.asarray(x2d)
    per_row = [row_quantiles(r, qs, omitnan) for r in x2d]
    out = {}
    for m in INTERPS:
        exact = [[per_row[r][m][k][0] for r in range(len(per_row))] for k in range(len(qs))]
        vlo = np.array([[per_row[r][m][k][1] for r in range(len(per_row))] for k in range(len(qs))], dtype=np.float64)
        vhi = np.array([[per_row[r][m][k][2] for r in range(len(per_row))] for k in range(len(qs))], dtype=np.float64)
        out[m] = (exact, vlo.reshape(len(qs), -1), vhi.reshape(len(qs), -1))
    return out


def as_dtype(exact, dtype):
    """exact[Q][rows] of an order-statistic mode (floats) as an array of `dtype`: those values are elements"""
    return np.array([[float(v) for v in r] for r in exact], dtype=np.float64).astype(dtype)


def worst_ratio(got, exact, vlo, vhi, eps):
    """max over the entries of |got - exact| / (eps * max(|v_lo|, |v_hi|)); asserts the NaN / infinity pattern:
    NaN exactly where the model is NaN, and a non-finite model value reproduced exactly"""
    got = np.asarray(got, dtype=np.float64)
    worst = 0.0
    for k, row in enumerate(exact):
        for r, e in enumerate(row):
            g = float(got[k, r])
            if isinstance(e, float) and not math.isfinite(e):
                assert (math.isnan(g) and math.isnan(e)) or g == e, (k, r, g, e)
                continue
            assert math.isfinite(g), (k, r, g, e)
            scale = max(abs(float(vlo[k, r])), abs(float(vhi[k, r])))
            err = abs(Fraction(g) - Fraction(e))
            if err == 0:
                continue
            assert scale > 0, (k, r, g, e)
            worst = max(worst, float(err / (Fraction(eps) * Fraction(scale))))
    return worst
