"""Shared by the generator (tests/golden/make_golden_special.py), the host test and the GPU test of the
`special` module: the case lists, the per-element bounds at C = 1 and the comparison helper.

tests/golden/special.npz holds, for inputs drawn once in float32 (the float64 cases use the same values):

group P (the reference is right)   besseli nu in {0, 1}, besseli_ratio, mvdigamma.  Truth T = the reference's
    float64 output: the same formulas, so what a kernel is measured against is rounding.
group A (the documented function)  besseli at the other orders.  T = mpmath.besseli at 40 digits.  The
    reference is right only for z > 2 nu and z >= 2 thr (special.py:337); `valid()` is that range, 2 % inside.
gradients on 64 points per case: the identities d log I = r + nu / z, r' = 1 - r^2 - (2 nu + 1) r / z,
    sum_p trigamma, evaluated in mpmath (r = I_{nu+1} / I_nu) and applied to T.

Bounds (eps of the dtype, times C):
    besseli None / 'norm' group P, besseli_ratio   eps |T|
    besseli 'log'                                  eps (1 + |T|)
    besseli None / 'norm' group A                  eps |T| (1 + |log I_nu(z)| + z)
    mvdigamma                                      eps sum_p (1 + |digamma(x_p)|)
    gradients                                      the same shapes on the derivative's terms before they are added
C = 2^ceil(log2(4 ref_ratio)) with ref_ratio the worst ratio of the REFERENCE's own result to these bounds (two
correct roundings of the same formula differ by the sum of their errors; then the next power of two): float32
on all of group P, float32 / float64 on the valid range of group A.  Group P in float64 takes the float32
figure: there the reference's float64 result IS the truth, and the same operations in the same order lose
the same number of ulps in either format.  Gradients use the C of their function.

Two allowances beyond the table above, both from the number formats and not from any result (counts over the 54
cases: profiles/special_accuracy.md): (1) `ratio` adds one subnormal step of the dtype to every bound: a
subnormal result (besseli None / 'norm' at small z and large nu) has no relative precision; (2) `grad_points` leaves
out the gradient points of besseli None / 'norm' whose forward truth is subnormal in the dtype: the backward pass
multiplies the SAVED output, which lost its relative precision before the pass starts.
"""
import os
import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'special.npz')
EPS = {'f32': 2.0 ** -23, 'f64': 2.0 ** -52}
NP = {'f32': np.float32, 'f64': np.float64}
MODES = (None, 'norm', 'log')
NU_P = (0.0, 1.0)
NU_A = (0.5, 2.0, 3.5, 7.0, 14.5, 15.0, 30.0, 100.0)
NU_R = (0.0, 0.5, 1.0, 2.5, 10.0)
NK = ((4, 10), (2, 3), (8, 20), (0, 0))
ORDERS = (1, 2, 3, 6)
SPECIAL = (0.0, 1e-30, 15.0 / 4.0, 1e4, float('inf'), float('nan'))
SPECIAL_DG = SPECIAL + (-1.0, -2.5, -1e-3, -1e-30)
FUNC = {'besseli': 0, 'besseli_bwd': 1, 'ratio': 2, 'ratio_bwd': 3, 'mvdigamma': 4, 'mvdigamma_bwd': 5}


def tag(v):
    return ('%g' % v).replace('.', 'p')


def valid(nu, z):
    """where the reference's besseli is right at an order other than 0 and 1, 2 % inside the edge"""
    ok = z > 2.04 * nu
    if nu < 15:
        thr = 5.0 * np.sqrt(15.0 - nu) * np.sqrt(nu + 15.0) / 3.0
        ok &= z >= 2.04 * thr
    return ok


def cases():
    """(kind, key, parameters): every forward case of the fixture; key names its arrays in the file"""
    out = []
    for nu in NU_P:
        for m in range(3):
            out.append(('besseliP', f'bi_{tag(nu)}_{m}', dict(nu=nu, mode=m)))
    for nu in NU_R:
        for N, K in NK:
            out.append(('ratio', f'br_{tag(nu)}_{N}_{K}', dict(nu=nu, N=N, K=K)))
    for order in ORDERS:
        out.append(('mvdigamma', f'dg_{order}', dict(order=order)))
    for nu in NU_A:
        for m in range(3):
            out.append(('besseliA', f'bi_{tag(nu)}_{m}', dict(nu=nu, mode=m)))
    return out


def group(kind):
    return 'A' if kind == 'besseliA' else 'P'


def input_key(kind, prm):
    return {'besseliP': 'zP', 'ratio': 'zP', 'besseliA': 'zA'}.get(kind) or f'x_{prm["order"]}'


class Fixture:
    def __init__(self, path=PATH):
        self.z = dict(np.load(path))

    def C(self, kind, dt):
        return float(self.z[f'C_{group(kind)}_{dt}'])

    def x(self, kind, prm):
        return self.z[input_key(kind, prm)]

    def bound(self, kind, key, prm, dt):
        """the C = 1 bound of a forward case, per element"""
        T = self.z['T_' + key]
        eps = EPS[dt]
        if kind == 'mvdigamma':
            return eps * self.z['B_' + key]
        if kind == 'ratio' or (kind == 'besseliP' and prm['mode'] != 2):
            return eps * np.abs(T)
        if prm['mode'] == 2:
            return eps * (1 + np.abs(T))
        logi = self.z['T_' + key[:-1] + '2']
        return eps * np.abs(T) * (1 + np.abs(logi) + self.z['zA'].astype(np.float64))

    def grad_bound(self, key, dt):
        return EPS[dt] * self.z['GB_' + key]

    def grad_points(self, kind, key, prm, dt):
        """(indices into the case's input, mask of the gradient points that are judged).  The derivative of
        besseli None / 'norm' is the saved output times a factor: where that output is subnormal in the dtype it has
        lost its relative precision before the backward pass starts, so those points are left out."""
        idx = self.z['gidx_' + input_key(kind, prm)]
        use = np.ones(len(idx), bool)
        if kind in ('besseliP', 'besseliA') and prm['mode'] != 2:
            use = np.abs(self.z['T_' + key][idx]) >= float(np.finfo(NP[dt]).tiny)
        return idx, use


def ratio(got, truth, bound, dt=None):
    """worst |got - truth| / bound over the elements where the truth is finite in the dtype; the others must
    match exactly (inf against inf, NaN against NaN).  With `dt`, a truth beyond the dtype's range counts as inf."""
    got = np.asarray(got, dtype=np.float64)
    truth = np.asarray(truth, dtype=np.float64)
    if dt is not None:
        truth = np.where(np.abs(truth) > float(np.finfo(NP[dt]).max), np.copysign(np.inf, truth), truth)
    fin = np.isfinite(truth)
    rest = ~fin
    if not np.array_equal(got[rest], truth[rest], equal_nan=True):
        return np.inf
    if not fin.any():
        return 0.0
    # a subnormal result has no relative precision: the bound never goes below one step of the format's grid
    step = float(np.finfo(NP[dt or 'f64']).smallest_subnormal)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        err = np.abs(got[fin] - truth[fin])
        r = np.where(err == 0, 0.0, err / (bound[fin] + step))
    return float(np.nanmax(np.where(np.isnan(r), np.inf, r)))


def same_pattern(got, want):
    """NaN / inf / zero pattern and signs of the non-finite values agree exactly"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
            and np.array_equal(got[np.isinf(want)], want[np.isinf(want)]) and np.array_equal(got == 0, want == 0))


def special_close(got, want, order, C, dt):
    """finite special-value entries of mvdigamma / its derivative: |got - want| <= C eps (order + |want|), which is
    at or below the fixture's bound eps sum_p (1 + |term_p|); the rest is judged by `same_pattern`"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    return bool((np.abs(got[fin] - want[fin]) <= C * EPS[dt] * (order + np.abs(want[fin]))).all())


def host_eval(lib, func, dt, x, mode_or_order=0, nu=0.0, N=0, K=0, saved=None, grad=None):
    """nfm_special_host_eval on numpy arrays: the kernels' arithmetic, compiled for the CPU"""
    x = np.ascontiguousarray(x, dtype=NP[dt])
    out = np.empty_like(x)
    keep = [np.ascontiguousarray(a, dtype=NP[dt]) if a is not None else None for a in (saved, grad)]
    rc = lib.nfm_special_host_eval(FUNC[func], 0 if dt == 'f32' else 1, mode_or_order, float(nu), N, K, x.size,
                                   x.ctypes.data, *(a.ctypes.data if a is not None else None for a in keep), out.ctypes.data)
    assert rc == 0, rc
    return out
