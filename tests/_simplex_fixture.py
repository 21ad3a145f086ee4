"""Reader of tests/golden/simplex.npz and the accuracy bounds of the simplex tests (shared by
test_simplex_host.py, test_gpu_simplex.py and tests/golden/make_golden_simplex.py).

The fixture stores, per shape (K, inner) and input dtype, what the reference returned.  Outputs that the
reference itself derives from another one by moving or dropping a column (softmax with the added class first
instead of last, a dropped class) are stored once: the generator checks, bit for bit, that
`derive(base, ...)` reproduces the reference's own output before it leaves one out.  The file is packed
(`pack` / `Store`): arrays lie end to end in a few pools, and an array that another one predicts (the float32
output from the rounded float64 one, log_softmax from x - logsumexp, logit's inputs from the softmax truth) is
stored as the integer difference of the two bit patterns -- exact for every value, NaN included, and nearly
all zeros.

Bounds (C = 1), per element, against the float64 truth T; m is the voxel's max (clamped at 0 for an implicit
input), K' the number of classes the arithmetic sees, eps the input dtype's:
  softmax      eps (K' + max_k |x_k - m|) T + tiny, tiny = the smallest normal number.  The class ADDED to an
               implicit input is formed by the reference as 1 - sum(p), so its float64 output carries an absolute
               error of eps64 K' there and its float32 output one of eps32 K'.  The kernels are judged against
               exp(-logsumexp), from the reference's float64 logsumexp, which has no cancellation
               (`truth(..., exact_added=True)`), under the plain bound; only where the REFERENCE's float32 output
               is judged (the fixture's self-consistency, C) does that class get an absolute eps K'
               (`bound(..., slack=True)`)
  logsumexp    eps (K' + |m|)
  log_softmax  eps (K' + |m| + |x_k|)
  logit        eps (K' + |log p_k| + |log p_ref| + [implicit input] K' / max(1 - sum p, 1e-8))
"""
import json
import os
import re
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'golden', 'simplex.npz')
KS = (1, 2, 3, 5, 8, 16, 17, 40)
INNERS = (1, 7, 64)
DTYPES = ('f32', 'f64')
IMPLICIT = ((False, False), (False, True), (True, False), (True, True))
INDICES = (0, -1)
FUNCS = ('softmax', 'log_softmax', 'logit', 'logsumexp')
EPS = {'f32': 2.0 ** -23, 'f64': 2.0 ** -52}
TINY = {'f32': float(np.finfo(np.float32).tiny), 'f64': float(np.finfo(np.float64).tiny)}


def shape_of(K, inner):
    """(outer, K, inner): 64 voxels for inner = 64, 7 for 7, 6 for the class-last layout"""
    return (6, K, 1) if inner == 1 else (1, K, inner)


def kprime(K, imp):
    return K + (1 if imp[0] else 0)


def norm_index(idx, kp):
    return idx % kp


def base_key(fn, imp, idx):
    """which stored array an (fn, implicit, implicit_index) output derives from: (key, how)"""
    if fn == 'logsumexp':
        return ('i' if imp[0] else 'e'), 'same'
    if fn in ('softmax', 'log_softmax'):
        if imp[0]:
            return 'i', ('same' if imp[1] else 'move')      # base: K + 1 classes, the hidden one LAST
        return 'e', ('drop' if imp[1] else 'same')
    if imp[0]:                                               # logit, hidden reference class
        return 'i', ('same' if imp[1] else 'insert0')       # base: K logits
    return ('e0' if idx == 0 else 'e1'), ('drop' if imp[1] else 'same')


def derive(base, how, idx, axis=1):
    """the reference's output from the stored base (idx normalised to the K'-long axis)"""
    if how == 'same':
        return base
    if how == 'drop':
        return np.delete(base, idx, axis)
    if how == 'move':        # hidden class stored last -> at idx; with 'same' for (True, True): drop it
        body, bg = np.delete(base, -1, axis), np.take(base, [-1], axis)
        return np.concatenate([np.take(body, range(idx), axis), bg,
                               np.take(body, range(idx, body.shape[axis]), axis)], axis)
    if how == 'insert0':
        z = np.zeros_like(np.take(base, [0], axis))
        return np.concatenate([np.take(base, range(idx), axis), z,
                               np.take(base, range(idx, base.shape[axis]), axis)], axis)
    raise ValueError(how)


def _bits(a):
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def predict(name, get):
    """the array that predicts `name` from others of the fixture, or None"""
    m = re.match(r'ref_(.+)_f32$', name)
    if m:
        return get('true_' + m.group(1)).astype(np.float32)
    m = re.match(r'true_log_softmax_([ei])_(\d+)_(\d+)$', name)
    if m:
        key, K, inner = m.groups()
        x = get(f'x_{K}_{inner}').astype(np.float64)
        if key == 'i':
            x = np.concatenate([x, np.zeros_like(x[:, :1])], 1)
        return x - get(f'true_logsumexp_{key}_{K}_{inner}')
    m = re.match(r'p_([ei])_(\d+)_(\d+)$', name)
    if m:
        key, K, inner = m.groups()
        t = get(f'true_softmax_{key}_{K}_{inner}')
        return (t if key == 'e' else t[:, :-1]).astype(np.float32)
    m = re.match(r'special_(.+)_f32$', name)
    if m:
        return get(f'special_{m.group(1)}_f64').astype(np.float32)
    return None


_POOLS = {'T': np.float64, 'X': np.float32, 'D8': np.int8, 'D16': np.int16, 'D32': np.int32, 'D64': np.int64}


def pack(path, arrays):
    """write the logical arrays {name: array} as a few pools + an index"""
    pools = {k: [] for k in _POOLS}
    fill = {k: 0 for k in _POOLS}
    index = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        pred = predict(name, arrays.__getitem__)
        if pred is not None and pred.shape == a.shape and pred.dtype == a.dtype:
            with np.errstate(over='ignore'):
                d = (_bits(a) - _bits(pred)).reshape(-1)
            if not d.any():
                index[name] = ['same', '', 0, list(a.shape)]
                continue
            pool = next(k for k in ('D8', 'D16', 'D32', 'D64')
                        if d.size == 0 or (d.min() >= np.iinfo(_POOLS[k]).min and d.max() <= np.iinfo(_POOLS[k]).max))
            index[name] = ['delta', pool, fill[pool], list(a.shape)]
            pools[pool].append(d.astype(_POOLS[pool]))
            fill[pool] += d.size
            continue
        pool = 'X' if a.dtype == np.float32 else 'T'
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        index[name] = ['raw', pool, fill[pool], list(a.shape)]
        pools[pool].append(a.reshape(-1))
        fill[pool] += a.size
    out = {k: (np.concatenate(v) if v else np.zeros(0, _POOLS[k])) for k, v in pools.items()}
    out['index'] = np.frombuffer(json.dumps(index, separators=(',', ':')).encode(), dtype=np.uint8)
    np.savez_compressed(path, **out)


class Store:
    """read side of `pack`: store[name] is the array the generator put in, bit for bit"""

    def __init__(self, path):
        z = np.load(path)
        self.pools = {k: z[k] for k in _POOLS}
        self.index = json.loads(bytes(z['index']).decode())
        self.cache = {}

    def __contains__(self, name):
        return name in self.index

    def __getitem__(self, name):
        if name not in self.cache:
            kind, pool, off, shape = self.index[name]
            n = int(np.prod(shape, dtype=np.int64))
            if kind == 'raw':
                a = self.pools[pool][off:off + n].reshape(shape)
            else:
                pred = predict(name, self.__getitem__)
                a = pred
                if kind == 'delta':
                    bits = _bits(np.ascontiguousarray(pred)).reshape(-1)
                    with np.errstate(over='ignore'):
                        a = (bits + self.pools[pool][off:off + n].astype(bits.dtype)).view(pred.dtype).reshape(shape)
            self.cache[name] = a
        return self.cache[name]


class Fixture:
    def __init__(self, path=PATH):
        self.z = Store(path)
        self.C = float(self.z['C'])
        self.ref_ratio = float(self.z['ref_ratio'])

    def x(self, fn, K, inner, dt, imp):
        """the input of a case: logits, or for logit the probabilities (with or without the hidden class)"""
        if fn == 'logit':
            a = self.z[f'p_{"i" if imp[0] else "e"}_{K}_{inner}']
        else:
            a = self.z[f'x_{K}_{inner}']
        return a.astype(np.float32 if dt == 'f32' else np.float64)

    def _out(self, kind, fn, K, inner, dt, imp, idx):
        kp = kprime(K, imp)
        key, how = base_key(fn, imp, norm_index(idx, kp))
        base = self.z[f'{kind}_{fn}_{key}_{K}_{inner}' + ('' if kind == 'true' else f'_{dt}')]
        if fn in ('softmax', 'log_softmax') and imp[0] and imp[1]:
            return np.delete(base, -1, 1)
        return derive(base, how, norm_index(idx, kp))

    def ref(self, fn, K, inner, dt, imp, idx):
        """the reference's output in the input dtype"""
        if dt == 'f64':
            return self.truth(fn, K, inner, imp, idx, exact_added=False)
        return self._out('ref', fn, K, inner, dt, imp, idx)

    def truth(self, fn, K, inner, imp, idx, exact_added=True):
        """the reference's float64 output on the float32-rounded inputs (which ARE the float64 cases' inputs).
        exact_added: the class softmax adds to an implicit input is exp(-logsumexp) from the reference's float64
        logsumexp instead of the reference's 1 - sum(p) (module docstring)"""
        t = self._out('true', fn, K, inner, 'f64', imp, idx)
        if exact_added and fn == 'softmax' and imp[0] and not imp[1]:
            t = t.copy()
            t[:, norm_index(idx, K + 1)] = np.exp(-self.z[f'true_logsumexp_i_{K}_{inner}'][:, 0])
        return t


def bound(fn, x, truth, imp, idx, dt, slack=False):
    """the C = 1 bound, shaped like `truth` (x: the case's input as float64).  slack: the absolute eps K' of the
    class the REFERENCE adds as 1 - sum(p); never for the kernels (module docstring)"""
    eps, tiny = EPS[dt], TINY[dt]
    x = x.astype(np.float64)
    K = x.shape[1]
    kp = kprime(K, imp)
    idx = norm_index(idx, kp)
    if fn == 'logit':
        with np.errstate(all='ignore'):
            if imp[0]:
                rest = np.maximum(1 - x.sum(1, keepdims=True), 1e-8)
                lp = derive(np.abs(np.log(x)), 'insert0', idx)
                b = kp + lp + np.abs(np.log(rest)) + kp / rest
            else:
                b = kp + np.abs(np.log(x)) + np.abs(np.log(x[:, idx:idx + 1]))
        if imp[1]:
            b = np.delete(b, idx, 1)
        return eps * b
    z = derive(x, 'insert0', idx) if imp[0] else x
    m = z.max(1, keepdims=True)
    if fn == 'logsumexp':
        return eps * (kp + np.abs(m))
    if fn == 'log_softmax':
        b = eps * (kp + np.abs(m) + np.abs(z))
    else:
        with np.errstate(all='ignore'):
            spread = np.abs(z - m).max(1, keepdims=True)
        b = np.broadcast_to(eps * (kp + spread), z.shape).copy()
        if imp[1]:
            b = np.delete(b, idx, 1)
        b = b * np.abs(truth) + tiny
        if slack and imp[0] and not imp[1]:
            b[:, idx] += eps * kp
        return b
    if imp[1]:
        b = np.delete(b, idx, 1)
    return b


def ratio(got, truth, bnd):
    """worst |got - truth| / bound over the finite entries of the truth (NaN / inf are checked as a pattern)"""
    ok = np.isfinite(truth) & np.isfinite(bnd)
    if not ok.any():
        return 0.0
    with np.errstate(all='ignore'):
        err = np.abs(got.astype(np.float64) - truth)
    err = np.where(ok, err, 0.0)
    if not np.isfinite(err).all():
        return float('inf')
    return float((err[ok] / bnd[ok]).max())


def cases():
    for fn in FUNCS:
        for K in KS:
            for inner in INNERS:
                for dt in DTYPES:
                    for imp in IMPLICIT:
                        if fn == 'logsumexp' and imp[0] != imp[1]:
                            continue
                        for idx in INDICES:
                            if fn == 'logsumexp' and idx != 0:
                                continue
                            if kprime(K, imp) - imp[1] < 1:
                                continue           # K = 1 with its only class dropped: nothing to compare
                            yield fn, K, inner, dt, imp, idx
