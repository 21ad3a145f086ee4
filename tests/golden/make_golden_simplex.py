#!/usr/bin/env python
"""Generate tests/golden/simplex.npz from the REAL reference `simplex.py` (build container only; same
namespace shim as make_golden_lie.py) and write profiles/simplex_accuracy.md.

    python tests/golden/make_golden_simplex.py <path of the reference package nitorch_fastmath>

Per shape (K, inner): float32-rounded logits (randn scaled by 1, 10 and 80, so that float32 exp underflows
in some classes) -- they are the inputs of the float32 AND of the float64 cases, so the reference's float64
output is at once the float64 expectation and the truth of the float32 cases.  Stored: the reference's
float32 and float64 outputs of softmax / log_softmax / logit / logsumexp for the four `implicit` pairs and
implicit_index in {0, -1} (outputs the reference derives from another by moving or dropping a column are
stored once, after a bit-for-bit check: tests/_simplex_fixture.py), gradients at K = 3, special-value
vectors, and C: the next power of two at or above 4 x the worst ratio of the reference's float32 result to
the C = 1 bounds of tests/_simplex_fixture.py.
"""
import importlib
import os
import sys
import types
import warnings
import numpy as np
import torch

warnings.filterwarnings('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _simplex_fixture as F  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('NFM_REFERENCE')
if not REF:
    sys.exit('usage: make_golden_simplex.py <path of the reference package nitorch_fastmath> (or NFM_REFERENCE)')
SCALES = (1.0, 10.0, 80.0)
SPECIAL = [
    [0.5, float('inf'), -1.0], [float('nan'), 0.0, 1.0], [-float('inf')] * 3, [-float('inf'), 0.25, 2.0],
    [float('inf'), float('inf'), 0.0], [-float('inf'), float('nan'), 3.0], [0.0, 0.0, 0.0], [-200.0, -300.0, -250.0],
    [100.0, -100.0, 0.0], [-float('inf'), -float('inf'), 1.0],
]


def load_ref():
    pkg = types.ModuleType('nitorch_fastmath')
    pkg.__path__ = [REF]
    sys.modules['nitorch_fastmath'] = pkg
    return importlib.import_module('nitorch_fastmath.simplex')


def call(R, fn, x, imp, idx):
    if fn == 'logsumexp':
        return R.logsumexp(x, 1, True, imp[0])
    return getattr(R, fn)(x, 1, imp, idx)


def main():
    R = load_ref()
    gen = torch.Generator().manual_seed(20261016)
    out = {}
    worst = {fn: 0.0 for fn in F.FUNCS}
    for K in F.KS:
        for inner in F.INNERS:
            shape = F.shape_of(K, inner)
            nvox = shape[0] * shape[2]
            scale = torch.tensor([SCALES[v % 3] for v in range(nvox)], dtype=torch.float64).reshape(shape[0], 1, shape[2])
            x32 = (torch.randn(shape, dtype=torch.float64, generator=gen) * scale).float()
            out[f'x_{K}_{inner}'] = x32.numpy()
            inputs = {'x': x32,
                      'e': R.softmax(x32.double(), 1, False, 0).float(),
                      'i': R.softmax(x32.double(), 1, True, 0).float()}
            out[f'p_e_{K}_{inner}'] = inputs['e'].numpy()
            out[f'p_i_{K}_{inner}'] = inputs['i'].numpy()
            for fn in F.FUNCS:
                stored = {}
                for imp in F.IMPLICIT:
                    if fn == 'logsumexp' and imp[0] != imp[1]:
                        continue
                    for idx in F.INDICES:
                        kp = F.kprime(K, imp)
                        nidx = F.norm_index(idx, kp)
                        if kp - imp[1] < 1:
                            continue
                        if K > 1 and 0 < nidx < kp - 1:
                            continue
                        xin = inputs['x'] if fn != 'logit' else inputs['i' if imp[0] else 'e']
                        # the reference raises for an interior index and mis-reads a negative one: give it the
                        # two positions it handles, 0 and "last", in the spelling it understands
                        ridx = 0 if nidx == 0 else -1
                        if fn == 'logit' and not imp[0]:
                            ridx = nidx
                        r32 = call(R, fn, xin.clone(), imp, ridx).numpy()
                        r64 = call(R, fn, xin.double(), imp, ridx).numpy()
                        key, how = F.base_key(fn, imp, nidx)
                        for kind, arr, name in (('ref', r32, f'ref_{fn}_{key}_{K}_{inner}_f32'),
                                                ('true', r64, f'true_{fn}_{key}_{K}_{inner}')):
                            is_base = how == 'same' or (how == 'move' and nidx == kp - 1)
                            if is_base and not (fn in ('softmax', 'log_softmax') and imp == (True, True)):
                                if name in stored:
                                    assert np.array_equal(stored[name], arr, equal_nan=True), name
                                stored[name] = arr
                        todo = stored.setdefault('_check', [])
                        todo.append((fn, K, inner, imp, idx, r32, r64))
                for name, arr in stored.items():
                    if name != '_check':
                        out[name] = arr
                stored_check = stored.get('_check', [])
                out_tmp = dict(out)
                fx = types.SimpleNamespace(z=out_tmp)
                for fn_, K_, inner_, imp, idx, r32, r64 in stored_check:
                    if K_ == 1 and imp == (True, False) and idx == 0:
                        continue   # the reference puts the added class of a one-class input last whatever the index
                    got32 = F.Fixture._out(fx, 'ref', fn_, K_, inner_, 'f32', imp, idx)
                    got64 = F.Fixture._out(fx, 'true', fn_, K_, inner_, 'f64', imp, idx)
                    assert np.array_equal(got32, r32, equal_nan=True), (fn_, K_, inner_, imp, idx, 'f32')
                    assert np.array_equal(got64, r64, equal_nan=True), (fn_, K_, inner_, imp, idx, 'f64')
                    xin = out_tmp[f'x_{K_}_{inner_}'] if fn_ != 'logit' else out_tmp[f'p_{"i" if imp[0] else "e"}_{K_}_{inner_}']
                    b = F.bound(fn_, xin, r64, imp, idx, 'f32', slack=True)
                    worst[fn_] = max(worst[fn_], F.ratio(r32, r64, b))
    # gradients (float64, K = 3): only where the reference's backward is the derivative of its forward
    g = torch.Generator().manual_seed(7)
    for inner in (1, 7):
        x = torch.from_numpy(out[f'x_3_{inner}']).double()
        for imp in ((False, False), (True, True)):
            tag = 'i' if imp[0] else 'e'
            for fn in ('softmax', 'log_softmax', 'logsumexp'):
                xr = x.clone().requires_grad_()
                y = call(R, fn, xr, imp, 0)
                go = torch.randn(y.shape, dtype=torch.float64, generator=g)
                (gx,) = torch.autograd.grad(y, xr, go)
                out[f'gout_{fn}_{tag}_{inner}'] = go.numpy()
                out[f'gin_{fn}_{tag}_{inner}'] = gx.numpy()
    # special values: (n, 3, 1) vectors, every function and implicit pair, implicit_index 0, both dtypes
    sp = torch.tensor(SPECIAL, dtype=torch.float32).reshape(-1, 3, 1)
    out['special_x'] = sp.numpy()
    for fn in F.FUNCS:
        for imp in F.IMPLICIT:
            if fn == 'logsumexp' and imp[0] != imp[1]:
                continue
            xin = sp if fn != 'logit' else sp.abs().clamp_max(2.0) / 4
            t = f'{int(imp[0])}{int(imp[1])}'
            out[f'special_{fn}_{t}_f32'] = call(R, fn, xin.clone(), imp, 0).numpy()
            out[f'special_{fn}_{t}_f64'] = call(R, fn, xin.double(), imp, 0).numpy()
    ref_ratio = max(worst.values())
    C = 2.0 ** int(np.ceil(np.log2(4 * ref_ratio)))
    out['ref_ratio'] = np.float64(ref_ratio)
    out['C'] = np.float64(C)
    for fn, w in worst.items():
        out[f'ref_ratio_{fn}'] = np.float64(w)
    path = os.path.join(HERE, 'simplex.npz')
    F.pack(path, out)
    st = F.Store(path)
    assert all(np.array_equal(st[k], np.asarray(v), equal_nan=True) and st[k].dtype == np.asarray(v).dtype for k, v in out.items())
    print(path, os.path.getsize(path), 'bytes; reference ratios', worst, 'C', C)
    prof = os.path.join(os.path.dirname(os.path.dirname(HERE)), 'profiles', 'simplex_accuracy.md')
    kernel = ''
    if os.path.exists(prof):
        txt = open(prof).read()
        if '## Kernels' in txt:
            kernel = txt[txt.index('## Kernels'):]
    with open(prof, 'w') as f:
        f.write('# simplex: accuracy against the float64 truth\n\n'
                'Worst ratio |result - truth| / bound (C = 1; bounds in tests/_simplex_fixture.py) over every case of\n'
                'tests/golden/simplex.npz.\n\n## Reference (float32, CPU)\n\n| function | worst ratio |\n|---|---|\n')
        for fn, w in worst.items():
            f.write(f'| {fn} | {w:.3f} |\n')
        f.write(f'\nWorst over all: {ref_ratio:.3f}.  C = next power of two at or above 4 x that = **{C:g}**.\n\n')
        f.write(kernel or '## Kernels\n\n(not measured yet: pytest -s tests/test_gpu_simplex.py -k golden prints them on the device)\n')


if __name__ == '__main__':
    main()
