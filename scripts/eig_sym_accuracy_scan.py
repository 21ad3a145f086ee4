#!/usr/bin/env python
"""Per-record accuracy scan of eig_sym (tests/_eig_ref.py) -> profiles/eig_sym_accuracy.md.

    scan   [--oracle DIR] --out scan.json      the CPU oracle (of this tree, or of another checkout's oracle/
                                               directory: the 'before' column) on every (dtype, order) batch
    gpu    --out gpu.json                      the kernels, both arithmetic modes, contiguous operands
    window [--oracle DIR]                      the oracle at every power of two around the ends of the native
                                               window (how NFM_EIG_WINDOW_LO / HI were chosen)
    table  --before B --after A [--gpu G]      the markdown table (stdout)

A cell's figure is its worst record's err / (n eps |A|_2) (values, residual) or / (n eps) (orthogonality)."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import _eig_ref as E  # noqa: E402


def load_oracle(path):
    if path is None:
        import oracle
        oracle.build()
        return oracle
    spec = importlib.util.spec_from_file_location('oracle_other', os.path.join(path, 'oracle.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    return mod


def key(dn, n, cell, metric):
    return f'{dn}|{n}|{cell}|{metric}'


def scan(backend, out):
    for dn in ('f32', 'f64'):
        for n in E.ORDERS:
            a = E.batch(dn, n)[0]
            vals = backend.eig_sym(a)
            vals_u, vecs = backend.eig_sym(a, True)
            for (cell, metric), r in E.per_cell(dn, n, E.judge(dn, n, vals, vals_u, vecs)).items():
                out[key(dn, n, cell, metric)] = r
    return out


def gpu_backend(mode):
    import torch
    import nitorch_fastmath_amd as N

    class B:
        @staticmethod
        def eig_sym(a, compute_u=False):
            r = N.qr.eig_sym(torch.from_numpy(np.ascontiguousarray(a)).cuda(), compute_u=compute_u, arithmetic=mode)
            return tuple(x.cpu().numpy() for x in r) if compute_u else r.cpu().numpy()
    return B


def window(oracle):
    """symmetrised N(0, 1) and graded records times 2^k, k around both ends of the window: worst values and
    residual ratio per k (orders 3, 8, 16)"""
    for dn, ks in (('f32', list(range(-70, -44)) + list(range(40, 66))),
                   ('f64', list(range(-520, -470, 2)) + list(range(470, 516, 2)))):
        for k in ks:
            row = []
            for n in (3, 8, 16):
                rng = np.random.default_rng(9000 + n)
                a = np.concatenate([E.family(f, rng, 256, n) for f in E.SWEEP_FAMILIES])
                a = np.ldexp(a, k).astype(E.NP[dn])
                a = np.tril(a) + np.tril(a, -1).swapaxes(-1, -2)
                tr = E.truth_of(a)
                vals = oracle.eig_sym(a)
                vals_u, vecs = oracle.eig_sym(a, True)
                r = E.judge(dn, n, vals, vals_u, vecs, tr)
                row.append(f'{r["values"].max():9.3g} {r["residual"].max():9.3g}')
            print(f'{dn} 2^{k:5d} | ' + ' | '.join(row), flush=True)


def fmt(x):
    if x is None:
        return '-'
    if not np.isfinite(x):
        return 'inf'
    return f'{x:.3g}' if x < 1e4 else f'{x:.1e}'


def table(before, after, gpu):
    cols = ['oracle before', 'oracle after'] + (['GPU reference', 'GPU fast'] if gpu else [])
    print('| dtype | n | cell | metric | ' + ' | '.join(cols) + ' |')
    print('|---|---|---|---|' + '---|' * len(cols))
    for k in after:
        dn, n, cell, metric = k.split('|')
        vals = [before.get(k), after[k]] + ([gpu['reference'].get(k), gpu['fast'].get(k)] if gpu else [])
        print(f'| {dn} | {n} | {cell} | {metric} | ' + ' | '.join(fmt(v) for v in vals) + ' |')
    sound = {k: v for k, v in after.items()
             if (k.split('|')[0], int(k.split('|')[1]), *k.split('|')[2:]) not in E.REFERENCE_EXCEEDS}
    worst = max(sound, key=sound.get)
    print(f'\nworst sound cell of the oracle: {worst} = {sound[worst]:.3g}; '
          f'C = next power of two >= 4 x that = {2.0 ** np.ceil(np.log2(4 * sound[worst])):g}')


def main():
    p = argparse.ArgumentParser()
    p.add_argument('cmd', choices=['scan', 'gpu', 'window', 'table'])
    p.add_argument('--oracle')
    p.add_argument('--out')
    p.add_argument('--before')
    p.add_argument('--after')
    p.add_argument('--gpu')
    a = p.parse_args()
    if a.cmd == 'scan':
        res = scan(load_oracle(a.oracle), {})
    elif a.cmd == 'gpu':
        res = {mode: scan(gpu_backend(mode), {}) for mode in ('reference', 'fast')}
    elif a.cmd == 'window':
        return window(load_oracle(a.oracle))
    else:
        ld = lambda f: json.load(open(f)) if f else None
        return table(ld(a.before) or {}, ld(a.after), ld(a.gpu))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=0)


if __name__ == '__main__':
    main()
