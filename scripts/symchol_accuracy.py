#!/usr/bin/env python
"""Accuracy of the Cholesky functions of `sym` (sym_chol, sym_chol_apply, sym_logdet, sym_mahalanobis,
sym_gauss_logpdf and the gradients of the three scalars) on the GPU -> profiles/symchol_accuracy.md.

The worst ratio per (dtype, N, op, cell) of the 1200-record batch of tests/_symchol_ref.py to its per-record
first-order bounds (the docstring of that file states them); the tests hold every cell to 1.  Beside it, the same
ratios for the CPU entry nfm_sym_chol_host (the record routines the kernels run) and for a plain numpy Cholesky in the
working precision, which validates the input cells.

    python scripts/symchol_accuracy.py [--md out.md]"""
import argparse
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _symchol_ref as C  # noqa: E402
import _symfun_ref as R  # noqa: E402
from nitorch_fastmath_amd import _lib, sym as S  # noqa: E402

FORWARD_OPS = ('factor',) + C.APPLY + C.SCALARS


def dev_of(x):
    return torch.as_tensor(np.array(x), device='cuda')


def gpu_forward(op, x, v):
    if op == 'factor':
        return S.sym_chol(x)
    if op in C.APPLY:
        return S.sym_chol_apply(x, v, op)
    if op == 'logdet':
        return S.sym_logdet(x)
    if op in ('maha', 'maha_sqrt'):
        return S.sym_mahalanobis(x, v, squared=op == 'maha')
    return S.sym_gauss_logpdf(x, v)


def gpu_backward(op, x, v, g):
    a, b = x.clone().requires_grad_(True), v.clone().requires_grad_(True)
    gpu_forward(op, a, b).backward(g)
    return a.grad if op == 'logdet' else torch.cat([a.grad, b.grad], -1)


def host(dn, n, op, comp, vec, g=None):
    T = R.NP[dn]
    comp, vec = np.ascontiguousarray(comp, T), np.ascontiguousarray(vec, T)
    nb, K = comp.shape
    size = (K + (0 if op == 'logdet' else n)) if g is not None else (K if op == 'factor' else (n if op in C.APPLY else 1))
    out = np.zeros((nb, size), T)
    g = None if g is None else np.ascontiguousarray(g, T)
    rc = _lib.lib().nfm_sym_chol_host(0 if dn == 'f32' else 1, n, C.CODE[op], nb, comp.ctypes.data, vec.ctypes.data,
                                      None if g is None else g.ctypes.data, out.ctypes.data)
    assert rc == 0
    return out[:, 0] if op in C.SCALARS and g is None else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    out = ['# Cholesky functions of sym: accuracy on MI355X (scripts/symchol_accuracy.py)', '',
           'Worst ratio of the error to the per-record first-order bound of tests/_symchol_ref.py over the 1200 records',
           'of every (dtype, N), and the cell it occurs in.  The bar of the tests is 1 in every cell.  `host`: the CPU',
           'entry nfm_sym_chol_host; `plain`: a numpy Cholesky in the working precision (forward ops only).', '',
           '| dtype | N | op | GPU worst | in cell | host worst | plain worst |', '|---|---|---|---|---|---|---|']
    cells_md = ['', '## Every cell (GPU)', '', '| dtype | N | op | ' + ' | '.join(C.CELLS) + ' |',
                '|---|---|---|' + '---|' * len(C.CELLS)]
    top = 0.0
    for dn in ('f32', 'f64'):
        for n in C.ORDERS:
            comp, vec, g, cells = C.batch(dn, n)
            assert C.judged(dn, n, comp).all()
            m = C.truth(dn, n)
            x, v, gg = dev_of(comp), dev_of(vec), dev_of(g)
            pl = C.plain(dn, comp, vec)
            rows = []
            for op in FORWARD_OPS:
                rows.append((op, C.forward_ratio(dn, m, op, gpu_forward(op, x, v).cpu().numpy()),
                             C.forward_ratio(dn, m, op, host(dn, n, op, comp, vec)),
                             C.forward_ratio(dn, m, op, pl[op])))
            for op in C.SCALARS:
                rows.append((op + ' backward', C.backward_ratio(dn, m, op, gpu_backward(op, x, v, gg).cpu().numpy()),
                             C.backward_ratio(dn, m, op, host(dn, n, op, comp, vec, g)), None))
            for op, r, rh, rp in rows:
                w = C.worst(r, cells)
                c = max(w, key=w.get)
                top = max(top, w[c])
                out.append(f'| {dn} | {n} | {op} | {w[c]:.3f} | {c} | {rh.max():.3f} | '
                           + ('-' if rp is None else f'{rp.max():.3f}') + ' |')
                cells_md.append(f'| {dn} | {n} | {op} | ' + ' | '.join(f'{w[c]:.3f}' for c in C.CELLS) + ' |')
    out += ['', f'Worst ratio of all: {top:.3f} (of 1).'] + cells_md
    text = '\n'.join(out) + '\n'
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
