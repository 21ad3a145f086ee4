#!/usr/bin/env python
"""Accuracy of the backward kernels of the Cholesky factor (the gradients of sym_chol and sym_chol_apply) on the GPU
-> profiles/cholgrad_accuracy.md.

The worst ratio per (dtype, N, op, cell) of the 1200-record batch of tests/_symchol_ref.py to the per-record
first-order bounds of tests/_cholgrad_ref.py (its docstring states them); the tests hold every cell to 1.  Beside it,
the same ratios for the CPU entry nfm_sym_chol_grad_host (the record routines the kernels run) and for a plain numpy
implementation in the working precision, which validates the bounds.  `factored`: the gradient with respect to the
factor handed in (tests/_cholgrad_ref.py: factor_input).

    python scripts/cholgrad_accuracy.py [--md out.md]"""
import argparse
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _cholgrad_ref as G  # noqa: E402
import _symchol_ref as C  # noqa: E402
import _symfun_ref as R  # noqa: E402
from nitorch_fastmath_amd import _lib, sym as S  # noqa: E402


def dev_of(x):
    return torch.as_tensor(np.array(x), device='cuda')


def gpu(op, mat, vec, cot, factored):
    a, b = dev_of(mat).requires_grad_(True), dev_of(vec).requires_grad_(True)
    res = S.sym_chol(a) if op == 'factor' else S.sym_chol_apply(a, b, op, factored=factored)
    res.backward(dev_of(cot))
    return (a.grad if op == 'factor' else torch.cat([a.grad, b.grad], -1)).cpu().numpy()


def host(dn, n, op, mat, vec, cot, factored):
    T = R.NP[dn]
    mat, vec, cot = (np.ascontiguousarray(t, T) for t in (mat, vec, cot))
    nb, K = mat.shape
    out = np.zeros((nb, K if op == 'factor' else K + n), T)
    rc = _lib.lib().nfm_sym_chol_grad_host(0 if dn == 'f32' else 1, n, C.CODE[op] | (C.FACTORED if factored else 0), nb,
                                           mat.ctypes.data, None if op == 'factor' else vec.ctypes.data, cot.ctypes.data,
                                           out.ctypes.data)
    assert rc == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    out = ['# Gradients of the Cholesky factor: accuracy on MI355X (scripts/cholgrad_accuracy.py)', '',
           'Worst ratio of the error to the per-record first-order bound of tests/_cholgrad_ref.py over the 1200 records',
           'of every (dtype, N), and the cell it occurs in.  The bar of the tests is 1 in every cell.  `host`: the CPU',
           'entry nfm_sym_chol_grad_host; `plain`: numpy substitutions and products in the working precision.', '',
           '| dtype | N | op | GPU worst | in cell | host worst | plain worst |', '|---|---|---|---|---|---|---|']
    cells_md = ['', '## Every cell (GPU)', '', '| dtype | N | op | ' + ' | '.join(C.CELLS) + ' |',
                '|---|---|---|' + '---|' * len(C.CELLS)]
    top = 0.0
    for dn in ('f32', 'f64'):
        for n in C.ORDERS:
            comp, vec, _, cells = C.batch(dn, n)
            assert C.judged(dn, n, comp).all()
            Gc, gc = G.cotangents(dn, n)
            for op, factored in [(op, False) for op in G.OPS] + [(op, True) for op in C.APPLY]:
                m = G.truth(dn, n, factored)
                mat = G.factor_input(dn, n) if factored else comp
                cot = Gc if op == 'factor' else gc
                r, rh, rp = (G.ratio(dn, m, op, got, vec, cot) for got in
                             (gpu(op, mat, vec, cot, factored), host(dn, n, op, mat, vec, cot, factored),
                              G.plain(dn, n, op, mat, vec, cot, factored)))
                w = C.worst(r, cells)
                c = max(w, key=w.get)
                top = max(top, w[c])
                name = op + (' factored' if factored else '')
                out.append(f'| {dn} | {n} | {name} | {w[c]:.3f} | {c} | {rh.max():.3f} | {rp.max():.3f} |')
                cells_md.append(f'| {dn} | {n} | {name} | ' + ' | '.join(f'{w[c]:.3f}' for c in C.CELLS) + ' |')
    out += ['', f'Worst ratio of all: {top:.3f} (of 1).'] + cells_md
    text = '\n'.join(out) + '\n'
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
