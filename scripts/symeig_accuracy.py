#!/usr/bin/env python
"""Accuracy of sym.sym_eigvals / sym.sym_eigh and of their gradient on the GPU -> profiles/symeig_accuracy.md.

Forward: the worst ratio per (dtype, N, cell, metric) of tests/_eig_ref.py `batch` (values, residual, orthogonality in
units of n eps |A|_2 resp. n eps); the tests hold every cell to 16.
Gradient: the worst ratio on the cells 'normal' and 'wilk' to the unit of the bounds of tests/_symeig_ref.py,

    values    |S^ - S|_F / (n eps (1 + kappa) |gl|_2)
    vectors   |S^ - S|_F / (n eps (1 + kappa) |gV|_F / gap)        kappa = |A|_2 / gap

again held to 16.

    python scripts/symeig_accuracy.py [--md out.md]"""
import argparse
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _eig_ref as E  # noqa: E402
import _symeig_ref as Q  # noqa: E402
import _symfun_ref as R  # noqa: E402
from nitorch_fastmath_amd import _lib, sym as S  # noqa: E402

ORDERS = (2, 3, 4, 5, 6, 8)


def dev_of(x):
    return torch.as_tensor(np.array(x), device='cuda')


def gradient(comp, gl, gv):
    x = dev_of(comp).requires_grad_(True)
    lam, V = S.sym_eigh(x)
    outs = [t for t, g in ((lam, gl), (V, gv)) if g is not None]
    torch.autograd.backward(outs, [dev_of(g) for g in (gl, gv) if g is not None])
    return V.detach().cpu().numpy(), x.grad.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    out = ['# sym_eigvals / sym_eigh: accuracy on MI355X (scripts/symeig_accuracy.py)', '',
           '## Forward', '',
           'Worst ratio over the records of every cell of tests/_eig_ref.py `batch` (plain and shuffled copies), per',
           'metric, and the cell it occurs in.  The bar of the tests is 16 in every cell.', '',
           '| dtype | N | values | residual | orthogonality | cells above 16 |', '|---|---|---|---|---|---|']
    cells_md = ['', '### Every cell', '', '| dtype | N | cell | values | residual | orthogonality |', '|---|---|---|---|---|---|']
    for dn in ('f32', 'f64'):
        for n in ORDERS:
            a = E.batch(dn, n)[0]
            x = dev_of(R.pack(a))
            vals = S.sym_eigvals(x).cpu().numpy()
            lam, V = S.sym_eigh(x)
            worst = E.per_cell(dn, n, E.judge(dn, n, vals, lam.cpu().numpy(), V.cpu().numpy()))
            row = []
            for m in E.METRICS:
                c = max((c for c, mm in worst if mm == m), key=lambda c: worst[(c, m)])
                row.append(f'{worst[(c, m)]:.2f} ({c})')
            over = sorted(f'{c}/{m}' for (_, _, c, m) in E.exceeding(dn, n, worst))
            out.append(f'| {dn} | {n} | ' + ' | '.join(row) + f" | {', '.join(over) if over else 'none'} |")
            print(out[-1], flush=True)
            for c in E.batch(dn, n)[1]:
                cells_md.append(f'| {dn} | {n} | {c} | ' + ' | '.join(f'{worst[(c, m)]:.2f}' for m in E.METRICS) + ' |')
    out += ['', '## Gradient', '',
            "Worst ratio on the cells 'normal' / 'wilk' for the cotangent of the values alone, of the vectors alone and of",
            'both.  The bar of the tests is 16.  float32 against numpy float64 `eigh`, float64 against the longdouble',
            'Jacobi model; no record of these cells is excluded (gap >= 64 n eps |A|_2).  A row marked * takes the split',
            'route (forward kernel, formula in torch) for the cotangent of the vectors.', '',
            '| dtype | N | values | vectors | both | smallest gap / norm |', '|---|---|---|---|---|---|']
    for dn, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        for n in ORDERS:
            full, comp, cells = Q.grad_batch(dn, n)
            gl, gv = Q.cotangents(dn, n, len(full))
            mod, row = None, []
            for a, b in ((gl, None), (None, gv), (gl, gv)):
                vecs, gx = gradient(comp, a, b)
                if mod is None:
                    mod = Q.model(dn, full, 'ascending', vecs, gl, gv)
                    assert Q.judged(dn, n, mod).all()
                r = Q.grad_ratio(dn, n, mod, gx, a, b)
                row.append(' / '.join(f'{r[cells[c]].max():.2f}' for c in Q.GRAD_CELLS))
            star = '' if n <= S._eigh_cap(dtype, _lib.EIGH_OP_BACKWARD) else '*'
            out.append(f'| {dn} | {n}{star} | ' + ' | '.join(row) + f" | {float((mod['gap'] / mod['norm']).min()):.1e} |")
            print(out[-1], flush=True)
    text = '\n'.join(out + cells_md) + '\n'
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as f:
            f.write(text)
    print('\n'.join(out))


if __name__ == '__main__':
    main()
