#!/usr/bin/env python
"""Accuracy of the two-matrix spectral functions of sym on the GPU -> profiles/sympencil_accuracy.md: the worst ratio of
the per-record error to the unit of each bound of tests/_sympencil_ref.py (its docstring states them), per
(quantity, dtype, N, family).  The tests hold every record to C of these units; C and the ratio R_REF of the
composition it was derived from are in that module.

    python scripts/sympencil_accuracy.py [--md out.md]"""
import argparse
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _sympencil_ref as P  # noqa: E402
from nitorch_fastmath_amd import _lib, sym as S  # noqa: E402

OPS = {'function': _lib.PENCIL_OP_FUNM, 'gradient': _lib.PENCIL_OP_FUNM_BACKWARD, 'eig': _lib.PENCIL_OP_EIG,
       'dist': _lib.PENCIL_OP_DIST_BACKWARD}


def T(x, grad=False):
    return torch.as_tensor(np.array(x), device='cuda').requires_grad_(grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    out = ['# sym_pencil_funm, sym_geneigvals, sym_dist: accuracy on MI355X (scripts/sympencil_accuracy.py)', '',
           f'Worst ratio over the records of tests/_sympencil_ref.py `batch` ({P.PER} per family) to the unit of the',
           f'bound.  The bar of the tests is C = {P.C:g} = max(16, 2 R_REF rounded up to a power of two), R_REF = '
           f'{P.R_REF:g} the worst',
           'ratio of the composition of single-matrix functions (nitorch_fastmath_amd/_sympencil.py, CPU tensors, working',
           'dtype) to the same units.  float32 against numpy float64, float64 against the longdouble Jacobi model.',
           f'`pow` is t = {P.POW_P}.  Function rows: result / gradient with respect to mat.  Distance rows: d2 / its',
           'gradient with respect to a / with respect to b.  A cell marked * ran the composition route for its gradient',
           '(order above that cap), ** for everything.', '',
           '| quantity | dtype | N | ' + ' | '.join(P.FAMILIES) + ' |', '|---|---|---|' + '---|' * len(P.FAMILIES)]
    worst = {}

    def row(name, dn, n, cells, ratios, star):
        cols = [' / '.join(f'{r[cells[f]].max():.2f}' for r in ratios) + star if f in cells else '-' for f in P.FAMILIES]
        out.append(f'| {name} | {dn} | {n} | ' + ' | '.join(cols) + ' |')
        print(out[-1], flush=True)
        for k, r in enumerate(ratios):
            worst[(name.split()[0], k)] = max(worst.get((name.split()[0], k), 0.0), float(r.max()))

    for dn, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        for n in (1, 2, 3, 4, 6, 7, 8):
            def star(fwd, bwd):
                return '**' if n > S._pencil_cap(dtype, OPS[fwd]) else ('*' if n > S._pencil_cap(dtype, OPS[bwd]) else '')
            for fn in P.FUNCS:
                ca, cb, cells = P.batch(dn, n, fn)
                g = P.cotangent(dn, n, len(ca))
                mod = P.truth(dn, n, fn)
                b = T(cb, True)
                y = S.sym_pencil_funm(T(ca), b, fn, p=P.fn_p(fn))
                y.backward(T(g))
                row(f'function {fn}', dn, n, cells,
                    [P.fun_ratio(dn, fn, mod, y.detach().cpu().numpy()), P.grad_ratio(dn, fn, mod, g, b.grad.cpu().numpy())],
                    star('function', 'gradient'))
            ca, cb, cells = P.batch(dn, n, 'log')
            mod = P.truth(dn, n, 'log')
            row('eigenvalues', dn, n, cells, [P.eig_ratio(dn, mod, S.sym_geneigvals(T(cb), T(ca)).cpu().numpy())],
                star('eig', 'eig'))
            a, b = T(ca, True), T(cb, True)
            d2 = S.sym_dist(a, b, squared=True)
            d2.sum().backward()
            ra, rb = P.dist_grad_ratios(dn, mod, a.grad.cpu().numpy(), b.grad.cpu().numpy())
            row('distance d2', dn, n, cells, [P.dist2_ratio(dn, mod, d2.detach().cpu().numpy()), ra, rb], star('eig', 'dist'))
    out += ['', 'Worst of all cells: ' + ', '.join(f'{k[0]}[{k[1]}] {v:.2f}' for k, v in sorted(worst.items()))
            + f' (of {P.C:g}).']
    text = '\n'.join(out) + '\n'
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
