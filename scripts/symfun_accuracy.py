#!/usr/bin/env python
"""Accuracy of sym.sym_funm and of its gradient on the GPU -> profiles/symfun_accuracy.md: the worst ratio of the
per-record error to the unit of each bound of tests/_symfun_ref.py, per (fn, dtype, N, family).

    forward   ||Y^ - Y||_F / (n eps (L ||A||_2 + ||Y||_2))
    gradient  ||S^ - S||_F / (n eps (M2 ||A||_2 + L) ||G||_F)        (exp: n + max|l| in place of n)

The tests hold every record to 16 of these units.

    python scripts/symfun_accuracy.py [--md out.md]"""
import argparse
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _symfun_ref as R  # noqa: E402
from nitorch_fastmath_amd import sym as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    out = ['# sym_funm: accuracy on MI355X (scripts/symfun_accuracy.py)', '',
           f'Worst ratio over the {R.NB} records of tests/_symfun_ref.py `batch` (each family its slice) to the unit of',
           'the bound: forward / gradient.  The bar of the tests is 16.  float32 against numpy float64 `eigh`, float64',
           'against the longdouble Jacobi model.  `pow` is p = 1.7, `clamp` is min = 0.75.  A gradient marked * is the',
           'torch route (order above the backward cap).', '',
           '| fn | dtype | N | ' + ' | '.join(R.FAMILIES) + ' |', '|---|---|---|' + '---|' * len(R.FAMILIES)]
    worst = [0.0, 0.0]
    for fn in R.FUNCS:
        for dn, dtype in (('f32', torch.float32), ('f64', torch.float64)):
            for n in (1, 2, 3, 4, 6, 8):
                comp, cells = R.batch(dn, n, fn)
                g = R.cotangent(dn, n)
                p, vmin = R.fn_args(fn)
                mod = R.truth(dn, n, fn)
                x = torch.as_tensor(np.array(comp), device='cuda').requires_grad_(True)
                y = S.sym_funm(x, fn, p=p, min=vmin)
                y.backward(torch.as_tensor(np.array(g), device='cuda'))
                rf = R.forward_ratio(dn, fn, mod, y.detach().cpu().numpy())
                rb = R.backward_ratio(dn, fn, mod, g, x.grad.cpu().numpy())
                star = '' if n <= S._funm_cap(dtype, True) else '*'
                row = [f'{rf[cells[f]].max():.2f} / {rb[cells[f]].max():.2f}{star}' if f in cells else '-'
                       for f in R.FAMILIES]
                worst = [max(worst[0], rf.max()), max(worst[1], rb.max())]
                out.append(f'| {fn} | {dn} | {n} | ' + ' | '.join(row) + ' |')
                print(out[-1], flush=True)
    out += ['', f'Worst of all cells: forward {worst[0]:.2f}, gradient {worst[1]:.2f} (of 16).']
    text = '\n'.join(out) + '\n'
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
