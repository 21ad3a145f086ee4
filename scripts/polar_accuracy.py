#!/usr/bin/env python
"""Accuracy of batched.batchsvdvals / batchsvd / batchpolar and of their gradients on the GPU ->
profiles/polar_accuracy.md: per (dtype, order, family) the worst ratio of the per-record error to the unit of each
bound of tests/_polar_ref.py (the bound without its constant C = 16; the tests hold every record to 16 units).

Forward: the NB records of `_polar_ref.batch` (float32 against numpy's float64 SVD; float64 against the mpmath
fixture on its records, the truth-free bounds on all).  Gradients: the fixture records, against mpmath; the unit
includes the 2 err_ref term of the bound (err_ref: the closed form from torch's CPU SVD in the same dtype).

    python scripts/polar_accuracy.py [--md out.md]"""
import argparse
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _polar_ref as R  # noqa: E402
from nitorch_fastmath_amd import batched as B  # noqa: E402

COLS = ('residual', 'orth U', 'orth Vh', 'values', 'orth R', 'A - R P', 'stretch', 'rotation', 'grad gR', 'grad gP',
        'grad gR+gP', 'grad gS')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    args = ap.parse_args()
    gpu = lambda x: torch.from_numpy(np.array(x)).cuda()          # noqa: E731
    cpu = lambda x: x.detach().cpu().numpy()          # noqa: E731
    out = ['# batchsvdvals / batchsvd / batchpolar: accuracy on MI355X (scripts/polar_accuracy.py)', '',
           'Worst ratio of the per-record error to the unit of each bound of tests/_polar_ref.py (the bound without C),',
           f'per family.  The bar of the tests is {R.C:g}.  `-`: the bound is not asked of the family.  A dtype / order marked *',
           'runs a composition for that function (order above the cap of its kernel): `polar*` the SVD kernel and torch',
           'products, `bwd*` the SVD kernel and the closed form in torch.', '',
           '| dtype | n | family | ' + ' | '.join(COLS) + ' |', '|---|---|---|' + '---|' * len(COLS)]
    worst = {}
    for dn in ('f32', 'f64'):
        for n in R.ORDERS:
            a, fam = R.batch(dn, n)
            x = gpu(a)
            S, svd, pol = B.batchsvdvals(x), B.batchsvd(x), B.batchpolar(x)
            ratios = R.forward_ratios(dn, n, cpu(S), tuple(cpu(t) for t in svd), tuple(cpu(t) for t in pol))
            af, _, gr, gp, gs, _, _, _ = R.grad_cases(dn, n)
            xf = gpu(af)
            ratios.update(R.grad_ratios(dn, n, cpu(B._polar_backward(xf, gpu(gr), None)),
                                        cpu(B._polar_backward(xf, None, gpu(gp))),
                                        cpu(B._polar_backward(xf, gpu(gr), gpu(gp))),
                                        cpu((svd[0][:len(af)] * gpu(gs)[:, None, :]) @ svd[2][:len(af)])))
            mark = ('' if n <= B.polar_max_order(R.TT[dn], 'polar') else ' polar*') + \
                   ('' if n <= B.polar_max_order(R.TT[dn], 'polar_backward') else ' bwd*')
            for fi, f in enumerate(R.FAMILIES):
                cells = []
                for c in COLS:
                    v = np.asarray(ratios[c], np.float64) * R.C
                    m = fam[:len(v)] == fi
                    skip = (c == 'rotation' or c.startswith('grad gR') or c == 'grad gP') and f == 'rankdef'
                    skip = skip or (c == 'grad gS' and f not in R.SEPARATED)
                    cells.append('-' if skip else f'{v[m].max():.2f}')
                    if not skip:
                        worst[c] = max(worst.get(c, 0.0), float(v[m].max()))
                out.append(f'| {dn}{mark} | {n} | {f} | ' + ' | '.join(cells) + ' |')
            print('\n'.join(out[-len(R.FAMILIES):]), flush=True)
    out += ['', 'Worst of all cells: ' + ', '.join(f'{c} {worst[c]:.2f}' for c in COLS) + f' (of {R.C:g}).']
    text = '\n'.join(out) + '\n'
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
