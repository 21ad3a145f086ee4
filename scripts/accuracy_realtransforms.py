#!/usr/bin/env python
"""Worst observed fraction of the error bound of the real-transform kernels (the lane kernels up to `max_len`, the
matrix-core kernel from there to `mm_max_len`), per kind, type and N (over the four
norms, both transpose settings, unit impulses and dense random lines, lines along the first and the last axis).
The bound is tests/_realtransforms_ref.bound: (N + 6) eps sum |M_kn| |x_n| + the smallest normal number.

    python scripts/accuracy_realtransforms.py [--md out.md]"""
import argparse
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _realtransforms_ref as R  # noqa: E402
from nitorch_fastmath_amd import realtransforms as RT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    lines = ['| kind | type | N | float32 | float64 |', '|---|---|---|---|---|']
    for kind in R.KINDS:
        for type in R.TYPES:
            for N in (2, 3, 8, 17, 32, 33, 64, 65, 128, 129, 182, 218, 256):
                row = []
                for dtype, td in ((np.float32, torch.float32), (np.float64, torch.float64)):
                    if N > max(RT.max_len(td), RT.mm_max_len(td)):
                        row.append('-')
                        continue
                    worst = 0.0
                    xs = [np.eye(N, dtype=dtype), rng.standard_normal((300, N)).astype(dtype)]
                    for norm in R.NORMS:
                        M = R.matrix(kind, type, norm, N)
                        for tr in (False, True):
                            Mt = M.T if tr else M
                            for x in xs:
                                for axis, xx in ((1, x), (0, np.ascontiguousarray(x.T))):
                                    got = RT._apply(torch.from_numpy(xx).cuda(), [axis], R.KINDS.index(kind), type, norm, tr)
                                    worst = max(worst, R.ratio(got.cpu().numpy(), R.apply(Mt, xx, axis),
                                                               R.bound(Mt, xx, dtype, axis)))
                    row.append(f'{worst:.3f}')
                r = f'| {kind} | {type} | {N} | {row[0]} | {row[1]} |'
                print(r, flush=True)
                lines.append(r)
    if a.md:
        with open(a.md, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
