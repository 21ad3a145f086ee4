#!/usr/bin/env python
"""Generate tests/golden/lie_frechet.npz: a truth beyond float64 for the Frechet derivatives of the matrix
exponential.  mpmath at 40 digits through the block identities

    L(X, A)     = expm([[X, A], [0, X]])[:D, D:]
    L2(X, A, B) = expm([[X, A, B, 0], [0, X, 0, B], [0, 0, X, A], [0, 0, 0, X]])[:D, 3D:]

on float64 inputs.  Per order 2, 3, 4: 96 records (one and a half wavefronts) in the class order of
tests/_lie_ref.py (`CLASSES`, `FIXTURE_COUNT`): 12 per general norm {1e-3, 0.5, 2, 8, 30}, 6 per skew-symmetric
norm {4, 20, 200}, 9 per nilpotent norm {1, 5}; directions randn.  Stored per record: X, A, B, L(X, A), L2(X, A, B).

    python tests/golden/make_golden_lie_frechet.py        # rewrites tests/golden/lie_frechet.npz (minutes)
"""
import os
import sys
import mpmath
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _lie_ref as R  # noqa: E402

mpmath.mp.dps = 40


def mp_expm(z):
    e = mpmath.expm(mpmath.matrix(z.tolist()))
    return np.array([[float(e[i, j]) for j in range(z.shape[1])] for i in range(z.shape[0])])


def truth(x, a, b=None):
    Z, (r, c) = R._blocks(torch.from_numpy(x), torch.from_numpy(a), None if b is None else torch.from_numpy(b),
                          torch.float64)
    return mp_expm(Z.numpy())[r, c]


def main():
    gen = torch.Generator().manual_seed(20261018)
    out = {}
    for D in R.FIXTURE_ORDERS:
        xs = [R.build_x(cls, R.FIXTURE_COUNT[cls[0]], D, gen) for cls in R.CLASSES]
        x = torch.cat(xs).numpy()
        a = torch.randn(len(x), D, D, dtype=torch.float64, generator=gen).numpy()
        b = torch.randn(len(x), D, D, dtype=torch.float64, generator=gen).numpy()
        out[f'x_{D}'], out[f'a_{D}'], out[f'b_{D}'] = x, a, b
        out[f'L_{D}'] = np.stack([truth(x[i], a[i]) for i in range(len(x))])
        out[f'L2_{D}'] = np.stack([truth(x[i], a[i], b[i]) for i in range(len(x))])
        print(D, len(x), flush=True)
    path = os.path.join(HERE, 'lie_frechet.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
