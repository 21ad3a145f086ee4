#!/usr/bin/env python
"""Generate tests/golden/lie_forward.npz: a truth beyond float64 for the forward kernels of `lie.expm`.  mpmath at 40
digits on float64 inputs.  Per order 2..7: 6 records of each float64 class of tests/_lie_ref.py (`FWD_CLASSES_F64`),
interleaved by class as the GPU tests' batches are (record i is of class i mod 20: 120 records), stored as `x_D`
and `t_D` = e^X rounded to float64.

`over_x_4`, `over_log2_4`: 6 general 4 x 4 matrices with ||X||_1 = 3000 whose exponential overflows float64, and
log2 |e^X| entry by entry -- no entry within 2 of the exponent 1024, so which entries overflow is beyond doubt.

    python tests/golden/make_golden_lie_forward.py        # rewrites tests/golden/lie_forward.npz (ten seconds)
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
OVER_NORM = 3000.0
OVER_COUNT = 6


def mp_expm(z):
    return mpmath.expm(mpmath.matrix(z.tolist()))


def as_float(e, D):
    return np.array([[float(e[i, j]) for j in range(D)] for i in range(D)])


def as_log2(e, D):
    return np.array([[float(mpmath.log(abs(e[i, j]), 2)) if e[i, j] != 0 else -np.inf for j in range(D)]
                     for i in range(D)])


def main():
    out = {}
    n = R.FWD_FIXTURE_COUNT * len(R.FWD_CLASSES_F64)
    for D in R.FWD_FIXTURE_ORDERS:
        assert R.fwd_classes('f64', D) == R.FWD_CLASSES_F64
        x = R.fwd_batch(n, D, 'f64', salt=1)[0].numpy()
        out[f'x_{D}'] = x
        out[f't_{D}'] = np.stack([as_float(mp_expm(x[i]), D) for i in range(n)])
        assert np.isfinite(out[f't_{D}']).all()
        print(D, n, flush=True)
    D = 4
    cand = R.build_x(('gen', OVER_NORM), 64, D, R._seed(('gen', OVER_NORM), D, 200)).numpy()
    xs, logs = [], []
    for i in range(len(cand)):
        lg = as_log2(mp_expm(cand[i]), D)
        if lg.max() > 1026 and not ((lg > 1022) & (lg < 1026)).any():
            xs.append(cand[i])
            logs.append(lg)
        if len(xs) == OVER_COUNT:
            break
    assert len(xs) == OVER_COUNT
    out[f'over_x_{D}'], out[f'over_log2_{D}'] = np.stack(xs), np.stack(logs)
    path = os.path.join(HERE, 'lie_forward.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
