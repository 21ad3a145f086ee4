#!/usr/bin/env python
"""Generate tests/golden/lstsq.npz from the REAL reference `sugar.py` on the CPU (build container only).

    python tests/golden/make_golden_lstsq.py <path of the reference package nitorch_fastmath>

Per dtype (f32, f64) and shape (M, N) of SHAPES, 16 records: a = randn (M x N), b with K = 2 columns, and the
reference's `lmdiv(a, b)` (a tall system: the reference takes `pinv` whatever the method).
"""
import importlib.util
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('NFM_REFERENCE')
if not REF:
    sys.exit('usage: make_golden_lstsq.py <path of the reference package nitorch_fastmath> (or NFM_REFERENCE)')
SHAPES = ((12, 3), (33, 6), (64, 8))
NREC, K = 16, 2


def load_ref():
    spec = importlib.util.spec_from_file_location('nfm_reference_sugar', os.path.join(REF, 'sugar.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    R = load_ref()
    gen = torch.Generator().manual_seed(20241018)
    out = {}
    for dt, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        for M, N in SHAPES:
            a = torch.randn(NREC, M, N, dtype=torch.float64, generator=gen).to(dtype)
            b = torch.randn(NREC, M, K, dtype=torch.float64, generator=gen).to(dtype)
            for k_, t in dict(a=a, b=b, lmdiv=R.lmdiv(a, b)).items():
                out[f'{dt}_{M}x{N}_{k_}'] = t.numpy()
    path = os.path.join(HERE, 'lstsq.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
