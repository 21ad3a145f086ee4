#!/usr/bin/env python
"""Generate tests/golden/svd.npz from the REAL reference `sugar.py` on the CPU (build container only).

    python tests/golden/make_golden_svd.py <path of the reference package nitorch_fastmath>

Per dtype (f32, f64) and shape (M, N) of SHAPES, 16 records: a = randn (M x N), b with K = 3 columns, a vector v,
and the reference's results of lmdiv, inv and solvevec (non-square systems: the reference takes `pinv` whatever
the method).  Per dtype, one batch of 8 x 8 records of rank 7 (products of small integer matrices, exact in both
dtypes) and the reference's `lmdiv(method='pinv')` at rcond 1e-6 (f32) / 1e-13 (f64).

One expectation does NOT come from the reference, which is wrong there (as in make_golden_sugar.py): rmdiv,
whose code returns lmdiv(b, a)^T where its docstring says A B^-1; `{dt}_{M}x{N}_rmdiv` is ar @ pinv(a), formed by
numpy in float64.
"""
import importlib.util
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('NFM_REFERENCE')
if not REF:
    sys.exit('usage: make_golden_svd.py <path of the reference package nitorch_fastmath> (or NFM_REFERENCE)')
SHAPES = ((2, 1), (1, 4), (8, 3), (3, 8), (7, 5), (5, 7), (8, 7))
NREC, K, KR = 16, 3, 2
RCOND = {'f32': 1e-6, 'f64': 1e-13}


def load_ref():
    spec = importlib.util.spec_from_file_location('nfm_reference_sugar', os.path.join(REF, 'sugar.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    R = load_ref()
    gen = torch.Generator().manual_seed(20240917)
    out = {}
    for dt, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        def rnd(*shape):
            return torch.randn(*shape, dtype=torch.float64, generator=gen)
        for M, N in SHAPES:
            a, b, v, ar = rnd(NREC, M, N).to(dtype), rnd(NREC, M, K).to(dtype), rnd(NREC, M).to(dtype), rnd(NREC, KR, N).to(dtype)
            res = dict(a=a, b=b, v=v, ar=ar, lmdiv=R.lmdiv(a, b), inv=R.inv(a), solvevec=R.solvevec(a, v))
            for k_, t in res.items():
                out[f'{dt}_{M}x{N}_{k_}'] = t.numpy()
            out[f'{dt}_{M}x{N}_rmdiv'] = ar.double().numpy() @ np.linalg.pinv(a.double().numpy())
        p = torch.randint(-3, 4, (NREC, 8, 7), generator=gen).double()
        q = torch.randint(-3, 4, (NREC, 7, 8), generator=gen).double()
        a = p @ q
        assert (torch.linalg.matrix_rank(a) == 7).all() and a.abs().max() < 2 ** 20
        a, b = a.to(dtype), rnd(NREC, 8, K).to(dtype)
        out[f'{dt}_rank7_a'], out[f'{dt}_rank7_b'] = a.numpy(), b.numpy()
        out[f'{dt}_rank7_lmdiv'] = R.lmdiv(a, b, method='pinv', rcond=RCOND[dt]).numpy()
    path = os.path.join(HERE, 'svd.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
