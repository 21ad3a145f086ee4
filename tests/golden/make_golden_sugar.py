#!/usr/bin/env python
"""Generate tests/golden/sugar.npz from the REAL reference `sugar.py` on the CPU (build container only).

    python tests/golden/make_golden_sugar.py <path of the reference package nitorch_fastmath>

Per dtype (f32, f64) and order N in 1..8 and 12, 16 records: a = randn + 8 I, an SPD matrix, b with K = 3
columns, a vector, and the reference's results of lmdiv (all four methods), inv, solvevec, kron2, outer, trace,
dot, mdot and round.

Two expectations do NOT come from the reference, which is wrong there:
  * rmdiv: its code returns lmdiv(b, a)^T = A^T B^-T (and raises unless k == m) where its docstring says A B^-1;
    `{dt}_{N}_rmdiv` is ar @ inv(a), formed by numpy in float64.
  * inv(method='chol') of a 2-D matrix: it hands the matrix itself to torch.cholesky_inverse, where the factor
    belongs; `{dt}_{N}_inv_chol_2d` is numpy's float64 inverse of the first SPD record.
"""
import importlib.util
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('NFM_REFERENCE')
if not REF:
    sys.exit('usage: make_golden_sugar.py <path of the reference package nitorch_fastmath> (or NFM_REFERENCE)')
ORDERS = tuple(range(1, 9)) + (12,)
NREC, K, KR = 16, 3, 2


def load_ref():
    spec = importlib.util.spec_from_file_location('nfm_reference_sugar', os.path.join(REF, 'sugar.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    R = load_ref()
    gen = torch.Generator().manual_seed(20240611)
    out = {}
    for dt, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        for N in ORDERS:
            def rnd(*shape):
                return torch.randn(*shape, dtype=torch.float64, generator=gen)
            a = (rnd(NREC, N, N) + 8 * torch.eye(N, dtype=torch.float64)).to(dtype)
            g = rnd(NREC, N, N)
            spd = (g @ g.transpose(-1, -2) / N + torch.eye(N, dtype=torch.float64)).to(dtype)
            b, v, w, ar = rnd(NREC, N, K).to(dtype), rnd(NREC, N).to(dtype), rnd(NREC, K).to(dtype), rnd(NREC, KR, N).to(dtype)
            res = dict(a=a, spd=spd, b=b, v=v, w=w, ar=ar)
            for m in ('lu', 'svd', 'pinv'):
                res['lmdiv_' + m] = R.lmdiv(a, b, method=m)
                res['inv_' + m] = R.inv(a, method=m)
            res['lmdiv_chol'] = R.lmdiv(spd, b, method='chol')
            res['inv_chol'] = R.inv(spd, method='chol')
            res['solvevec'] = R.solvevec(a, v)
            res['kron2'] = R.kron2(a[0], b[0])
            res['outer'] = R.outer(v, w)
            res['trace'] = R.trace(a)
            res['dot'] = R.dot(v, b[..., 0])
            res['mdot'] = R.mdot(a, spd)
            res['round'] = R.round(a, 2)
            for k_, t in res.items():
                out[f'{dt}_{N}_{k_}'] = t.numpy()
            out[f'{dt}_{N}_rmdiv'] = ar.double().numpy() @ np.linalg.inv(a.double().numpy())
            out[f'{dt}_{N}_inv_chol_2d'] = np.linalg.inv(spd[0].double().numpy())
    path = os.path.join(HERE, 'sugar.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
