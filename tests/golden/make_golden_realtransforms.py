#!/usr/bin/env python
"""Generate tests/golden/realtransforms.npz from the REAL reference `realtransforms.py` (build container only;
same namespace shim as make_golden_lie.py).

    python tests/golden/make_golden_realtransforms.py <path of the reference package nitorch_fastmath>

Everything is recorded in float64.  For every kind (dct, dst) x type (1, 2, 3) x norm x direction (forward,
inverse):
  mat_{kind}_{type}_{norm}_{dir}_{N}   the transform of the N x N identity along axis 0, i.e. the matrix itself
                                       (column n = the transform of the n-th unit impulse), N in NS
  y_{kind}_{type}_{norm}_{dir}_{tag}   the transform along the last axis of the random inputs x_{tag}: float32
                                       values (x_f32, transformed as float64) and float64 values (x_f64)
  nd_{kind}_{type}_{norm}_{dir}_{case} the n-d forms of x_nd over dims [0, 2] ('02') and over every axis ('all')
  raises                               'kind type norm dir N exception' for every case the reference raises in
"""
import importlib
import os
import sys
import types
import warnings
import numpy as np
import torch

warnings.filterwarnings('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('NFM_REFERENCE')
if not REF:
    sys.exit('usage: make_golden_realtransforms.py <path of the reference package nitorch_fastmath> (or NFM_REFERENCE)')
NS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17)
KINDS = ('dct', 'dst')
NORMS = ('backward', 'forward', 'ortho', 'ortho_scipy')


def load_ref():
    pkg = types.ModuleType('nitorch_fastmath')
    pkg.__path__ = [REF]
    sys.modules['nitorch_fastmath'] = pkg
    return importlib.import_module('nitorch_fastmath.realtransforms')


def main():
    R = load_ref()
    gen = torch.Generator().manual_seed(20261018)
    out = {}
    raises = []
    out['x_f32'] = torch.randn(5, 7, dtype=torch.float32, generator=gen).double().numpy()
    out['x_f64'] = torch.randn(4, 12, dtype=torch.float64, generator=gen).numpy()
    out['x_nd'] = torch.randn(6, 5, 7, dtype=torch.float64, generator=gen).numpy()
    for kind in KINDS:
        for type in (1, 2, 3):
            for norm in NORMS:
                for direction in ('fwd', 'inv'):
                    name = ('i' if direction == 'inv' else '') + kind
                    fn, fnn = getattr(R, name), getattr(R, name + 'n')
                    key = f'{kind}_{type}_{norm}_{direction}'
                    for N in NS:
                        try:
                            out[f'mat_{key}_{N}'] = fn(torch.eye(N, dtype=torch.float64), 0, norm, type).numpy()
                        except Exception as e:   # noqa: BLE001 -- the exception's name is the record
                            raises.append(f'{kind} {type} {norm} {direction} {N} {e.__class__.__name__}')
                    for tag in ('f32', 'f64'):
                        out[f'y_{key}_{tag}'] = fn(torch.from_numpy(out[f'x_{tag}']), -1, norm, type).numpy()
                    xnd = torch.from_numpy(out['x_nd'])
                    out[f'nd_{key}_02'] = fnn(xnd, [0, 2], norm, type).numpy()
                    out[f'nd_{key}_all'] = fnn(xnd, None, norm, type).numpy()
    out['raises'] = np.array(raises)
    out['ns'] = np.array(NS)
    path = os.path.join(HERE, 'realtransforms.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', len(out), 'arrays;', len(raises), 'raising cases')


if __name__ == '__main__':
    main()
