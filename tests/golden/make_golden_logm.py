#!/usr/bin/env python
"""Generate tests/golden/logm.npz from the REAL reference `lie.logm` / `lie.meanm` (build container only;
same namespace shim as make_golden_lie.py).  Stores, per (dtype, order 1..8): the inputs, the reference's
output (float64 whatever the input dtype: scipy upcasts) and the truth, `mpmath.logm` at 40 digits of the
dtype-rounded input (its imaginary part is asserted to vanish at 40 digits).  Input classes (`cls_*`):

    > 0      A = expm(X) with ||X||_1 = cls
    SPD      G G^T + D I
    ROT      expm(skew), largest rotation angle 0.5, 2 or 3 (< pi)
    UNIP     I + N, N strictly upper triangular (the finite series of log(I + N) is a second truth)

plus 4x4 rigid and affine matrices from make_golden_lie.py's bases, one block of inputs without a real
principal logarithm (`bad_*`: inputs only), and the reference's `meanm` on three float64 sets with the
residual sum of squares of its result.

    python tests/golden/make_golden_logm.py        # rewrites tests/golden/logm.npz
"""
import importlib
import os
import sys
import types
import warnings
import mpmath
import numpy as np
import torch

warnings.filterwarnings('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_lie import REF, rigid_basis, affine_basis  # noqa: E402

mpmath.mp.dps = 40
NORMS = [1e-3, 0.1, 0.5, 2.0, 4.0]
SPD, ROT, UNIP = -1.0, -2.0, -3.0
PER_CLASS = 4


def load_ref():
    pkg = types.ModuleType('nitorch_fastmath')
    pkg.__path__ = [REF]
    sys.modules['nitorch_fastmath'] = pkg
    return importlib.import_module('nitorch_fastmath.lie')


def mp_logm(a):
    """principal logarithm of a float64 numpy matrix at 40 digits -> float64 (real; asserted)"""
    L = mpmath.logm(mpmath.matrix(a.tolist()))
    n = a.shape[0]
    re = np.array([[float(mpmath.re(L[i, j])) for j in range(n)] for i in range(n)])
    im = max(abs(mpmath.im(L[i, j])) for i in range(n) for j in range(n))
    assert im <= mpmath.mpf(10) ** -34 * max(1.0, np.abs(re).max()), im
    return re


def inputs(D, gen):
    eye = torch.eye(D, dtype=torch.float64)
    xs, cls = [], []
    for nrm in NORMS:
        for _ in range(PER_CLASS):
            x = torch.randn(D, D, dtype=torch.float64, generator=gen)
            xs.append(torch.linalg.matrix_exp(x * (nrm / x.abs().sum(0).max())))
            cls.append(nrm)
    for _ in range(PER_CLASS):
        g = torch.randn(D, D, dtype=torch.float64, generator=gen)
        xs.append(g @ g.T + D * eye)
        cls.append(SPD)
    if D > 1:
        for angle in (0.5, 2.0, 3.0):
            g = torch.randn(D, D, dtype=torch.float64, generator=gen)
            s = g - g.T
            s = s * (angle / torch.linalg.eigvals(s).imag.abs().max())
            xs.append(torch.linalg.matrix_exp(s))
            cls.append(ROT)
        for nrm in (1.0, 5.0):
            n = torch.triu(torch.randn(D, D, dtype=torch.float64, generator=gen), 1)
            xs.append(eye + n * (nrm / max(n.abs().sum(0).max(), 1e-300)))
            cls.append(UNIP)
    return torch.stack(xs), np.array(cls)


def bad_inputs(D):
    """no real principal logarithm: an eigenvalue -1, a singular matrix, a reflection, a NaN and an inf entry"""
    eye = torch.eye(D, dtype=torch.float64)
    d = torch.arange(1, D + 1, dtype=torch.float64)
    neg = torch.diag(d.clone())
    neg[0, 0] = -1
    sing = torch.diag(d.clone())
    sing[0, 0] = 0
    v = torch.ones(D, 1, dtype=torch.float64) / D ** 0.5
    refl = eye - 2 * v @ v.T
    nan = eye.clone()
    nan[-1, 0] = float('nan')
    inf = eye.clone()
    inf[0, -1] = float('inf')
    return torch.stack([neg, sing, refl, nan, inf])


def residual(R, mean, mats):
    """sum of squares of mean_n logm(mean^-1 A_n), with the reference's own logm"""
    logs = R.logm(torch.linalg.solve(mean, mats))
    return float(logs.mean(0).square().sum())


def main():
    R = load_ref()
    gen = torch.Generator().manual_seed(20261016)
    out = {}
    for dt, tdt in (('f32', torch.float32), ('f64', torch.float64)):
        for D in range(1, 9):
            x, cls = inputs(D, gen)
            x = x.to(tdt)
            ref = R.logm(x)
            assert not ref.is_complex()
            out[f'x_{dt}_{D}'] = x.numpy()
            out[f'ref_{dt}_{D}'] = ref.double().numpy()
            out[f'true_{dt}_{D}'] = np.stack([mp_logm(xi.double().numpy()) for xi in x])
            out[f'cls_{dt}_{D}'] = cls
            out[f'bad_{dt}_{D}'] = bad_inputs(D).to(tdt).numpy()
    sets = {}
    for name, B in (('rigid', rigid_basis()), ('affine', affine_basis())):
        p = torch.randn(8, B.shape[0], dtype=torch.float64, generator=gen) * 0.3
        a = torch.linalg.matrix_exp(torch.einsum('nf,fij->nij', p, B))
        out[f'{name}_x'] = a.numpy()
        out[f'{name}_ref'] = R.logm(a).double().numpy()
        out[f'{name}_true'] = np.stack([mp_logm(ai.numpy()) for ai in a])
        n = {'rigid': 7, 'affine': 12}[name]
        p = torch.randn(n, B.shape[0], dtype=torch.float64, generator=gen) * 0.4
        sets[name] = torch.linalg.matrix_exp(torch.einsum('nf,fij->nij', p, B))
    g = torch.randn(16, 3, 3, dtype=torch.float64, generator=gen)
    sets['spd'] = g @ g.transpose(-1, -2) + 3 * torch.eye(3, dtype=torch.float64)
    for name, mats in sets.items():
        mean = R.meanm(mats)
        out[f'meanm_{name}_x'] = mats.numpy()
        out[f'meanm_{name}_ref'] = mean.numpy()
        out[f'meanm_{name}_sos'] = np.array(residual(R, mean, mats))
    path = os.path.join(HERE, 'logm.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
