#!/usr/bin/env python
"""Generate tests/golden/lie.npz from the REAL reference `_impl/expm.py` (build container only;
same namespace shim as make_golden.py).  Stores, per (dtype, order): the inputs, the reference's
output (one call per matrix, so its batch-wide stop test is a per-matrix one) and a truth computed
with mpmath at 40 digits from the dtype-rounded input.  The derivatives (float64, orders 2..4) get
their truth from the block identities

    L(X, A)     = expm([[X, A], [0, X]])[:D, D:]
    L2(X, A, B) = expm([[X, A, B, 0], [0, X, 0, B], [0, 0, X, A], [0, 0, 0, X]])[:D, 3D:]

    python tests/golden/make_golden_lie.py        # rewrites tests/golden/lie.npz
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
REF = '/root/reference/nitorch_fastmath'
mpmath.mp.dps = 40

NORMS = [1e-3, 0.5, 2.0, 8.0, 30.0]   # ||X||_1 of the general classes
SKEW, NILP = -1.0, -2.0               # class labels of the structured inputs
PER_CLASS = 6


def load_ref():
    pkg = types.ModuleType('nitorch_fastmath')
    pkg.__path__ = [REF]
    sys.modules['nitorch_fastmath'] = pkg
    return importlib.import_module('nitorch_fastmath._impl.expm')


def mp_expm(a):
    """expm of a float64 numpy matrix at 40 digits -> float64"""
    e = mpmath.expm(mpmath.matrix(a.tolist()))
    return np.array([[float(e[i, j]) for j in range(a.shape[1])] for i in range(a.shape[0])])


def frechet_truth(x, a, b=None):
    D = x.shape[0]
    if b is None:
        z = np.zeros((2 * D, 2 * D))
        z[:D, :D] = z[D:, D:] = x
        z[:D, D:] = a
        return mp_expm(z)[:D, D:]
    z = np.zeros((4 * D, 4 * D))
    for q in range(4):
        z[q * D:(q + 1) * D, q * D:(q + 1) * D] = x
    z[:D, D:2 * D] = a
    z[:D, 2 * D:3 * D] = b
    z[D:2 * D, 3 * D:] = b
    z[2 * D:3 * D, 3 * D:] = a
    return mp_expm(z)[:D, 3 * D:]


def inputs(D, gen):
    xs, cls = [], []
    for nrm in NORMS:
        for _ in range(PER_CLASS):
            x = torch.randn(D, D, dtype=torch.float64, generator=gen)
            xs.append(x * (nrm / x.abs().sum(0).max()))
            cls.append(nrm)
    if D > 1:
        for nrm in (0.5, 4.0, 20.0):
            g = torch.randn(D, D, dtype=torch.float64, generator=gen)
            s = g - g.T
            xs.append(s * (nrm / s.abs().sum(0).max()))
            cls.append(SKEW)
        for nrm in (1.0, 5.0):
            n = torch.triu(torch.randn(D, D, dtype=torch.float64, generator=gen), 1)
            xs.append(n * (nrm / max(n.abs().sum(0).max(), 1e-300)))
            cls.append(NILP)
    return torch.stack(xs), np.array(cls)


def rigid_basis():
    """3 translations + 3 rotations of 4x4 homogeneous matrices (se(3))"""
    B = torch.zeros(6, 4, 4, dtype=torch.float64)
    for k in range(3):
        B[k, k, 3] = 1
    for k, (i, j) in enumerate([(0, 1), (0, 2), (1, 2)]):
        B[3 + k, i, j], B[3 + k, j, i] = 1, -1
    return B


def affine_basis():
    """the 12 entries of the top 3 rows of a 4x4 homogeneous matrix (aff(3))"""
    B = torch.zeros(12, 4, 4, dtype=torch.float64)
    for k in range(12):
        B[k, k // 4, k % 4] = 1
    return B


def main():
    R = load_ref()
    gen = torch.Generator().manual_seed(20261016)
    out = {}
    for dt, tdt in (('f32', torch.float32), ('f64', torch.float64)):
        for D in range(1, 9):
            x, cls = inputs(D, gen)
            x = x.to(tdt)
            ref = torch.stack([R.expm(xi) for xi in x])
            true = np.stack([mp_expm(xi.double().numpy()) for xi in x])
            out[f'x_{dt}_{D}'] = x.numpy()
            out[f'ref_{dt}_{D}'] = ref.numpy()
            out[f'true_{dt}_{D}'] = true
            out[f'cls_{dt}_{D}'] = cls
    # Lie-algebra bases at D = 4 (float64)
    for name, B in (('rigid', rigid_basis()), ('affine', affine_basis())):
        p = torch.randn(8, B.shape[0], dtype=torch.float64, generator=gen) * 0.3
        out[f'{name}_basis'] = B.numpy()
        out[f'{name}_x'] = p.numpy()
        out[f'{name}_ref'] = torch.stack([R.expm(pi, B) for pi in p]).numpy()
        out[f'{name}_true'] = np.stack([mp_expm((pi[:, None, None] * B).sum(0).numpy()) for pi in p])
    # derivatives, float64, basis = None (one-hot, F = D^2): grad_X, grad_basis, unbatched hess_X
    for D in (2, 3, 4):
        n = 2
        x = torch.randn(n, D, D, dtype=torch.float64, generator=gen) * (0.7 / D)
        x[1] *= 4                                     # a matrix that needs squarings
        onehot = np.eye(D * D).reshape(D * D, D, D)
        e, dX, dB, hX = [], [], [], []
        te, tdX, thX = [], [], []
        for xi in x:
            r = R.expm_derivatives(xi, grad_X=True, grad_basis=True, hess_X=True)
            e.append(r[0][0] if r[0].dim() == 3 else r[0])
            dX.append(r[1])
            dB.append(r[2].reshape(D * D, D, D, D, D))
            hX.append(r[3])
            xn = xi.numpy()
            te.append(mp_expm(xn))
            tdX.append(np.stack([frechet_truth(xn, onehot[f]) for f in range(D * D)]))
            h = np.zeros((D * D, D * D, D, D))
            for f in range(D * D):
                for g in range(f, D * D):
                    h[f, g] = h[g, f] = frechet_truth(xn, onehot[f], onehot[g])
            thX.append(h)
        out[f'dx_{D}'] = x.numpy()
        out[f'dref_e_{D}'] = torch.stack(e).numpy()
        out[f'dref_dX_{D}'] = torch.stack(dX).numpy()
        out[f'dref_dB_{D}'] = torch.stack(dB).numpy()
        out[f'dref_hX_{D}'] = torch.stack(hX).numpy()
        out[f'dtrue_e_{D}'] = np.stack(te)
        out[f'dtrue_dX_{D}'] = np.stack(tdX)
        out[f'dtrue_hX_{D}'] = np.stack(thX)
    path = os.path.join(HERE, 'lie.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
