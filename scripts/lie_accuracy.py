#!/usr/bin/env python
"""Accuracy table of lie.expm / expm_derivatives against the 40-digit truth of tests/golden/lie.npz:
per (dtype, D) the worst error max|K - T| / max|T| of the kernel and of the reference, and the worst ratio
err / (D eps (1 + ||X||_1)) -- the constant C of the test bound C D eps (1 + ||X||_1).

    python scripts/lie_accuracy.py [--md out.md]"""
import argparse
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nitorch_fastmath_amd as N  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    a = ap.parse_args()
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'lie.npz'))
    lines = ['| dtype | D | kernel worst err | reference worst err | kernel worst C | reference worst C (finite) |',
             '|---|---|---|---|---|---|']
    worst = 0.0
    for dt, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        eps = torch.finfo(dtype).eps
        for D in range(1, 9):
            x, ref, true = (g[f'{k}_{dt}_{D}'] for k in ('x', 'ref', 'true'))
            k = N.lie.expm(torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float64)
            den = np.abs(true).max((1, 2))
            ek = np.abs(k - true).max((1, 2)) / den
            er = np.abs(ref.astype(np.float64) - true).max((1, 2)) / den
            b = D * eps * (1 + np.abs(x.astype(np.float64)).sum(1).max(1))
            ck, cr = ek / b, er / b
            worst = max(worst, ck.max())
            lines.append(f'| {dt} | {D} | {ek.max():.2e} | {np.nanmax(er):.2e} | {ck.max():.2f} | '
                         f'{np.nanmax(np.where(np.isfinite(cr), cr, 0)):.3g} |')
    dl = ['', '| derivatives (float64) | D | dX worst err | hX worst err | worst C |', '|---|---|---|---|---|']
    worst_d = 0.0
    for D in (2, 3, 4):
        x = torch.from_numpy(g[f'dx_{D}']).cuda()
        _, dX, hX = N.lie.expm_derivatives(x, grad_X=True, hess_X=True)
        xn = g[f'dx_{D}']
        b = D * 2.0 ** -52 * (1 + np.abs(xn).sum(1).max(1))
        e1 = np.abs(dX.cpu().numpy() - g[f'dtrue_dX_{D}']).reshape(2, -1).max(1) / np.abs(g[f'dtrue_dX_{D}']).reshape(2, -1).max(1)
        e2 = np.abs(hX.cpu().numpy() - g[f'dtrue_hX_{D}']).reshape(2, -1).max(1) / np.abs(g[f'dtrue_hX_{D}']).reshape(2, -1).max(1)
        c = max((e1 / b).max(), (e2 / b).max())
        worst_d = max(worst_d, c)
        dl.append(f'| | {D} | {e1.max():.2e} | {e2.max():.2e} | {c:.2f} |')
    # 10^6 random matrices (randn * 0.7) against matrix_exp in float64 on the device, as tests/test_gpu_lie.py::test_scale
    sl = ['', '| 10^6 x randn * 0.7 vs matrix_exp (float64) | D | worst err | worst C |', '|---|---|---|---|']
    gen = torch.Generator(device='cuda').manual_seed(7)
    for dtype in (torch.float32, torch.float64):
        for D in (3, 4):
            x = (torch.randn(10 ** 6, D, D, dtype=torch.float64, device='cuda', generator=gen) * 0.7).to(dtype)
            t = torch.linalg.matrix_exp(x.double())
            err = (N.lie.expm(x).double() - t).abs().amax((-2, -1)) / t.abs().amax((-2, -1))
            c = err / (D * torch.finfo(dtype).eps * (1 + x.double().abs().sum(-2).amax(-1)))
            sl.append(f'| {str(dtype)[6:]} | {D} | {float(err.max()):.2e} | {float(c.max()):.2f} |')
    out = '\n'.join(lines + dl + sl + ['', f'worst C on the fixture: expm {worst:.2f}, derivatives {worst_d:.2f}']) + '\n'
    print(out)
    if a.md:
        open(a.md, 'w').write(out)


if __name__ == '__main__':
    main()
