#!/usr/bin/env python
"""Throughput of lie.expm (nfm_lie.hip) against torch.linalg.matrix_exp on the same device, and of the
Frechet kernel over a (n, F = 12) affine-basis batch -- the `grad_X` launch of expm_derivatives.

Inputs: randn * 0.3 (||X||_1 around 1, the range registration parameters live in).  Per row: matrices/s,
the mean degree m and squarings s the kernel runs (replayed on the host with the kernel's formulas,
nfm_lie_ops.hpp), the share of the larger roofline bound (FLOPs done over the vector peak -- FP32 157.3 TF
from MI355X_MICROARCH.md, FP64 78.6 TF vendor spec -- or algorithmic bytes over 8 TB/s), and the ratio
to matrix_exp (for the Frechet rows: the block identity L(X, A) = expm([[X, A], [0, X]])[:D, D:] on it).

    python scripts/bench_lie.py [--md out.md] [--n 10000000]"""
import argparse
import math
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timeit  # noqa: E402
import nitorch_fastmath_amd as N  # noqa: E402

PEAK = {torch.float32: 157.3e12, torch.float64: 78.6e12}
BW = 8.0e12


def degree_and_squarings(x, tol=1e-32, max_order=10000):
    """host replay of lie_scale / lie_degree (nfm_lie_ops.hpp) on a sample"""
    x = x.double()
    D = x.shape[-1]
    n1 = x.abs().sum(-2).amax(-1)
    _, e = torch.frexp(n1)
    s = e.clamp(min=0, max=64)
    y = x / (2.0 ** s)[..., None, None]
    b = y.square().sum((-2, -1)).sqrt().tolist()
    lim = D * D * tol
    ms = []
    for bi in b:
        term, m = bi, 1
        for n in range(2, max_order + 1):
            term = term * bi / n
            m = n
            if not term * term > lim or math.isinf(term):
                break
        ms.append(m)
    return sum(ms) / len(ms), float(s.double().mean())


def row(name, dtype, D, n, fn, ref, flops_per, bytes_per, m, s):
    t = timeit(fn)
    tr = timeit(ref) if ref is not None else float('nan')
    fl, by = flops_per * n, bytes_per * n
    share_c, share_b = fl / t / PEAK[dtype], by / t / BW
    bound = 'compute' if share_c >= share_b else 'memory'
    return (f'| {name} | {str(dtype)[6:]} | {D} | {n:.0e} | {n / t / 1e9:.3f} | {m:.1f} | {s:.2f} | '
            f'{max(share_c, share_b):.2f} ({bound}) | {tr / t:.1f} |')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    ap.add_argument('--n', type=int, default=10 ** 7)
    ap.add_argument('--nf', type=int, default=10 ** 6)
    a = ap.parse_args()
    lines = ['| op | dtype | D | matrices | Gmat/s | mean degree m | mean squarings s | share of bound | x matrix_exp |',
             '|---|---|---|---|---|---|---|---|---|']
    gen = torch.Generator(device='cuda').manual_seed(0)
    for dtype in (torch.float32, torch.float64):
        for D in (2, 3, 4, 6, 8):
            if D > N.lie.FORWARD_MAX[dtype]:
                continue
            n = a.n
            x = (torch.randn(n, D, D, device='cuda', generator=gen, dtype=torch.float64) * 0.3).to(dtype)
            m, s = degree_and_squarings(x[:2000].cpu())
            el = x.element_size()
            fl = 2 * D ** 3 * (m + s)
            r = row('expm', dtype, D, n, lambda: N.lie.expm(x), lambda: torch.linalg.matrix_exp(x), fl,
                    2 * D * D * el, m, s)
            print(r, flush=True)
            lines.append(r)
            del x
            torch.cuda.empty_cache()
        # Frechet over the 12-matrix affine basis: one launch over (n, F), X at stride 0 along F
        D, F, n = 4, 12, a.nf
        B = torch.zeros(F, D, D, dtype=dtype, device='cuda')
        for k in range(F):
            B[k, k // 4, k % 4] = 1
        p = (torch.randn(n, F, device='cuda', generator=gen, dtype=torch.float64) * 0.3).to(dtype)
        M = torch.einsum('nf,fij->nij', p, B).unsqueeze(-3)
        m, s = degree_and_squarings(M[:2000, 0].cpu())
        m = m + 1                                # the L kernel runs one degree past the exponential's
        el = p.element_size()
        fl = F * (3 * 2 * D ** 3 * m + 6 * D ** 3 * s)
        bl = (D * D + F * D * D) * el
        r = row('frechet L(X, B_f), F = 12', dtype, D, n * F, lambda: N.lie._frechet(M, B, None, 10000, 1e-32),
                lambda: N.lie._frechet_torch(M, B), fl / F, bl / F, m, s)
        print(r, flush=True)
        lines.append(r)
        del p, M
        torch.cuda.empty_cache()
    if a.md:
        with open(a.md, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
