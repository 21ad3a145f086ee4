#!/usr/bin/env python
"""Throughput of the special functions (nfm_special.hip) against what a user has from stock torch without them:
`torch.special.i0e` / `i1e` compositions for besseli at nu in {0, 1} and for the ratio at nu = 0, the
`torch.digamma` loop for mvdigamma.  besseli at any other nu has no stock counterpart: roofline column only.

2^27 elements (512 MiB in float32, twice the Infinity Cache), float32 and float64.  besseli rows confine z below
the 15/4 split, above it, and mix both sides within every wave; the general orders confine z to the series
range, to the asymptotic range, and mix them.  Per row: time (median of event-timed launches after a settle
phase, scripts/_timing.py), one read + one write per element over that time as a share of 8 TB/s, and
baseline time / our time.  Backward rows time `torch.autograd.grad` alone on a retained graph.

    python scripts/bench_special.py [--md out.md] [--log2n 27]"""
import argparse
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timeit  # noqa: E402
import nitorch_fastmath_amd as N  # noqa: E402

S = N.special
BW = 8.0e12
SP = torch.special


def stock_besseli(nu, z, mode):
    e = SP.i0e(z) if nu == 0 else SP.i1e(z)
    return e if mode == 'norm' else e.log() + z if mode == 'log' else e * z.exp()


def stock_digamma(x, order):
    dg = torch.digamma(x)
    for p in range(2, order + 1):
        dg += torch.digamma(x + (1 - p) / 2)
    return dg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    ap.add_argument('--log2n', type=int, default=27)
    a = ap.parse_args()
    lines = ['| function | pass | dtype | input | ms | share of 8 TB/s | x torch |', '|---|---|---|---|---|---|---|']
    n = 1 << a.log2n
    gen = torch.Generator(device='cuda').manual_seed(0)

    def row(name, pas, dtype, rng, t, nbytes, tb):
        r = (f'| {name} | {pas} | {str(dtype)[6:]} | {rng} | {t * 1e3:.3f} | {nbytes / t / BW:.3f} | '
             f'{"-" if tb is None else f"{tb / t:.2f}"} |')
        print(r, flush=True)
        lines.append(r)

    def bench(name, dtype, rng, x, ours, stock, backward=True):
        es = x.element_size()
        with torch.no_grad():
            t = timeit(lambda: ours(x))
            tb = timeit(lambda: stock(x)) if stock else None
        row(name, 'forward', dtype, rng, t, 2 * n * es, tb)
        if not backward:
            return
        xr = x.clone().requires_grad_()
        y = ours(xr)
        g = torch.ones_like(y)
        t = timeit(lambda: torch.autograd.grad(y, xr, g, retain_graph=True))
        saved = 2 if name.startswith('besseli') else 1       # besseli and the ratio save z and the output
        del y
        tb = None
        if stock:
            yb = stock(xr)
            tb = timeit(lambda: torch.autograd.grad(yb, xr, g, retain_graph=True))
            del yb
        row(name, 'backward', dtype, rng, t, (saved + 2) * n * es, tb)
        del xr, g
        torch.cuda.empty_cache()

    for dtype in (torch.float32, torch.float64):
        u = torch.rand(n, device='cuda', generator=gen, dtype=dtype)
        ranges = {'z < 15/4': u * 3.7 + 0.01, 'z > 15/4': u * 60 + 3.76, 'mixed in a wave': u * 7.4 + 0.01}
        for rng, z in ranges.items():
            for nu in (0, 1):
                for mode in (None, 'norm', 'log'):
                    bench(f'besseli({nu}, z, {mode!r})', dtype, rng, z, lambda t: S.besseli(nu, t, mode),
                          lambda t: stock_besseli(nu, t, mode), backward=(mode == 'log' and rng == 'mixed in a wave'))
        del ranges
        # general order: series below w = sqrt(nu^2 + z^2) = 12 (float32) / 40 (float64), uniform expansion above
        sw = 12.0 if dtype == torch.float32 else 40.0
        ranges = {'series': u * (0.9 * sw - 3) + 0.01, 'asymptotic': u * 200 + sw, 'mixed in a wave': u * 2 * sw + 0.01}
        for rng, z in ranges.items():
            for mode in (None, 'norm', 'log'):
                bench(f'besseli(2.5, z, {mode!r})', dtype, rng, z, lambda t: S.besseli(2.5, t, mode), None,
                      backward=(mode == 'log'))
        del ranges
        z = u * 60 + 0.01
        bench('besseli_ratio(0, X)', dtype, '(0, 60)', z, lambda t: S.besseli_ratio(0, t), lambda t: SP.i1e(t) / SP.i0e(t))
        bench('besseli_ratio(0, X, 8, 20)', dtype, '(0, 60)', z, lambda t: S.besseli_ratio(0, t, 8, 20), None, backward=False)
        bench('besseli_ratio(2.5, X, 0, 0)', dtype, '(0, 60)', z, lambda t: S.besseli_ratio(2.5, t, 0, 0), None, backward=False)
        x = u * 30 + 0.01
        for order in (1, 3, 6):
            bench(f'mvdigamma(x, {order})', dtype, '(0, 30) + (order - 1) / 2', x + (order - 1) / 2,
                  lambda t: S.mvdigamma(t, order), lambda t: stock_digamma(t, order), backward=(order == 3))
        del u, z, x
        torch.cuda.empty_cache()
    if a.md:
        with open(a.md, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
