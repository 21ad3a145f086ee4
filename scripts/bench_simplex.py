#!/usr/bin/env python
"""Throughput of the simplex functions (nfm_simplex.hip) against what a user has without them: torch.softmax /
torch.log_softmax / torch.logsumexp, with a zero channel concatenated in front for an implicit input.

float32 fields of 2^27 voxels-times-classes (512 MiB, twice the Infinity Cache), K in {2, 4, 8, 16, 32},
channel-first `(K, N)` and class-last `(N, K)`; explicit, implicit `(True, False)` (the baseline pays the `cat`) and
implicit `(True, True)` (the baseline pays the `cat` and a slice copy of the K kept classes).  Per row: time
(median of event-timed launches after a settle phase, scripts/_timing.py), the bytes that MUST move (one read
of each input, one write of each output) over that time as a share of 8 TB/s, and baseline time / our time.
Backward rows time `torch.autograd.grad` alone on a retained graph, for both sides.

    python scripts/bench_simplex.py [--md out.md] [--log2n 27]"""
import argparse
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timeit  # noqa: E402
import nitorch_fastmath_amd as N  # noqa: E402

S = N.simplex
BW = 8.0e12


def baseline(fn, x, dim, implicit):
    """the same result from stock torch ops (the implicit class first); implicit: False, 'in' or 'both'"""
    K = x.shape[dim]

    def kept(t):          # the slice copy that drops the implicit class again
        return t.narrow(dim, 1, K).contiguous() if implicit == 'both' else t

    if fn == 'logit':
        if implicit:
            rest = (1 - x.sum(dim, keepdim=True)).clamp_min(1e-8).log()
            return x.log() - rest if implicit == 'both' else torch.cat([torch.zeros_like(rest), x.log() - rest], dim)
        lg = x.log()
        return lg - lg.narrow(dim, 0, 1)
    z = torch.cat([torch.zeros_like(x.narrow(dim, 0, 1)), x], dim) if implicit else x
    if fn == 'softmax':
        return kept(torch.softmax(z, dim))
    if fn == 'log_softmax':
        return kept(torch.log_softmax(z, dim))
    if fn == 'logsumexp':
        return torch.logsumexp(z, dim, keepdim=True)
    return kept(torch.softmax(z, dim)), torch.logsumexp(z, dim).sum(dtype=torch.float64)


def ours(fn, x, dim, implicit):
    imp = {False: False, 'in': (True, False), 'both': (True, True)}[implicit]
    if fn == 'logsumexp':
        return S.logsumexp(x, dim, True, bool(implicit))
    if fn == 'softmax_lse':
        return S.softmax_lse(x, dim, None, imp)
    return getattr(S, fn)(x, dim, imp, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    ap.add_argument('--log2n', type=int, default=27)
    a = ap.parse_args()
    lines = ['| function | pass | K | layout | implicit | ms | must-move MiB | share of 8 TB/s | x torch |',
             '|---|---|---|---|---|---|---|---|---|']
    gen = torch.Generator(device='cuda').manual_seed(0)
    total = 1 << a.log2n
    for K in (2, 4, 8, 16, 32):
        nvox = total // K
        for layout in ('channel-first', 'class-last'):
            shape, dim = ((K, nvox), 0) if layout == 'channel-first' else ((nvox, K), 1)
            x = torch.randn(shape, device='cuda', generator=gen) * 3
            prob = torch.softmax(x, dim) * 0.9
            for implicit in (False, 'in', 'both'):
                imp_name = {False: 'no', 'in': '(True, False)', 'both': '(True, True)'}[implicit]
                for fn in ('softmax', 'log_softmax', 'logsumexp', 'logit', 'softmax_lse'):
                    if fn == 'logsumexp' and implicit == 'both':
                        continue          # no output class to drop: the 'in' row
                    inp = prob if fn == 'logit' else x
                    with torch.no_grad():
                        y = ours(fn, inp, dim, implicit)
                        # outputs only: softmax_lse returns p and ONE float64 (its per-voxel lse is an intermediate)
                        nout = y[0].numel() + 2 if fn == 'softmax_lse' else y.numel()
                        del y
                        t = timeit(lambda: ours(fn, inp, dim, implicit))
                        tb = timeit(lambda: baseline(fn, inp, dim, implicit))
                    by = (inp.numel() + nout) * 4
                    r = (f'| {fn} | forward | {K} | {layout} | {imp_name} | {t * 1e3:.3f} | {by / 2 ** 20:.0f} | '
                         f'{by / t / BW:.2f} | {tb / t:.2f} |')
                    print(r, flush=True)
                    lines.append(r)
                    if fn in ('logit', 'softmax_lse'):
                        continue
                    xr = x.clone().requires_grad_()
                    y = ours(fn, xr, dim, implicit)
                    g = torch.randn_like(y)
                    t = timeit(lambda: torch.autograd.grad(y, xr, g, retain_graph=True))
                    saved = y.numel() if fn == 'softmax' else xr.numel()
                    by = (saved + g.numel() + xr.numel()) * 4
                    del y
                    yb = baseline(fn, xr, dim, implicit)
                    tb = timeit(lambda: torch.autograd.grad(yb, xr, g, retain_graph=True))
                    del yb, g, xr
                    r = (f'| {fn} | backward | {K} | {layout} | {imp_name} | {t * 1e3:.3f} | {by / 2 ** 20:.0f} | '
                         f'{by / t / BW:.2f} | {tb / t:.2f} |')
                    print(r, flush=True)
                    lines.append(r)
                    torch.cuda.empty_cache()
            del x, prob
            torch.cuda.empty_cache()
    if a.md:
        with open(a.md, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
