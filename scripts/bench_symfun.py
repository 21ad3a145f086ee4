#!/usr/bin/env python
"""Throughput of sym.sym_funm and of its gradient (nfm_symfun.hip) -> the speed part of profiles/symfun_table.md.

N in {3, 6, 8}, both dtypes, log and rsqrt, forward and backward, 2^22 compact SPD records, contiguous and
channel-first.  Per row: records/s, the share of the HBM roofline (8 TB/s) on the algorithmic bytes -- 2 K
elements per record forward, 3 K backward, K = N (N + 1) / 2 -- and the ratio to
  * the composition the function replaces, on contiguous records: sym_to_full -> eig_sym(compute_u=True,
    arithmetic='fast') -> V f(L) V^T in torch -> pack; its backward is torch's autograd through that chain;
  * logm.logm on the dense matrix (for log, forward, where it has a kernel); the dense matrix is built outside
    the timed region.
A ratio above 1 means sym_funm is faster.

    python scripts/bench_symfun.py [--md out.md] [--n 4194304]"""
import argparse
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timeit  # noqa: E402
from nitorch_fastmath_amd import _lib, logm as LM, qr as Q, sym as S  # noqa: E402

BW = 8.0e12


def spd(n, N, dtype):
    g = torch.randn(n, N, N, dtype=dtype, device='cuda')
    a = g @ g.transpose(-1, -2) / N + torch.eye(N, dtype=dtype, device='cuda')
    r = list(range(N)) + [i for i in range(N) for j in range(i + 1, N)]
    c = list(range(N)) + [j for i in range(N) for j in range(i + 1, N)]
    return a[:, r, c].contiguous(), (torch.as_tensor(r, device='cuda'), torch.as_tensor(c, device='cuda'))


def composition(x, fn, rc):
    full = S.sym_to_full(x)
    vals, vecs = Q.eig_sym(full, compute_u=True, arithmetic='fast', check_finite=False)
    f = vals.log() if fn == 'log' else vals.rsqrt()
    y = (vecs * f[..., None, :]) @ vecs.transpose(-1, -2)
    return y[:, rc[0], rc[1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--n', type=int, default=1 << 22)
    args = ap.parse_args()
    n = args.n
    out = ['## Speed (scripts/bench_symfun.py)', '',
           f'{n} compact SPD records per row, steady-state medians.  `x composition`: time of sym_to_full -> eig_sym '
           "(vectors, arithmetic='fast') -> torch products -> pack (backward: autograd through it) over the time of "
           'sym_funm, contiguous records; `x logm`: the same for logm.logm on the dense matrix.', '',
           '| fn | dtype | N | direction | layout | 1e9 records/s | HBM roofline share | x composition | x logm |',
           '|---|---|---|---|---|---|---|---|---|']
    slower = []
    for dtype in (torch.float32, torch.float64):
        for N in (3, 6, 8):
            x, rc = spd(n, N, dtype)
            g = torch.randn_like(x)
            K = x.shape[-1]
            xs, gs = x.t().contiguous().t(), g.t().contiguous().t()
            full = S.sym_to_full(x)
            for fn in ('log', 'rsqrt'):
                code = _lib.FUN[fn]
                t_comp = timeit(lambda: composition(x, fn, rc), reps=5)
                xr = x.clone().requires_grad_(True)
                yr = composition(xr, fn, rc)
                t_comp_b = timeit(lambda: torch.autograd.grad(yr, xr, g, retain_graph=True), reps=5)
                del yr, xr
                t_logm = timeit(lambda: LM.logm(full), reps=5) if (fn == 'log' and N <= LM.FORWARD_MAX[dtype]) else None
                for direction in ('forward', 'backward'):
                    kernel = N <= S._funm_cap(dtype, direction == 'backward')
                    for layout, xx, gg in (('contiguous', x, g), ('channel-first', xs, gs)):
                        if not kernel:      # above the cap: torch.linalg.eigh, minutes at this batch size -- not timed
                            out.append(f'| {fn} | {str(dtype)[6:]} | {N} | {direction} (torch route) | {layout} | '
                                       'not timed | - | - | - |')
                            continue
                        if direction == 'forward':
                            t = timeit(lambda: S.sym_funm(xx, fn))
                        else:
                            t = timeit(lambda: S._funm_backward(xx, gg, code, 0.0, None, None))
                        byts = (2 if direction == 'forward' else 3) * K * x.element_size() * n
                        base = t_comp if direction == 'forward' else t_comp_b
                        rl = f'{t_logm / t:.1f}' if (t_logm and direction == 'forward') else '-'
                        out.append(f'| {fn} | {str(dtype)[6:]} | {N} | {direction} | '
                                   f'{layout} | {n / t * 1e-9:.3f} | {byts / t / BW:.3f} | {base / t:.1f} | {rl} |')
                        print(out[-1], flush=True)
                        if layout == 'contiguous' and kernel and base < t:
                            slower.append(f'{fn} {str(dtype)[6:]} N={N} {direction}: {base / t:.2f}x the composition')
            del x, g, xs, gs, full
    out += ['', 'Cases slower than the composition: ' + ('; '.join(slower) if slower else 'none') + '.']
    text = '\n'.join(out) + '\n'
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
