#!/usr/bin/env python
"""Throughput of `sugar.lmdiv(method='svd' / 'pinv')` and of non-square `lmdiv` (nfm_svd.hip) against the route
the same call took before the kernel existed: the reference's torch composition on the same device
(`torch.svd` + two matmuls for 'svd', `torch.linalg.pinv(a, rcond) @ b` for 'pinv' and every non-square system).

Cases: (M, N, K) in (3,3,1) (4,4,3) (8,8,3) (8,3,1) (3,8,1); float32 and float64; both methods (non-square
systems take 'pinv' whatever the method, so they have one row).  2^20 records, contiguous.  Per row: time (median
of event-timed launches after a settle phase, scripts/_timing.py), the algorithmic bytes (M N + M K + N K)
sizeof(T) per record over that time as a share of 8 TB/s, and baseline time / our time.  The baseline runs on the
same tensors.

    python scripts/bench_svd.py [--md profiles/svd_table.md] [--log2n 20]"""
import argparse
import os
import sys
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import timeit  # noqa: E402
import nitorch_fastmath_amd as N_  # noqa: E402

S = N_.sugar
BW = 8.0e12
CASES = ((3, 3, 1), (4, 4, 3), (8, 8, 3), (8, 3, 1), (3, 8, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    ap.add_argument('--log2n', type=int, default=20)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    n = 1 << args.log2n
    lines = ['| method | M | N | K | dtype | log2 n | ms | share of 8 TB/s | x torch route |', '|---|---|---|---|---|---|---|---|---|']
    gen = torch.Generator(device='cuda').manual_seed(0)
    for M, N, K in CASES:
        for dtype in (torch.float32, torch.float64):
            es = 4 if dtype == torch.float32 else 8
            a = torch.randn(n, M, N, dtype=dtype, device=dev, generator=gen)
            if M == N:
                a = a + 4 * torch.eye(N, dtype=dtype, device=dev)
            b = torch.randn(n, M, K, dtype=dtype, device=dev, generator=gen)
            for method in (('svd', 'pinv') if M == N else ('pinv',)):
                with torch.no_grad():
                    t = timeit(lambda: S.lmdiv(a, b, method))
                    tb = timeit(lambda: S._torch_lmdiv(a, b, method, 1e-15, None), reps=3, settle_ms=10.0)
                r = (f'| {method} | {M} | {N} | {K} | {str(dtype)[6:]} | {args.log2n} | {t * 1e3:.3f} | '
                     f'{(M * N + M * K + N * K) * es * n / t / BW:.3f} | {tb / t:.1f} |')
                print(r, flush=True)
                lines.append(r)
            del a, b
            torch.cuda.empty_cache()
    if args.md:
        open(args.md, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
