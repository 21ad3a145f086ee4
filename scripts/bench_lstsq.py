#!/usr/bin/env python
"""Throughput of tall `sugar.lmdiv` (nfm_lstsq.hip: more than 8 rows, at most 8 columns) against what the same
call cost before the kernel existed, `torch.linalg.pinv(a, rcond) @ b`, and against `torch.linalg.lstsq(a, b)`,
on the same device in the same run.

Cases: (M, N, K) in (16,3,1) (32,6,1) (64,7,1) (64,7,4) (256,8,1); float32 and float64; 2^20 records (2^18 at
M = 256); batch-major (n, M, N) and channel-first ((M, N, n) storage) operands.  Per row: time (median of
event-timed launches after a settle phase, scripts/_timing.py), baseline time / our time for both baselines, and
the algorithmic bytes (M (N + K) + N K) sizeof(T) per record over that time as a fraction of the copy ceiling --
the rate of a device-to-device copy of 1 GiB measured first in the same run (bytes read + bytes written).
The baselines are batched LAPACK-style factorisations that take seconds at 2^20 records: `--base-log2n` times them
on the first 2^b records (one warm-up, median of three) and the table scales that time by the ratio of the record
counts, and says so; with `--base-log2n 0` (the default) they run at the full count.

    python scripts/bench_lstsq.py [--md profiles/lstsq_table.md] [--log2n 20] [--base-log2n 16]"""
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
CASES = ((16, 3, 1), (32, 6, 1), (64, 7, 1), (64, 7, 4), (256, 8, 1))


def copy_ceiling(dev):
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    t = timeit(lambda: dst.copy_(src))
    return 2.0 * src.numel() * 4 / t


def time_base(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return sorted(ts)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    ap.add_argument('--log2n', type=int, default=20)
    ap.add_argument('--base-log2n', type=int, default=0)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    ceil = copy_ceiling(dev)
    head = [f'Copy ceiling measured in this run: {ceil / 1e12:.2f} TB/s (device-to-device copy of 1 GiB, read + write).',
            '']
    if args.base_log2n:
        head += [f'Baselines timed on the first 2^{args.base_log2n} records and scaled to the record count of the row.', '']
    lines = head + ['| M | N | K | dtype | layout | log2 n | ms | of the copy ceiling | pinv @ b ms | x pinv @ b | lstsq ms | x lstsq |',
                    '|---|---|---|---|---|---|---|---|---|---|---|---|']
    print('\n'.join(lines), flush=True)
    gen = torch.Generator(device='cuda').manual_seed(0)
    for M, N, K in CASES:
        log2n = args.log2n - 2 if M >= 256 else args.log2n
        n = 1 << log2n
        nb = min(n, 1 << args.base_log2n) if args.base_log2n else n
        for dtype in (torch.float32, torch.float64):
            es = 4 if dtype == torch.float32 else 8
            a = torch.randn(n, M, N, dtype=dtype, device=dev, generator=gen)
            b = torch.randn(n, M, K, dtype=dtype, device=dev, generator=gen)
            with torch.no_grad():
                tp = time_base(lambda: torch.linalg.pinv(a[:nb], rcond=1e-15) @ b[:nb]) * (n / nb)
                tl = time_base(lambda: torch.linalg.lstsq(a[:nb], b[:nb]).solution) * (n / nb)
            torch.cuda.empty_cache()
            for layout in ('batch-major', 'channel-first'):
                if layout == 'channel-first':
                    a, b = (x.permute(1, 2, 0).contiguous().movedim(-1, 0) for x in (a, b))
                with torch.no_grad():
                    t = timeit(lambda: S.lmdiv(a, b))
                r = (f'| {M} | {N} | {K} | {str(dtype)[6:]} | {layout} | {log2n} | {t * 1e3:.3f} | '
                     f'{(M * (N + K) + N * K) * es * n / t / ceil:.3f} | {tp * 1e3:.1f} | {tp / t:.1f} | '
                     f'{tl * 1e3:.1f} | {tl / t:.1f} |')
                print(r, flush=True)
                lines.append(r)
            del a, b
            torch.cuda.empty_cache()
    if args.md:
        open(args.md, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
