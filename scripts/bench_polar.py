#!/usr/bin/env python
"""Throughput of batched.batchsvdvals / batchsvd / batchpolar and of the polar backward (nfm_polar.hip) ->
profiles/polar_table.md: the registers of every instantiation (scripts/kernel_resources.py on the library) and the
speed table.

2^20 records at n in {2, 3, 4, 6, 8}, both dtypes, contiguous and channel-first.  Per row: records/s, the share of
the HBM roofline (8 TB/s) on the bytes read and written, and the ratio to the torch composition the call would
otherwise take, on the same device in the same run: torch.linalg.svdvals; torch.linalg.svd; U @ Vh and Vh^T S Vh from
it; and autograd through that with both cotangents.  A ratio above 1 means the kernel is faster.  The torch
composition is timed on contiguous records (a channel-first operand would first be copied).  torch's batched SVD of
tiny matrices is slow: when a probe at 2^12 records predicts more than `--torch-budget` seconds for one call at the
full batch, the composition is timed at the largest power-of-two batch inside the budget and scaled linearly to 2^20
(marked ~); its time per record does not fall with the batch.

    python scripts/bench_polar.py [--md out.md] [--n 1048576] [--torch-budget 2.0]"""
import argparse
import os
import sys
import time
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
sys.path.insert(0, ROOT)
from _timing import timeit  # noqa: E402
import kernel_resources as KR  # noqa: E402
from nitorch_fastmath_amd import batched as B  # noqa: E402

BW = 8.0e12
OPS = ('svdvals', 'svd', 'polar', 'polar_backward')


def torch_call(op, a, gr, gp):
    if op == 'svdvals':
        return lambda: torch.linalg.svdvals(a)
    if op == 'svd':
        return lambda: torch.linalg.svd(a)

    def polar(x):
        U, S, Vh = torch.linalg.svd(x)
        return U @ Vh, (Vh.transpose(-1, -2) * S[..., None, :]) @ Vh
    if op == 'polar':
        return lambda: polar(a)

    def backward():
        x = a.detach().requires_grad_()
        return torch.autograd.grad(list(polar(x)), x, [gr, gp])
    return backward


def wall(fn, reps=3):
    """a slow call: one warm-up, then the median of `reps` synchronised wall times"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def torch_time(op, a, gr, gp, n, budget):
    """(seconds for n records, extrapolated?)"""
    m = min(n, 1 << 12)
    t = wall(torch_call(op, a[:m], gr[:m], gp[:m]))
    full = t * n / m
    if full <= budget:
        m2 = n
    else:
        m2 = m
        while m2 * 2 <= n and t * (m2 * 2) / m <= budget:
            m2 *= 2
    if m2 == m:
        return full, n != m
    t2 = wall(torch_call(op, a[:m2], gr[:m2], gp[:m2]))
    return t2 * n / m2, m2 != n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--n', type=int, default=1 << 20)
    ap.add_argument('--torch-budget', type=float, default=2.0)
    args = ap.parse_args()
    n = args.n
    rows = [k for k in KR.collect([os.path.join(ROOT, 'nitorch_fastmath_amd', 'libnfm_hip.so')])
            if any(s in k['kernel'] for s in ('SvdValsOp', 'SvdFullOp', 'PolarOp', 'PolarBwdOp'))]
    out = ['# batchsvdvals / batchsvd / batchpolar: registers and speed (scripts/bench_polar.py)', '',
           '## Registers (scripts/kernel_resources.py on libnfm_hip.so)', '',
           'Layout kind of `rec_kernel`: 0 run-time modes, 1 contiguous, 2 channel-first, 3 channel-first with 512-lane tiles.',
           '', '| kernel | VGPR | SGPR | scratch B/lane | waves/SIMD |', '|---|---|---|---|---|']
    for k in sorted(rows, key=lambda k: k['kernel']):
        out.append(f"| `{k['kernel']}` | {k['vgpr']} | {k['sgpr']} | {k['scratch']} | {k['waves_per_simd']} |")
    out += ['', '## Speed', '',
            f'{n} records per row, steady-state medians.  `x torch`: time of the torch composition on the same device in the '
            'same run over the time of the call (~: the composition was timed on a smaller batch and scaled, see the script).  '
            '`route`: what the facade runs (kernel; svd kernel + torch: the SVD kernel and torch products above the cap of '
            'the polar kernels).', '',
            '| function | dtype | n | layout | route | 1e6 records/s | HBM roofline share | x torch |', '|---|---|---|---|---|---|---|---|']
    slower = []
    for dtype in (torch.float32, torch.float64):
        for N in (2, 3, 4, 6, 8):
            a = torch.randn(n, N, N, dtype=dtype, device='cuda')
            gr, gp = torch.randn_like(a), torch.randn_like(a)
            cf = lambda x: x.permute(1, 2, 0).contiguous().permute(2, 0, 1)          # noqa: E731
            lay = (('contiguous', a, gr, gp), ('channel-first', cf(a), cf(gr), cf(gp)))
            for op in OPS:
                tt, approx = torch_time(op, a, gr, gp, n, args.torch_budget)
                kernel = N <= B.polar_max_order(dtype, op)
                for layout, x, g1, g2 in lay:
                    call = {'svdvals': lambda: B.batchsvdvals(x), 'svd': lambda: B.batchsvd(x),
                            'polar': lambda: B.batchpolar(x), 'polar_backward': lambda: B._polar_backward(x, g1, g2)}[op]
                    t = timeit(call)
                    vals = {'svdvals': N * N + N, 'svd': 2 * N + 3 * N * N, 'polar': 3 * N * N, 'polar_backward': 4 * N * N}[op]
                    share = f'{vals * a.element_size() * n / t / BW:.3f}' if kernel else '-'
                    out.append(f"| {op} | {str(dtype)[6:]} | {N} | {layout} | {'kernel' if kernel else 'svd kernel + torch'} | "
                               f"{n / t * 1e-6:.1f} | {share} | {'~' if approx else ''}{tt / t:.1f} |")
                    print(out[-1], flush=True)
                    if tt < t:
                        slower.append(f'{op} {str(dtype)[6:]} n={N} {layout}: {tt / t:.2f}x torch')
            del a, gr, gp, lay
    out += ['', 'Cases slower than the torch composition (routed back to it in the facade): ' +
            ('; '.join(slower) if slower else 'none') + '.']
    text = '\n'.join(out) + '\n'
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
