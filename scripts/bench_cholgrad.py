#!/usr/bin/env python
"""Forward + backward of the differentiable Cholesky factor (nfm_symchol.hip + nfm_cholgrad.hip)
-> profiles/cholgrad_table.md.

2^22 compact SPD records at 3 x 3 and 6 x 6 float32 and 2^20 at 8 x 8 float64, contiguous.  Per row: the time of one
forward call with requires_grad plus its gradients for a given cotangent (`torch.autograd.grad`), records/s, the
share of the HBM roofline (8 TB/s) on the algorithmic bytes of the two passes, registers and waves per SIMD of the
contiguous-records backward kernel from the census (--census: the json of scripts/kernel_resources.py on
nfm_cholgrad_*.o), and the ratio to the same call routed through the torch composition `_symchol` on the device (what
the library ran for these calls before it had the backward kernels).  The composition is timed on 2^18 records (it
keeps full N x N matrices for autograd) and compared per record.  A ratio above 1 means the kernels are faster.
Algorithmic elements per record, K = N (N + 1) / 2:
  * sym_chol             forward K + K, backward K + K + K
  * sym_chol_apply       forward K + N + N, backward K + N + N + (K + N)
Steady-state medians by HIP events (scripts/_timing.py), one run.

    python scripts/bench_cholgrad.py [--md out.md] [--census census.json]"""
import argparse
import json
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timeit  # noqa: E402
from nitorch_fastmath_amd import sym as S, _symchol as Y  # noqa: E402

BW = 8.0e12
SIZES = ((3, 1 << 22, torch.float32), (6, 1 << 22, torch.float32), (8, 1 << 20, torch.float64))
N_TORCH = 1 << 18


def records(n, N, dtype):
    g = torch.randn(n, N, N, dtype=dtype, device='cuda')
    a = g @ g.transpose(-1, -2) / N + torch.eye(N, dtype=dtype, device='cuda')
    r = list(range(N)) + [i for i in range(N) for j in range(i + 1, N)]
    c = list(range(N)) + [j for i in range(N) for j in range(i + 1, N)]
    return a[:, r, c].contiguous()


def census_of(path):
    if not path or not os.path.exists(path):
        return {}
    return {k['kernel']: k for k in json.load(open(path))['kernels']}


def resources(census, apply, dtype, N):
    pat = ('CholApplyGradOp<{t}, {N}>' if apply else 'CholFactorGradOp<{t}, {N}>').format(
        t='float' if dtype == torch.float32 else 'double', N=N)
    rows = [k for name, k in census.items() if pat in name and name.endswith(', 1>')]      # the contiguous form
    if not rows:
        return 'not measured', 'not measured'
    return f"{rows[0]['vgpr']} + {rows[0]['agpr']}", str(rows[0]['waves_per_simd'])


def both_passes(f, g, *leaves):
    leaves = [t.clone().requires_grad_(True) for t in leaves]
    return lambda: torch.autograd.grad(f(*leaves), leaves, g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--census', default=None)
    args = ap.parse_args()
    census = census_of(args.census)
    out = ['# The differentiable Cholesky factor: forward + backward on MI355X (scripts/bench_cholgrad.py)', '',
           'Contiguous compact records, one forward call with requires_grad and its gradients for a given cotangent, '
           'steady-state medians by device events, one run: the spread between runs was not measured.  `x composition`: '
           f'the time per record of the same call through the torch composition `_symchol` ({N_TORCH} records) over the '
           'time per record of the kernels; above 1 the kernels are faster.  VGPR (+ AGPR) / waves per SIMD: the '
           'contiguous-records backward kernel.', '',
           '| call | dtype | N | records | ms | 1e9 records/s | HBM roofline share | VGPR + AGPR | waves/SIMD | x composition |',
           '|---|---|---|---|---|---|---|---|---|---|']
    slower = []
    for N, n, dtype in SIZES:
        x = records(n, N, dtype)
        K, es = x.shape[-1], x.element_size()
        v = torch.randn(n, N, dtype=dtype, device='cuda')
        fac = S.sym_chol(x)
        gK = torch.randn(n, K, dtype=dtype, device='cuda')
        gN = torch.randn(n, N, dtype=dtype, device='cuda')
        m = N_TORCH
        rows = [('sym_chol', False, 5 * K, both_passes(lambda a: S.sym_chol(a), gK, x),
                 both_passes(lambda a: Y.chol(a), gK[:m], x[:m]))]
        for op in ('L', 'Linv'):
            for factored in (False, True):
                mat = fac if factored else x
                rows.append((f"sym_chol_apply '{op}'" + (' factored' if factored else ''), True, 3 * K + 5 * N,
                             both_passes(lambda a, b, op=op, f=factored: S.sym_chol_apply(a, b, op, factored=f), gN, mat, v),
                             both_passes(lambda a, b, op=op, f=factored: Y.chol_apply(a, b, op, factored=f), gN[:m],
                                         mat[:m], v[:m])))
        for name, apply, elems, call, comp in rows:
            t = timeit(call)
            tc = timeit(comp, reps=3, settle_ms=0.0) * (n / m)
            vg, wv = resources(census, apply, dtype, N)
            if tc < t:
                slower.append(f'{name} {str(dtype)[6:]} N={N}: {tc / t:.2f}x the composition')
            out.append(f'| {name} | {str(dtype)[6:]} | {N} | {n} | {t * 1e3:.3f} | {n / t * 1e-9:.3f} | '
                       f'{elems * es * n / t / BW:.3f} | {vg} | {wv} | {tc / t:.1f} |')
            print(out[-1], flush=True)
        del x, v, fac, gK, gN, rows
    out += ['', '## Known weak spots', '',
            'Cases slower than the composition: ' + ('; '.join(slower) if slower else 'none') + '.']
    text = '\n'.join(out) + '\n'
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
