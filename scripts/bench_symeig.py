#!/usr/bin/env python
"""Throughput of sym.sym_eigvals / sym.sym_eigh and of their gradient (nfm_symeig.hip) -> profiles/symeig_table.md.

2^22 compact symmetric records at 3 x 3 and 6 x 6, 2^20 at 8 x 8, both dtypes, contiguous records; the four ops:
values, vectors, the gradient for a cotangent of the values, the gradient for cotangents of values and vectors.
Per row: records/s, the share of the HBM roofline (8 TB/s) on the algorithmic bytes (K in + N out; K in + N + N^2 out;
K + N in + K out; K + N + N^2 in + K out elements per record, K = N (N + 1) / 2), registers and waves per SIMD of the
contiguous-records kernel from the census (--census: the json of scripts/kernel_resources.py on nfm_symeig_*.o), and
the ratio to
  * the composition the functions replace: sym_to_full -> qr.eig_sym(arithmetic='fast') -> sort and gather in torch;
    its backward is autograd through that chain (EigSymFn);
  * torch.linalg.eigvalsh / eigh of the expanded field (built outside the timed region), forward only, on 2^14
    records (minutes at the full size) and compared per record.
A ratio above 1 means the new function is faster.  Steady-state medians by HIP events (scripts/_timing.py).

    python scripts/bench_symeig.py [--md out.md] [--census census.json]"""
import argparse
import json
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timeit  # noqa: E402
from nitorch_fastmath_amd import qr as Q, sym as S  # noqa: E402

BW = 8.0e12
SIZES = ((3, 1 << 22), (6, 1 << 22), (8, 1 << 20))
N_TORCH = 1 << 14
OPS = ('values', 'vectors', 'values backward', 'backward')
OP_KERNEL = {'values': 'SymEigOp<{t}, {N}, false>', 'vectors': 'SymEigOp<{t}, {N}, true>',
             'values backward': 'SymEigValBwdOp<{t}, {N}>', 'backward': 'SymEigBwdOp<{t}, {N}>'}


def records(n, N, dtype):
    a = torch.randn(n, N, N, dtype=dtype, device='cuda')
    a = a + a.transpose(-1, -2)
    r = list(range(N)) + [i for i in range(N) for j in range(i + 1, N)]
    c = list(range(N)) + [j for i in range(N) for j in range(i + 1, N)]
    return a[:, r, c].contiguous()


def composition(x, vectors):
    full = S.sym_to_full(x)
    if not vectors:
        return Q.eig_sym(full, arithmetic='fast', check_finite=False).sort(-1).values
    vals, vecs = Q.eig_sym(full, compute_u=True, arithmetic='fast', check_finite=False)
    vals, idx = vals.sort(-1)
    return vals, vecs.gather(-1, idx[..., None, :].expand(vecs.shape))


def census_of(path):
    if not path or not os.path.exists(path):
        return {}
    return {k['kernel']: k for k in json.load(open(path))['kernels']}


def resources(census, op, dtype, N):
    pat = OP_KERNEL[op].format(t='float' if dtype == torch.float32 else 'double', N=N)
    rows = [k for name, k in census.items() if pat in name]
    if not rows:
        return 'not measured', 'not measured'
    k = max(rows, key=lambda k: k['vgpr'] or 0)                  # the widest of the layout forms
    # the code object's vgpr_count is the unified total (accumulation registers included): 512 per SIMD lane
    return str(k['vgpr']), str(min(8, 512 // (-(-max(k['vgpr'], 1) // 8) * 8)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--census', default=None)
    args = ap.parse_args()
    census = census_of(args.census)
    out = ['# sym_eigvals / sym_eigh: speed on MI355X (scripts/bench_symeig.py)', '',
           'Contiguous compact records (2^22 at N = 3, 6; 2^20 at N = 8), steady-state medians.  `x composition`: time of '
           "sym_to_full -> qr.eig_sym(arithmetic='fast') -> sort / gather in torch (backward: autograd through it) over "
           f'the time of the new function; `x torch`: the same per record for torch.linalg.eigvalsh / eigh on {N_TORCH} '
           'expanded records.  VGPR / waves per SIMD: the widest layout form of the kernel.', '',
           '| op | dtype | N | records | 1e9 records/s | HBM roofline share | VGPR | waves/SIMD | x composition | x torch |',
           '|---|---|---|---|---|---|---|---|---|---|']
    slower = []
    for dtype in (torch.float32, torch.float64):
        for N, n in SIZES:
            x = records(n, N, dtype)
            K, es = x.shape[-1], x.element_size()
            gl = torch.randn(n, N, dtype=dtype, device='cuda')
            gv = torch.randn(n, N, N, dtype=dtype, device='cuda')
            full_small = S.sym_to_full(x[:N_TORCH])
            t_torch = {'values': timeit(lambda: torch.linalg.eigvalsh(full_small), reps=3) / N_TORCH,
                       'vectors': timeit(lambda: torch.linalg.eigh(full_small), reps=3) / N_TORCH}
            del full_small
            t_comp = {'values': timeit(lambda: composition(x, False), reps=5),
                      'vectors': timeit(lambda: composition(x, True), reps=5)}
            xr = x.clone().requires_grad_(True)
            yr = composition(xr, False)
            t_comp['values backward'] = timeit(lambda: torch.autograd.grad(yr, xr, gl, retain_graph=True), reps=5)
            del yr
            yr = composition(xr, True)
            t_comp['backward'] = timeit(lambda: torch.autograd.grad(yr, xr, (gl, gv), retain_graph=True), reps=5)
            del yr, xr
            elems = {'values': K + N, 'vectors': K + N + N * N, 'values backward': 2 * K + N,
                     'backward': 2 * K + N + N * N}
            calls = {'values': lambda: S.sym_eigvals(x), 'vectors': lambda: S.sym_eigh(x),
                     'values backward': lambda: S._eigh_backward(x, gl, None, 0, None),
                     'backward': lambda: S._eigh_backward(x, gl, gv, 0, None)}
            for k, op in enumerate(OPS):
                route = '' if N <= S._eigh_cap(dtype, k) else ' (split route)'
                t = timeit(calls[op])
                vg, wv = resources(census, op, dtype, N) if not route else ('-', '-')
                xt = f'{t_torch[op] * n / t:.1f}' if op in t_torch else '-'
                out.append(f'| {op}{route} | {str(dtype)[6:]} | {N} | {n} | {n / t * 1e-9:.3f} | '
                           f'{elems[op] * es * n / t / BW:.3f} | {vg} | {wv} | {t_comp[op] / t:.1f} | {xt} |')
                print(out[-1], flush=True)
                if t_comp[op] < t:
                    slower.append(f'{op}{route} {str(dtype)[6:]} N={N}: {t_comp[op] / t:.2f}x the composition '
                                  f'({n / t * 1e-9:.3f}e9 records/s)')
            del x, gl, gv
    out += ['', '## Known weak spots', '',
            'Cases slower than the composition (listed, not routed away): ' + ('; '.join(slower) if slower else 'none') + '.']
    text = '\n'.join(out) + '\n'
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
