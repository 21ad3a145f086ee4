#!/usr/bin/env python
"""Throughput of the Cholesky functions of `sym` (nfm_symchol.hip) -> profiles/symchol_table.md.

2^22 compact SPD records at 3 x 3 and 4 x 4, 2^20 at 6 x 6 and 8 x 8, both dtypes, contiguous records.  Per row:
records/s, the share of the HBM roofline (8 TB/s) on the algorithmic bytes (K = N (N + 1) / 2 values of the matrix, N of
a vector, the result), registers and waves per SIMD of the contiguous-records kernel from the census (--census: the
json of scripts/kernel_resources.py on nfm_symchol_*.o), and the ratio to the chain the function replaces:
  * sym_logdet          sym_det -> torch.log
  * sym_mahalanobis     sym_solve -> dot product
  * sym_gauss_logpdf    both of the above and the combination
  * sym_chol            sym_to_full -> torch.linalg.cholesky        (on 2^16 records, compared per record)
  * sym_chol_apply Linv sym_to_full -> cholesky -> solve_triangular (on 2^16 records, compared per record)
  * A^-1 v from a factor that is there ('Linv' then 'LTinv', factored=True)   torch.cholesky_solve on the full factor
    (on 2^16 records, per record; the factor is built outside the timed region on both sides)
  * the gradients: autograd through the chains above (sym_det -> log; sym_solve -> dot)
A ratio above 1 means the new function is faster.  The last rows time sym_solve itself, the yardstick of the
expectation "logpdf moves about the bytes of sym_solve and should land near its share of the roofline".
Steady-state medians by HIP events (scripts/_timing.py).

    python scripts/bench_symchol.py [--md out.md] [--census census.json]"""
import argparse
import json
import math
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _timing import timeit  # noqa: E402
from nitorch_fastmath_amd import sym as S  # noqa: E402

BW = 8.0e12
SIZES = ((3, 1 << 22), (4, 1 << 22), (6, 1 << 20), (8, 1 << 20))
N_TORCH = 1 << 16
KERNEL = {'sym_chol': 'CholFactorOp<{t}, {N}>', 'apply Linv': 'CholApplyOp<{t}, {N}>',
          'solve from factor': 'CholApplyOp<{t}, {N}>', 'sym_logdet': 'CholLogdetOp<{t}, {N}>',
          'sym_mahalanobis': 'CholQuadOp<{t}, {N}>', 'sym_gauss_logpdf': 'CholQuadOp<{t}, {N}>',
          'logdet backward': 'CholLogdetBwdOp<{t}, {N}>', 'mahalanobis backward': 'CholQuadBwdOp<{t}, {N}, false>',
          'logpdf backward': 'CholQuadBwdOp<{t}, {N}, true>'}


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


def resources(census, op, dtype, N):
    if op not in KERNEL:
        return '-', '-'
    pat = KERNEL[op].format(t='float' if dtype == torch.float32 else 'double', N=N)
    rows = [k for name, k in census.items() if pat in name and name.endswith(', 1>')]      # the contiguous form
    if not rows:
        return 'not measured', 'not measured'
    k = rows[0]
    return str(k['vgpr']), str(min(8, 512 // (-(-max(k['vgpr'], 1) // 8) * 8)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md', default=None)
    ap.add_argument('--census', default=None)
    args = ap.parse_args()
    census = census_of(args.census)
    out = ['# Cholesky functions of sym: speed on MI355X (scripts/bench_symchol.py)', '',
           'Contiguous compact records (2^22 at N = 3, 4; 2^20 at N = 6, 8), steady-state medians.  `x chain`: time of the '
           f'chain of existing calls the function replaces over the time of the function (chains through torch.linalg on '
           f'{N_TORCH} records, per record); `-`: no chain timed.  The chains of `apply Linv` and `solve from factor` are batched LAPACK-style torch calls on tiny systems (a launch-bound route nobody would choose for a field): their ratios say that such a route is no alternative, not how much a realistic one gains.  Call times by device events, one run: the spread between runs was not measured.  VGPR / waves per SIMD: the contiguous-records kernel.', '',
           '| op | dtype | N | records | 1e9 records/s | HBM roofline share | VGPR | waves/SIMD | chain | x chain |',
           '|---|---|---|---|---|---|---|---|---|---|']
    slower, shares = [], {}
    for dtype in (torch.float32, torch.float64):
        for N, n in SIZES:
            x = records(n, N, dtype)
            K, es = x.shape[-1], x.element_size()
            v = torch.randn(n, N, dtype=dtype, device='cuda')
            g = torch.randn(n, dtype=dtype, device='cuda')
            fac = S.sym_chol(x)
            c0 = N * math.log(2 * math.pi)
            xs, vs = x[:N_TORCH], v[:N_TORCH]
            full_l = torch.linalg.cholesky(S.sym_to_full(xs))
            per = n / N_TORCH

            def chain_grad(f, *leaves):
                leaves = [t.clone().requires_grad_(True) for t in leaves]
                try:
                    y = f(*leaves)
                except NotImplementedError:          # a chain that is not differentiable is not timed
                    return None
                return lambda: torch.autograd.grad(y, leaves, g, retain_graph=True)

            # (op, the call, algorithmic elements per record, chain name, the chain or None, chain scale)
            rows = [
                ('sym_chol', lambda: S.sym_chol(x), 2 * K, 'to_full + cholesky',
                 lambda: torch.linalg.cholesky(S.sym_to_full(xs)), per),
                ('apply Linv', lambda: S.sym_chol_apply(x, v, 'Linv'), K + 2 * N, 'to_full + cholesky + solve_triangular',
                 lambda: torch.linalg.solve_triangular(torch.linalg.cholesky(S.sym_to_full(xs)), vs[..., None],
                                                       upper=False), per),
                ('solve from factor',
                 lambda: S.sym_chol_apply(fac, S.sym_chol_apply(fac, v, 'Linv', factored=True), 'LTinv', factored=True),
                 2 * (K + 2 * N), 'cholesky_solve', lambda: torch.cholesky_solve(vs[..., None], full_l), per),
                ('sym_logdet', lambda: S.sym_logdet(x), K + 1, 'sym_det + log', lambda: S.sym_det(x).log(), 1.0),
                ('sym_mahalanobis', lambda: S.sym_mahalanobis(x, v), K + N + 1, 'sym_solve + dot',
                 lambda: (S.sym_solve(x, v) * v).sum(-1), 1.0),
                ('sym_gauss_logpdf', lambda: S.sym_gauss_logpdf(x, v), K + N + 1, 'sym_det + log, sym_solve + dot',
                 lambda: -0.5 * (c0 + S.sym_det(x).log() + (S.sym_solve(x, v) * v).sum(-1)), 1.0),
                ('logdet backward', lambda: S._chol_backward(5, x, None, g, None), 2 * K + 1, 'autograd of sym_det + log',
                 chain_grad(lambda a: S.sym_det(a).log(), x), 1.0),
                ('mahalanobis backward', lambda: S._chol_backward(6, x, v, g, None), 2 * (K + N) + 1,
                 'autograd of sym_solve + dot', chain_grad(lambda a, b: (S.sym_solve(a, b) * b).sum(-1), x, v), 1.0),
                ('logpdf backward', lambda: S._chol_backward(8, x, v, g, None), 2 * (K + N) + 1, '-', None, 1.0),
                ('sym_solve (yardstick)', lambda: S.sym_solve(x, v), K + 2 * N, '-', None, 1.0),
            ]
            for op, call, elems, cname, chain, scale in rows:
                t = timeit(call)
                share = elems * es * n / t / BW
                shares[(op, dtype, N)] = share
                vg, wv = resources(census, op, dtype, N)
                if chain is None:
                    ratio = '-'
                else:
                    tc = timeit(chain, reps=5) * scale
                    ratio = f'{tc / t:.1f}'
                    if tc < t:
                        slower.append(f'{op} {str(dtype)[6:]} N={N}: {tc / t:.2f}x the chain `{cname}` '
                                      f'({n / t * 1e-9:.3f}e9 records/s)')
                out.append(f'| {op} | {str(dtype)[6:]} | {N} | {n} | {n / t * 1e-9:.3f} | {share:.3f} | {vg} | {wv} | '
                           f'{cname} | {ratio} |')
                print(out[-1], flush=True)
            del x, v, g, fac, full_l
    out += ['', '## The expectation', '',
            'logpdf at 3 x 3 / 4 x 4 float32 moves about the bytes of sym_solve at the same order; its share of the '
            'roofline beside sym_solve\'s:', '']
    for N in (3, 4):
        a, b = shares[('sym_gauss_logpdf', torch.float32, N)], shares[('sym_solve (yardstick)', torch.float32, N)]
        out.append(f'- N = {N}: logpdf {a:.3f}, sym_solve {b:.3f} ({a / b:.2f} of it)')
    out += ['', '## Known weak spots', '',
            'Cases slower than the chain they replace: ' + ('; '.join(slower) if slower else 'none') + '.']
    text = '\n'.join(out) + '\n'
    if args.md:
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
