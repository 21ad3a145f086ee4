#!/usr/bin/env python
"""Throughput of `sugar.lmdiv` (nfm_sugar.hip) against what a user has on the same device without it:
`torch.linalg.solve` (for 'chol': `torch.linalg.cholesky` + `torch.cholesky_solve`, the reference's composition)
and `batchinv(a) @ b`.

Cases: method lu and chol; (N, K) in (3,3) (4,4) (6,6) (8,8) (4,1) (8,1); float32 and float64; layouts
contiguous, channel-first (a, b and the result) and one `a` broadcast against every `b`.  The batch is 2^24
records where the three operands and the baselines' temporaries stay below ~3 GiB, else halved down to 2^20.
Per row: time (median of event-timed launches after a settle phase, scripts/_timing.py), the algorithmic bytes
(N^2 + 2 N K) sizeof(T) per record over that time as a share of 8 TB/s (a broadcast `a` is not counted), and
baseline time / our time.  The baselines run on the first 2^20 records of the same tensors (torch's batched LU takes
seconds beyond, and its temporaries do not fit next to the operands); their time is scaled to the full batch.

    python scripts/bench_sugar.py [--md profiles/sugar_table.md] [--max-log2n 24]
    python scripts/bench_sugar.py --accuracy [--md profiles/sugar_accuracy.md]

--accuracy: the per-record excess eta / (2 eta_ref + 4 N eps) of tests/_solver_ref.py over the graded families
(every cond, n = 209 and 17, K = 1, 3, 8, per-record powers of two), worst column of the worst record per
(method, dtype, N); the reference is torch on the CPU in the same dtype."""
import argparse
import os
import sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import timeit  # noqa: E402
import nitorch_fastmath_amd as N_  # noqa: E402

S, B = N_.sugar, N_.batched
BW = 8.0e12
CASES = ((3, 3), (4, 4), (6, 6), (8, 8), (4, 1), (8, 1))


def small_matmul(a, b):
    out = a[..., :, 0:1] * b[..., 0:1, :]
    for k in range(1, a.shape[-1]):
        out = out + a[..., :, k:k + 1] * b[..., k:k + 1, :]
    return out


def speed(args):
    dev = torch.device('cuda:0')
    lines = ['| method | N | K | dtype | layout | log2 n | ms | share of 8 TB/s | x torch solve | x batchinv @ b |',
             '|---|---|---|---|---|---|---|---|---|---|']
    gen = torch.Generator(device='cuda').manual_seed(0)
    for method in ('lu', 'chol'):
        for N, K in CASES:
            for dtype in (torch.float32, torch.float64):
                es = 4 if dtype == torch.float32 else 8
                rec = (N * N + 2 * N * K) * es
                log2n = args.max_log2n
                while log2n > 20 and (rec + 2 * N * N * es) * (1 << log2n) > 3 << 30:
                    log2n -= 1
                n = 1 << log2n
                g = torch.randn(n, N, N, dtype=dtype, device=dev, generator=gen)
                a = (small_matmul(g, g.mT) / N if method == 'chol' else g) + (1 if method == 'chol' else 4) * torch.eye(N, dtype=dtype, device=dev)
                del g
                b = torch.randn(n, N, K, dtype=dtype, device=dev, generator=gen)
                if method == 'lu':
                    stock = (lambda x, y: torch.linalg.solve(x, y))
                else:
                    stock = (lambda x, y: torch.cholesky_solve(y, torch.linalg.cholesky(x, upper=False), upper=False))
                side = 1 << (log2n // 2)
                cf = (lambda x: x.reshape(side, n // side, *x.shape[1:]).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
                layouts = (('contiguous', a, b, rec), ('channel-first', cf(a), cf(b), rec),
                           ('a broadcast', a[0], b, 2 * N * K * es))
                nbase = 1 << 20
                for name, x, y, nbytes in layouts:
                    if name == 'channel-first':
                        xb, yb = x[:nbase // (n // side)], y[:nbase // (n // side)]
                    else:
                        xb, yb = (x if x.dim() == 2 else x[:nbase]), y[:nbase]
                    with torch.no_grad():
                        t = timeit(lambda: S.lmdiv(x, y, method))
                        ts = timeit(lambda: stock(xb, yb), reps=3, settle_ms=10.0) * (n / nbase)
                        ti = timeit(lambda: small_matmul(B.batchinv(xb), yb), reps=3, settle_ms=10.0) * (n / nbase)
                    r = (f'| {method} | {N} | {K} | {str(dtype)[6:]} | {name} | {log2n} | {t * 1e3:.3f} | '
                         f'{nbytes * n / t / BW:.3f} | {ts / t:.1f} | {ti / t:.2f} |')
                    print(r, flush=True)
                    lines.append(r)
                del a, b
                torch.cuda.empty_cache()
    return lines


def accuracy(args):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _solver_ref as R
    dev = torch.device('cuda:0')
    lines = ['| method | dtype | N | worst eta / bound | worst eta / (N eps) | worst reference eta / (N eps) |', '|---|---|---|---|---|---|']
    for method in ('lu', 'chol'):
        for dn in ('f32', 'f64'):
            for N in range(1, 9):
                wx = we = wr = 0.0
                for cond in R.CONDS[dn]:
                    for n in R.NS:
                        k = R.pow2_scales(n, R.KMAX_LINEAR[dn], 900 + N)
                        if method == 'lu':
                            a = R.scaled(R.general_graded(n, N, cond, dn, 200 + N)[0], k)
                        else:
                            a = R.scaled(R.to_full(R.spd_graded(n, N, cond, dn, 100 + N)[0]).astype(R.NP[dn]), k)
                        for K in (1, 3, 8):
                            b = np.random.default_rng(910 + K).standard_normal((n, N, K)).astype(R.NP[dn])
                            got = S.lmdiv(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), method).cpu().numpy()
                            ta, tb = torch.from_numpy(a), torch.from_numpy(b)
                            if method == 'lu':
                                ref = torch.linalg.solve(ta, tb).numpy()
                            else:
                                ref = torch.cholesky_solve(tb, torch.linalg.cholesky(ta), upper=False).numpy()
                            for col in range(K):
                                eta = R.solve_eta(a, got[..., col], b[..., col], dn)
                                er = R.solve_eta(a, ref[..., col], b[..., col], dn)
                                wx = max(wx, float((eta / R.eta_bound(er, N, dn)).max()))
                                we, wr = max(we, float(eta.max())), max(wr, float(er.max()))
                u = N * R.EPS[dn]
                r = f'| {method} | {dn} | {N} | {wx:.3f} | {we / u:.3f} | {wr / u:.3f} |'
                print(r, flush=True)
                lines.append(r)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    ap.add_argument('--max-log2n', type=int, default=24)
    ap.add_argument('--accuracy', action='store_true')
    args = ap.parse_args()
    lines = accuracy(args) if args.accuracy else speed(args)
    if args.md:
        open(args.md, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
