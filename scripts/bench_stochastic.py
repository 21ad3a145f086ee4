#!/usr/bin/env python
"""What the library side of the stochastic estimators costs (nfm_stochastic.hip) against the torch compositions the
reference uses for the same work, on the same device in the same run, at 2^27 elements, float32 and float64:

  fill      Rademacher and Gaussian probes against `bernoulli(full(.5).expand(n)).sub_(.5).mul_(2)` / `randn`,
            and as a fraction of the write ceiling (a `fill_` of 1 GiB measured first);
  gram      (1, 1) against `torch.dot`; (4, 4) against the 16 dots and against one `matmul` of the flattened stacks;
  combine   (4, 4) against the 16 `addcmul_` passes (+ the subtraction);
  orth      m = 4 (Gram-Schmidt applied twice) against `torch.linalg.qr` of the n x 4 matrix;
  trapprox  Hutchinson and Hutch++ (samples = 12, 5 moments) end to end on a diagonal operator and on `sym_matvec` of
            a 3 x 3 compact field, against the reference's algorithm restated in torch ops on the device.

Times are medians of event-timed calls after a settle phase (scripts/_timing.py).

    python scripts/bench_stochastic.py [--md profiles/stochastic_table.md] [--log2n 27]"""
import argparse
import math
import os
import sys
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _timing import timeit  # noqa: E402
import nitorch_fastmath_amd as N_  # noqa: E402

S, L = N_.stochastic, N_._lib
LINES = []
MD = [None]


def emit(line):
    print(line, flush=True)
    LINES.append(line)
    if MD[0]:       # kept current: the table survives a run that is cut short
        open(MD[0], 'w').write('\n'.join(LINES) + '\n')


def row(what, dtype, t, tb, base, extra=''):
    emit(f'| {what} | {str(dtype)[6:]} | {t * 1e3:.3f} | {base} | {tb * 1e3:.3f} | {tb / t:.2f} | {extra} |')


def torch_rademacher(shape, dtype, dev):
    x = torch.bernoulli(torch.full([], 0.5, dtype=dtype, device=dev).expand(shape))
    return x.sub_(0.5).mul_(2)


def torch_trapprox(matvec, shape, moments, samples, hutchpp, dtype, dev):
    """Hutchinson / Hutch++ as the reference composes them from torch ops: dots in the working dtype, scalar
    writes into the result, addcmul_ passes for the deflation, torch.linalg.qr for the basis"""
    t = torch.zeros(moments, dtype=dtype, device=dev)
    if not hutchpp:
        for _ in range(samples):
            m = v = torch_rademacher(shape, dtype, dev)
            for j in range(moments):
                m = matvec(m)
                t[j] += m.flatten().dot(v.flatten())
        return t / samples
    m_ = int(math.ceil(samples / 3))
    apply = lambda x: torch.stack([matvec(x[j]) for j in range(m_)])                      # noqa: E731
    q, g = torch_rademacher([m_, *shape], dtype, dev), torch_rademacher([m_, *shape], dtype, dev)
    q = torch.linalg.qr(apply(q).reshape(m_, -1).T)[0].T.reshape(q.shape)
    z = q.new_empty(m_, m_)
    for j in range(m_):
        for k in range(m_):
            z[j, k] = q[j].flatten().dot(g[k].flatten())
    d = torch.zeros_like(g)
    for j in range(m_):
        for k in range(m_):
            d[j].addcmul_(q[k], z[k, j])
    g -= d
    mq, mg = q, g
    for j in range(moments):
        mq, mg = apply(mq), apply(mg)
        t[j] = sum(q[i].flatten().dot(mq[i].flatten()) for i in range(m_)) \
            + sum(g[i].flatten().dot(mg[i].flatten()) for i in range(m_)) / m_
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    ap.add_argument('--log2n', type=int, default=27)
    args = ap.parse_args()
    MD[0] = args.md
    dev = torch.device('cuda:0')
    n = 1 << args.log2n
    buf = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    wceil = buf.numel() * 4 / timeit(lambda: buf.fill_(1.0))
    src = torch.empty_like(buf).normal_()
    rceil = 2.0 * buf.numel() * 4 / timeit(lambda: buf.copy_(src))
    del buf, src
    torch.cuda.empty_cache()
    emit(f'n = 2^{args.log2n} elements per vector.  Write ceiling measured in this run: {wceil / 1e12:.2f} TB/s (`fill_` of '
         f'1 GiB); copy ceiling {rceil / 1e12:.2f} TB/s (read + write).')
    emit('')
    emit('| case | dtype | ms | torch composition | its ms | x torch | note |')
    emit('|---|---|---|---|---|---|---|')
    for dtype in (torch.float32, torch.float64):
        es = 4 if dtype == torch.float32 else 8
        out = torch.empty(n, dtype=dtype, device=dev)
        # ---- fill
        t = timeit(lambda: S._fill(out, L.STOCH_RADEMACHER, 1234))
        tb = timeit(lambda: torch_rademacher([n], dtype, dev))
        row('fill rademacher', dtype, t, tb, 'bernoulli(full(.5).expand).sub_.mul_', f'{n * es / t / wceil:.2f} of the write ceiling')
        t = timeit(lambda: S._fill(out, L.STOCH_GAUSSIAN, 1234))
        tb = timeit(lambda: torch.randn(n, dtype=dtype, device=dev))
        row('fill gaussian', dtype, t, tb, 'randn', f'{n * es / t / wceil:.2f} of the write ceiling')
        del out
        # ---- gram / combine
        xs = torch.randn(4, n, dtype=dtype, device=dev)
        ys = torch.randn(4, n, dtype=dtype, device=dev)
        o1 = torch.empty(1, dtype=torch.float64, device=dev)
        o16 = torch.empty(16, dtype=torch.float64, device=dev)
        t = timeit(lambda: S._gram([xs[0]], [ys[0]], o1))
        tb = timeit(lambda: torch.dot(xs[0], ys[0]))
        row('gram (1,1)', dtype, t, tb, 'dot', f'{2 * n * es / t / rceil:.2f} of the copy ceiling')
        xl, yl = [xs[j] for j in range(4)], [ys[k] for k in range(4)]
        t = timeit(lambda: S._gram(xl, yl, o16))
        tb = timeit(lambda: [torch.dot(a, b) for a in xl for b in yl])
        row('gram (4,4)', dtype, t, tb, '16 dots', f'{8 * n * es / t / rceil:.2f} of the copy ceiling')
        tb = timeit(lambda: xs @ ys.T)
        row('gram (4,4)', dtype, t, tb, 'matmul of the stacks', '')
        c = torch.randn(16, dtype=torch.float64, device=dev)
        cd = c.to(dtype).reshape(4, 4)
        zs = torch.empty_like(ys)
        zl = [zs[k] for k in range(4)]

        def addcmul_loop():
            d = torch.zeros_like(ys)
            for j in range(4):
                for k in range(4):
                    d[j].addcmul_(xs[k], cd[k, j])
            return ys - d
        t = timeit(lambda: S._combine(xl, c, yl, zl))
        tb = timeit(addcmul_loop)
        row('combine (4,4)', dtype, t, tb, '16 addcmul_ + sub', f'{12 * n * es / t / rceil:.2f} of the copy ceiling')
        # ---- orth
        work = torch.empty_like(xs)

        def orth():
            work.copy_(xs)
            S._orth(work)
        tcopy = timeit(lambda: work.copy_(xs))
        t = timeit(orth, reps=4) - tcopy
        tb = timeit(lambda: torch.linalg.qr(xs.T), reps=3)
        row('orth m = 4', dtype, t, tb, 'linalg.qr of the n x 4 matrix', 'CGS2: 30 launches')
        del xs, ys, zs, work, xl, yl, zl
        torch.cuda.empty_cache()
        # ---- trapprox end to end
        lam = torch.rand(n, dtype=dtype, device=dev) + 0.5
        n3 = n // 3
        sym = torch.rand(n3, 6, dtype=dtype, device=dev)
        sym[:, :3] += 2
        ops = {'diagonal': (lambda x: x * lam, [n]), 'sym_matvec 3x3': (lambda x: N_.sym_matvec(sym, x), [n3, 3])}
        for name, (mv, shape) in ops.items():
            for hpp in (False, True):
                kw = dict(moments=5, samples=12, hutchpp=hpp, dtype=dtype, device=dev)
                t = timeit(lambda: S.trapprox(mv, shape, **kw), reps=3)
                tb = timeit(lambda: torch_trapprox(mv, shape, 5, 12, hpp, dtype, dev), reps=3)
                row(f'trapprox {"hutch++" if hpp else "hutchinson"}, {name}', dtype, t, tb, 'the reference composition', '12 samples, 5 moments')
        del lam, sym
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
