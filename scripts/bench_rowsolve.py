#!/usr/bin/env python
"""Throughput of `sugar.lmdiv` at the square orders 9..16 (nfm_rowsolve.hip) against the route the same call took
before the kernel existed, on the same tensors: `torch.linalg.solve` for 'lu', `torch.linalg.cholesky` +
`torch.cholesky_solve` for 'chol'; `batchinv(a) @ b` as information.

Cases: (N, K) in (9,1) (12,3) (16,1) (16,8); float32 and float64; 'lu' and 'chol'; layouts contiguous, channel-first
(a, b and the result) and `a.mT`.  2^20 records, 2^19 for float64 at order 16 (a, its baselines' temporaries and the
channel-first copies stay below ~8 GiB).  The baselines run on the first 2^17 records of the same tensors (torch's
batched LU takes seconds beyond) and their times are scaled to the full batch.

Per row: the median of event-timed launches after a settle phase (the protocol of scripts/_timing.py, all samples
kept), the run-to-run spread (max - min) / median of ours and of the baseline, the algorithmic bytes
(N^2 + 2 N K) sizeof(T) per record over the median as a share of 8 TB/s, baseline / ours, and the verdict of the
routing rule: `kernel` when even our slowest sample is below the baseline's fastest, `torch` otherwise.

    python scripts/bench_rowsolve.py [--md profiles/rowsolve_table.md]
    python scripts/bench_rowsolve.py --accuracy [--md profiles/rowsolve_accuracy.md]
    python scripts/bench_rowsolve.py --build-forms          # no device needed
    python scripts/bench_rowsolve.py --forms [--md profiles/rowsolve_forms.md]

--accuracy: the worst eta / (2 eta_ref + 4 N eps) per (method, dtype, N) over the cases of
tests/test_gpu_rowsolve.py::test_lmdiv_graded_per_record (which asserts it for every column of every record).
--build-forms compiles the kernels in every candidate form (R rows per lane in 1, 2, 4; pivot row by ds_bpermute or
through the LDS slot) into build/rowsolve_forms/librowsolve_R<r>_LB<0|1>.so; --forms times them against each other
through the C entry point (contiguous operands, K = 1 and 8, 2^18 records): the table `rowsolve_choice` is filled from."""
import argparse
import ctypes
import os
import subprocess
import sys
import time
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BW = 8.0e12
CASES = ((9, 1), (12, 3), (16, 1), (16, 8))
FORMS = [(r, lb) for r in (1, 2, 4) for lb in (0, 1)]
FORM_DIR = os.path.join(ROOT, 'build', 'rowsolve_forms')
CSRC = os.path.join(ROOT, 'nitorch_fastmath_amd', 'csrc')


def samples(fn, reps=8, settle_ms=40.0):
    """scripts/_timing.py's protocol, every sample returned (sorted, seconds)"""
    fn()
    torch.cuda.synchronize()
    t_end = time.perf_counter() + settle_ms * 1e-3
    while time.perf_counter() < t_end:
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(max(3, reps)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return sorted(ts)


def med(ts):
    return ts[len(ts) // 2]


def spread(ts):
    return (ts[-1] - ts[0]) / med(ts)


def small_matmul(a, b):
    out = a[..., :, 0:1] * b[..., 0:1, :]
    for k in range(1, a.shape[-1]):
        out = out + a[..., :, k:k + 1] * b[..., k:k + 1, :]
    return out


def systems(method, n, N, dtype, dev, gen):
    g = torch.randn(n, N, N, dtype=dtype, device=dev, generator=gen)
    if method == 'chol':
        return small_matmul(g, g.mT) / N + torch.eye(N, dtype=dtype, device=dev)
    return g + 4 * torch.eye(N, dtype=dtype, device=dev)


def speed(args):
    import nitorch_fastmath_amd as N_
    S, B = N_.sugar, N_.batched
    dev = torch.device('cuda:0')
    lines = ['| method | N | K | dtype | layout | log2 n | ms | spread | share of 8 TB/s | parent route ms | its spread | '
             'x parent route | x batchinv @ b | route |', '|' + '---|' * 14]
    gen = torch.Generator(device='cuda').manual_seed(0)
    nbase = 1 << 17
    for method in ('lu', 'chol'):
        for N, K in CASES:
            for dtype in (torch.float32, torch.float64):
                es = 4 if dtype == torch.float32 else 8
                log2n = 19 if (es == 8 and N == 16) else 20
                n = 1 << log2n
                a = systems(method, n, N, dtype, dev, gen)
                b = torch.randn(n, N, K, dtype=dtype, device=dev, generator=gen)
                if method == 'lu':
                    stock = (lambda x, y: torch.linalg.solve(x, y))
                else:
                    stock = (lambda x, y: torch.cholesky_solve(y, torch.linalg.cholesky(x, upper=False), upper=False))
                side = 1 << (log2n // 2)
                cf = (lambda x: x.reshape(side, n // side, *x.shape[1:]).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
                layouts = (('contiguous', a, b), ('channel-first', cf(a), cf(b)), ('a.mT', a.mT.contiguous().mT, b))
                for name, x, y in layouts:
                    if name == 'channel-first':
                        xb, yb = x[:nbase // (n // side)], y[:nbase // (n // side)]
                    else:
                        xb, yb = x[:nbase], y[:nbase]
                    with torch.no_grad():
                        t = samples(lambda: S.lmdiv(x, y, method))
                        ts = [v * (n / nbase) for v in samples(lambda: stock(xb, yb), reps=5, settle_ms=10.0)]
                        ti = med(samples(lambda: small_matmul(B.batchinv(xb), yb), reps=3, settle_ms=10.0)) * (n / nbase)
                    route = 'kernel' if t[-1] < ts[0] else 'torch'
                    r = (f'| {method} | {N} | {K} | {str(dtype)[6:]} | {name} | {log2n} | {med(t) * 1e3:.3f} | {spread(t):.3f} | '
                         f'{(N * N + 2 * N * K) * es * n / med(t) / BW:.3f} | {med(ts) * 1e3:.1f} | {spread(ts):.3f} | '
                         f'{med(ts) / med(t):.1f} | {ti / med(t):.2f} | {route} |')
                    print(r, flush=True)
                    lines.append(r)
                del a, b, layouts
                torch.cuda.empty_cache()
    return lines


def accuracy(args):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gpu_rowsolve as T
    dev = torch.device('cuda:0')
    lines = ['| method | dtype | N | worst eta / bound |', '|---|---|---|---|']
    rows = {}
    for dn in T.DNS:
        for N in T.ORDERS:
            for method, w in T.graded_worst(dev, dn, N).items():
                rows[(method, dn, N)] = w
    for method in T.METHODS:
        for dn in T.DNS:
            for N in T.ORDERS:
                lines.append(f'| {method} | {dn} | {N} | {rows[(method, dn, N)]:.3f} |')
                print(lines[-1], flush=True)
    return lines


def form_lib(r, lb):
    return os.path.join(FORM_DIR, f'librowsolve_R{r}_LB{lb}.so')


def build_forms(args):
    """the entry object and the 16 part objects of every form into one small shared library each (nfm_batch_inv,
    which the entry point names, resolves against libnfm_hip.so at load time)"""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    flags = ['-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-ffp-contract=off', '-Wno-pass-failed']
    src = os.path.join(CSRC, 'nfm_rowsolve.hip')
    for r, lb in FORMS:
        d = os.path.join(FORM_DIR, f'R{r}_LB{lb}')
        os.makedirs(d, exist_ok=True)
        defs = [f'-DNFM_ROWSOLVE_FORM_R={r}', f'-DNFM_ROWSOLVE_FORM_LB={lb}']
        jobs = [(os.path.join(d, 'entry.o'), [])] + [(os.path.join(d, f'part_{p}.o'), [f'-DNFM_ROWSOLVE_PART={p}']) for p in range(16)]
        for chunk in (jobs[:1], jobs[1:]):                  # at most 16 compilers at a time
            procs = [subprocess.Popen([hipcc] + flags + defs + extra + ['-c', src, '-o', obj]) for obj, extra in chunk]
            if any([p.wait() for p in procs]):
                raise RuntimeError(f'form R={r} LB={lb} does not compile')
        # -Bsymbolic: the entry point reaches its own parts, not the same symbols of libnfm_hip.so loaded before it
        subprocess.check_call([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-Wl,-Bsymbolic', '-o', form_lib(r, lb)] +
                              [obj for obj, _ in jobs])
        print('built', form_lib(r, lb), flush=True)
    return []


def forms(args):
    import nitorch_fastmath_amd as N_
    from nitorch_fastmath_amd import _lib
    from nitorch_fastmath_amd._dispatch import stream_ptr
    ctypes.CDLL(_lib.LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    dev = torch.device('cuda:0')
    libs = {}
    for r, lb in FORMS:
        L = ctypes.CDLL(form_lib(r, lb))
        L.nfm_rowsolve.argtypes = _lib.SIGNATURES['nfm_rowsolve']
        L.nfm_rowsolve.restype = ctypes.c_int
        libs[(r, lb)] = L
    gen = torch.Generator(device='cuda').manual_seed(0)
    n = 1 << 18
    head = ' | '.join(f'R={r} {"slot" if lb else "bperm"}' for r, lb in FORMS)
    lines = [f'| dtype | N | method | K | {head} | best | spread of the best |', '|' + '---|' * (6 + len(FORMS))]
    for dtype, code in ((torch.float32, 0), (torch.float64, 1)):
        for N in range(9, 17):
            for method, flag in (('lu', 0), ('chol', 1)):
                a = systems(method, n, N, dtype, dev, gen)
                for K in (1, 8):
                    b = torch.randn(n, N, K, dtype=dtype, device=dev, generator=gen)
                    out = torch.empty_like(b)
                    got, ref = {}, None
                    for form, L in libs.items():
                        def run():
                            rc = L.nfm_rowsolve(code, N, K, flag, 1, n, a.data_ptr(), 0, N * N, N, 1, b.data_ptr(), 0, N * K, K, 1,
                                                out.data_ptr(), 0, N * K, K, 1, stream_ptr(dev))
                            assert rc == 0, rc
                        got[form] = samples(run, reps=5, settle_ms=10.0)
                        ref = out.clone() if ref is None else ref
                        # the forms differ in movement only, and in which of two tied rows pivots
                        same = (out == ref).all(-1).all(-1).float().mean().item()
                        assert same >= 0.99, f'form {form}: {1 - same:.3g} of the records differ from the first form'
                    best = min(got, key=lambda f: med(got[f]))
                    cells = ' | '.join(f'{med(got[f]) * 1e6:.0f}' for f in FORMS)
                    lines.append(f'| {str(dtype)[6:]} | {N} | {method} | {K} | {cells} | R={best[0]} {"slot" if best[1] else "bperm"} | '
                                 f'{spread(got[best]):.3f} |')
                    print(lines[-1], flush=True)
    lines += ['', 'times in microseconds for 2^18 contiguous records, median of 5 after a settle phase']
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--md')
    ap.add_argument('--accuracy', action='store_true')
    ap.add_argument('--build-forms', action='store_true')
    ap.add_argument('--forms', action='store_true')
    args = ap.parse_args()
    fn = accuracy if args.accuracy else build_forms if args.build_forms else forms if args.forms else speed
    lines = fn(args)
    if args.md and lines:
        open(args.md, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
