"""Shared timing helper of the table scripts: steady-state launch time by HIP events.

The first ~10 launches after an idle gap run up to 30 % slower (power-state ramp, bench.py's settle
phase exists for the same reason), so two warm-up calls are not enough for sub-millisecond kernels:
`fn` is launched back to back for `settle_ms` first, then `reps` launches are timed one by one and
the MEDIAN is returned (seconds) -- round 2's tables quoted the minimum after two warm-ups."""
import ctypes
import os
import time
import torch


def timeit(fn, reps=8, settle_ms=40.0, stat='median'):
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
    ts.sort()
    return ts[0] if stat == 'min' else ts[len(ts) // 2]


# ---- two builds of libnfm_hip.so in one process (bench_select_builds.py, bench_spectral_builds.py)
BUILDS_HEADER = ('| call | parent ms | branch ms | parent again ms | parent slower / faster | branch / faster parent | within '
                 '| same bits |\n|---|---|---|---|---|---|---|---|')


def load_build(path, names):
    """another build of the library, with the entry points `names` bound as nitorch_fastmath_amd._lib binds them"""
    from nitorch_fastmath_amd import _lib
    L = ctypes.CDLL(os.path.abspath(path))
    for name in names:
        fn = getattr(L, name)
        fn.argtypes = _lib.SIGNATURES[name]
        fn.restype = ctypes.c_size_t if name.endswith('_workspace_bytes') else ctypes.c_int
    return L


def builds_row(name, parent, branch, val, reps=24):
    """One table row: parent, branch, parent on the same buffers, the branch's result `val` against the first
    parent's bit for bit.  `within`: branch / faster parent <= slower parent / faster parent."""
    times, kept = [], []
    for fn in (parent, branch, parent):
        val.zero_()
        times.append(timeit(fn, reps=reps) * 1e3)
        torch.cuda.synchronize()
        kept.append(val.clone(memory_format=torch.contiguous_format))
    same = torch.equal(kept[0].view(torch.uint8), kept[1].view(torch.uint8))
    p1, b, p2 = times
    spread, ratio = max(p1, p2) / min(p1, p2), b / min(p1, p2)
    print(f'| {name} | {p1:.4f} | {b:.4f} | {p2:.4f} | {spread:.4f} | {ratio:.4f} | {"yes" if ratio <= spread else "no"} | '
          f'{"yes" if same else "NO"} |', flush=True)
    return ratio <= spread, same
