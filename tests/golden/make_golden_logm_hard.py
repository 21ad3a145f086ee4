#!/usr/bin/env python
"""Generate tests/golden/logm_hard.npz: hard inputs of `logm`, `logm_solve` and the Frechet kernel with a validated
truth (classes, tiers and bounds: tests/_logm_ref.py).  Needs mpmath and scipy, no GPU.

Per (dtype, order) and class, PER_CLASS records (2 at the torch route's orders, tier-A classes only).  A record is
    x       the input, rounded to the dtype first
    true    log x: mpmath at 60 digits, `mpmath.logm` or else the eigendecomposition, accepted only when
            ||expm(T) - x||_max <= 1e-30 ||x||_max and |Im T| <= 1e-30 (`res` keeps the larger of the two)
    nK, cl  ||K(x)||_2 and cond_log(x) (float64, from the truth)
    cls, par, tier
    E, L    at orders 2..5: a direction and L_log(x, E), the central difference of validated logarithms at
            h = 1e-20 ||x||_max and 80 digits
and per (dtype, order with a kernel) the logm_solve pairs: a graded M, an A of each tier-A class, the validated
logarithm of M^-1 A formed in mpmath, kappa_1(M) and cond_log(M^-1 A); a class of which no draw of 48 gives an
M^-1 A with a real logarithm is listed in `no_pair` (rotations by almost pi at small orders).

A seed is kept only if the torch route `_logm_torch` (the kernel's algorithm), run on the CPU in the record's dtype,
and its `torch.func.jvp` meet the record's bounds at half the constant without a NaN; a tier-A class that cannot fill
its records that way at some (dtype, order) is moved to tier B there and reported (`demoted`), never dropped.
`rejected` counts the seeds turned away per (dtype, order, class): the fixture is a sample of what the algorithm can
do, not of the class.

    python tests/golden/make_golden_logm_hard.py [-j N]       # rewrites tests/golden/logm_hard.npz
"""
import argparse
import os
import pickle
import sys
import warnings
from multiprocessing import Pool
import numpy as np

warnings.filterwarnings('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _logm_ref as R  # noqa: E402

MAX_TRY = 12            # seeds per record before a tier-A class is moved to tier B
HALF = R.C_LOGM / 2


def np_dtype(dt):
    return np.float32 if dt == 'f32' else np.float64


def truth(a64):
    """-> (T float64, residual, ||K||_2, cond_log, Kexp) or None"""
    import mpmath
    with mpmath.workdps(60):
        L, res, _ = R.mp_logm(R.mp_of(a64))
        if L is None:
            return None
        T = R.mp_to_np(L)
    nK, Kexp = R.klog_norm(T)
    if not np.isfinite(nK):
        return None
    return T, res, nK, nK * R.fro(a64) / R.fro(T), Kexp


def frechet_truth(a64, e64, Kexp):
    import mpmath
    with mpmath.workdps(80):
        L = R.mp_frechet(R.mp_of(a64), R.mp_of(e64))
        if L is None:
            return None
        L = R.mp_to_np(L)
    # the two truths against each other: L_exp(T, L_log(x, E)) = E
    back = (Kexp @ L.ravel()).reshape(e64.shape)
    assert R.fro(back - e64) <= 1e-6 * np.linalg.norm(Kexp, 2) * R.fro(L), 'K and L_true disagree'
    return L


def route_ok(x, rec, dt, tier):
    """the torch route on the CPU in the record's dtype, at half the constant"""
    import torch
    from torch.func import jvp
    from nitorch_fastmath_amd.logm import _logm_torch
    xt = torch.from_numpy(x)[None]
    one = {k: np.asarray(v)[None] for k, v in rec.items()}
    one['tier'] = np.array([tier])
    ok, _, _ = R.check_logm(_logm_torch(xt).numpy(), one, dt, HALF)
    if not ok[0]:
        return False
    if 'L' in rec and tier == R.TIER_A:
        l = jvp(_logm_torch, (xt,), (torch.from_numpy(rec['E'])[None],))[1].numpy()
        if not (np.isfinite(l).all() and R.frechet_ratio(l, one, dt)[0] <= HALF):
            return False
    return True


def one_record(dt, D, cls, par, tier, rng):
    a = R.make(cls, D, par, rng).astype(np_dtype(dt))
    e = rng.standard_normal((D, D)).astype(np_dtype(dt))
    if not np.isfinite(a).all():
        return None
    t = truth(a.astype(np.float64))
    if t is None:
        return None
    rec = {'true': t[0], 'res': t[1], 'nK': t[2], 'cl': t[3]}
    if D in R.FRECHET_ORDERS:
        L = frechet_truth(a.astype(np.float64), e.astype(np.float64), t[4])
        if L is None:
            return None
        rec['E'], rec['L'] = e, L
    if not route_ok(a, rec, dt, tier):
        return None
    rec.update(x=a, cls='rot' if cls == 'rotb' else cls, par=float(par), tier=tier)
    return rec


def one_class(dt, D, cls, tier, pars, n, rng, log):
    recs, rejected = [], 0
    for i in range(n):
        par = pars[(i + D) % len(pars)]
        for _ in range(MAX_TRY):
            rec = one_record(dt, D, cls, par, tier, rng)
            if rec is not None:
                break
            rejected += 1
        else:
            if tier == R.TIER_A:
                log['demoted'].append(f'{dt}/{D}/{cls}/{par:g}')
                return one_class(dt, D, cls, R.TIER_B, pars, n, rng, log)
            raise RuntimeError(f'no seed of {dt} D={D} {cls} {par} meets even tier B')
        recs.append(rec)
    bump(log, f'{dt}/{D}/{cls}/{"AB"[tier]}', rejected)
    return recs


def bump(log, key, n=1):
    if n:
        log['rejected'][key] = log['rejected'].get(key, 0) + n


def solve_pairs(dt, D, rng, log):
    import torch
    import mpmath
    from nitorch_fastmath_amd.logm import _logm_torch
    out = []
    ta = [c for c, (t, _) in R.CLASSES.items() if t == R.TIER_A]
    for i, cls in enumerate(ta):
        pars = R.CLASSES[cls][1][dt]
        for k in range(4 * MAX_TRY):
            M = R.make('graded', D, R.SOLVE_M[dt][(i + D) % 2], rng).astype(np_dtype(dt))
            A = R.make(cls, D, pars[(i + D + k) % len(pars)], rng).astype(np_dtype(dt))
            with mpmath.workdps(60):
                Q = mpmath.inverse(R.mp_of(M)) * R.mp_of(A)
                L, res, _ = R.mp_logm(Q)
                if L is None:
                    bump(log, f'{dt}/{D}/solve-{cls}/no real logarithm')
                    continue
                T, q64 = R.mp_to_np(L), R.mp_to_np(Q)
            nK, _ = R.klog_norm(T)
            cl = nK * R.fro(q64) / R.fro(T)
            kap = np.linalg.cond(M.astype(np.float64), 1)
            x = _logm_torch(torch.linalg.solve(torch.from_numpy(M), torch.from_numpy(A))[None])[0].numpy()
            r = R.fro(x.astype(np.float64) - T) / R.fro(T) / (D * R.EPS[dt] * kap * max(1.0, cl))
            if np.isfinite(x).all() and r <= HALF:
                out.append(dict(sm=M, sa=A, strue=T, skap=kap, scl=cl, scls=cls, sres=res))
                break
            bump(log, f'{dt}/{D}/solve-{cls}/over the bound')
        else:
            # (M^-1 A of a rotation by almost pi and a graded M has its eigenvalues on the negative real axis at
            # small orders: there is no such pair to keep)
            log['no_pair'].append(f'{dt}/{D}/{cls}')
    return out


def task(arg):
    dt, D, route, cache = arg
    path = cache and os.path.join(cache, f'{dt}_{D}.pkl')
    if path and os.path.exists(path):
        with open(path, 'rb') as f:
            return pickle.load(f)
    res = build(dt, D, route)
    if path:
        with open(path, 'wb') as f:
            pickle.dump(res, f)
    return res


def build(dt, D, route):
    import torch
    torch.set_num_threads(1)
    rng = np.random.default_rng([20261019, 0 if dt == 'f32' else 1, D])
    log = {'demoted': [], 'rejected': {}, 'no_pair': []}
    recs = []
    for cls, (tier, pars) in R.CLASSES.items():
        if route and tier == R.TIER_B:
            continue
        recs += one_class(dt, D, cls, tier, pars[dt], 2 if route else R.PER_CLASS, rng, log)
    out = {}
    for k in recs[0]:
        out[f'{k}_{dt}_{D}'] = np.stack([r[k] for r in recs]) if k not in ('cls',) else np.array([r[k] for r in recs])
    out[f'tier_{dt}_{D}'] = out[f'tier_{dt}_{D}'].astype(np.uint8)
    if not route:
        pairs = solve_pairs(dt, D, rng, log)
        for k in pairs[0]:
            out[f'{k}_{dt}_{D}'] = np.stack([p[k] for p in pairs]) if k != 'scls' else np.array([p[k] for p in pairs])
    print(dt, D, 'done', log, flush=True)
    return out, log


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('-j', type=int, default=8)
    ap.add_argument('--out', default=R.PATH)
    ap.add_argument('--cache', help='directory that keeps every finished (dtype, order): a rerun takes them from there')
    args = ap.parse_args()
    if args.cache:
        os.makedirs(args.cache, exist_ok=True)
    tasks = [(dt, D, False, args.cache) for dt in R.ORDERS for D in R.ORDERS[dt]]
    tasks += [(dt, D, True, args.cache) for dt in R.ROUTE_ORDERS for D in R.ROUTE_ORDERS[dt]]
    tasks.sort(key=lambda t: -t[1])
    out, demoted, rejected, no_pair = {}, [], [], []
    with Pool(args.j) as pool:
        for o, log in pool.imap_unordered(task, tasks):
            out.update(o)
            demoted += log['demoted']
            rejected += [f'{k}:{v}' for k, v in log['rejected'].items()]
            no_pair += log['no_pair']
    out['demoted'] = np.array(sorted(demoted), dtype=str)
    out['rejected'] = np.array(sorted(rejected), dtype=str)
    out['no_pair'] = np.array(sorted(no_pair), dtype=str)
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), 'bytes')
    print('demoted:', sorted(demoted))
    print('rejected:', sorted(rejected))
    print('no logm_solve pair:', sorted(no_pair))


if __name__ == '__main__':
    main()
