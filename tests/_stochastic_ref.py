"""numpy model of the stochastic module, written from the definitions in include/nfm_hip.h and the public
algorithms (Salmon et al. 2011 for Philox4x32-10; Hutchinson 1989; Meyer et al. 2021 for Hutch++): the
probe streams in float64, Hutchinson and Hutch++ (with Householder QR) on given probes, power iteration."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)


def philox4x32_10(counter, key):
    """counter: 4 uint32 arrays (or ints), key: 2 ints -> 4 uint32 arrays"""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & MASK for x in counter]
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return [x.astype(np.uint32) for x in c]


def _key(seed):
    return seed & 0xffffffff, (seed >> 32) & 0xffffffff


def _units(e, per):
    """the distinct counters e // per of the elements e (uint64), and each element's index into them"""
    g = e // np.uint64(per)
    ug, inv = np.unique(g, return_inverse=True)
    return ug, inv


def rademacher(seed, offset, n):
    """elements [offset, offset + n) of the +-1 stream, float64"""
    e = np.uint64(offset) + np.arange(n, dtype=np.uint64)
    ug, inv = _units(e, 128)
    zero = np.zeros_like(ug)
    w = np.stack(philox4x32_10([ug & MASK, ug >> np.uint64(32), zero, zero], _key(seed)), 1)    # (units, 4)
    b = (e % np.uint64(128)).astype(np.int64)
    bits = (w[inv, b // 32] >> (b % 32).astype(np.uint32)) & np.uint32(1)
    return np.where(bits == 1, 1.0, -1.0)


def _sincospi(x):
    """sin(pi x), cos(pi x) for x in (0, 2) with few significant bits: the reduction to |f| <= 1/4 is exact"""
    k = np.rint(2 * x)
    f = x - k / 2
    s, c = np.sin(np.pi * f), np.cos(np.pi * f)
    k = k.astype(np.int64) % 4
    sn = np.choose(k, [s, c, -s, -c])
    cs = np.choose(k, [c, -s, -c, s])
    return sn, cs


def gaussian(seed, offset, n, return_radius=False):
    """elements [offset, offset + n) of the normal stream, float64 (and the Box-Muller radius of each)"""
    e = np.uint64(offset) + np.arange(n, dtype=np.uint64)
    ug, inv = _units(e, 4)
    zero = np.zeros_like(ug)
    w = philox4x32_10([ug & MASK, ug >> np.uint64(32), zero, zero + np.uint64(1)], _key(seed))
    u = [(2.0 * (x >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24 for x in w]
    r0, r1 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
    s0, c0 = _sincospi(2 * u[1])
    s1, c1 = _sincospi(2 * u[3])
    quad = np.stack([r0 * c0, r0 * s0, r1 * c1, r1 * s1], 1)
    rad = np.stack([r0, r0, r1, r1], 1)
    b = (e % np.uint64(4)).astype(np.int64)
    return (quad[inv, b], rad[inv, b]) if return_radius else quad[inv, b]


def probes(kind, seed, count, numel, first=0):
    """samples first .. first + count - 1 of a call's stream: (count, numel) float64"""
    fn = rademacher if kind[0] == 'r' else gaussian
    return fn(seed, first * numel, count * numel).reshape(count, numel)


def hutchinson(A, V, moments):
    """t[j] = mean_i <A^(j+1) v_i, v_i> over the rows of V"""
    t = np.zeros(moments)
    for v in V:
        m = v
        for j in range(moments):
            m = A @ m
            t[j] += m @ v
    return t / len(V)


def hutchpp(A, S, G, moments, qr=np.linalg.qr):
    """Hutch++ with the sketch probes S and the Hutchinson probes G (rows): Q = orth(A S) by Householder QR,
    G <- (I - Q Q^T) G, t[j] = tr(Q^T A^j Q) + tr(G^T A^j G) / m"""
    m = len(S)
    Q = qr((A @ S.T))[0]                 # (n, m)
    G = G.T - Q @ (Q.T @ G.T)
    t = np.zeros(moments)
    MQ, MG = Q, G
    for j in range(moments):
        MQ, MG = A @ MQ, A @ MG
        t[j] = np.sum(Q * MQ) + np.sum(G * MG) / m
    return t


def power_iteration(A, v, max_iter=512, tol=1e-6):
    mu = np.inf
    for _ in range(max_iter):
        w, v = v, A @ v
        mu0, mu = mu, w @ v
        v = v / np.sqrt(v @ v)
        if abs(mu - mu0) < tol:
            break
    return mu
