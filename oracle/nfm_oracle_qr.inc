/* nfm_oracle_qr.inc -- QR family of the oracle (included by nfm_oracle_body.inc for
 * T = float / double).  TEST INFRASTRUCTURE ONLY.  Restates, per matrix, the operation
 * sequence of /root/reference/nitorch_fastmath/_impl/qr.py (real dtypes).  Matrices are
 * row-major N x N, contiguous batch-major.  Results are compared with the golden vectors
 * to tolerance (norm / dot reductions are summed in index order here, torch's order is
 * unspecified).  Deviations from the reference, all deliberate (SURVEY quirks):
 *   Q7  matvec_sym for n > 4 raises upstream for batched input -> the intended product;
 *   Q8  rq_hessenberg column rotations cover rows 0..k+1 (true R Q) unless `sym`;
 *   Q9  convergence is judged per matrix, with the reference's criterion;
 *   Q9c the public building blocks (everything but eig_sym) guard the range of their sums of squares. */

/* _givens_jit :326-334 */
static inline void FN(givens1)(T x, T y, T *c, T *s)
{
    T nrm = SQRT(x * x + y * y);
    if (nrm == (T)0) { *c = (T)1; *s = (T)0; return; }
    *c = x / nrm;
    *s = -(y / nrm);
}

/* The range guard of the public building blocks (Q9c; shared bit for bit with nfm_qr_core.hpp `sq_in_window`,
 * `givens_guard1`, `householder1<.., GUARD>`).  Upstream normalises by an unscaled sum of squares; outside this
 * window the squares are subnormal or zero (or overflow) and the "unit" vector is not of unit length.  A pair or a
 * vector outside it takes the scaled form; inside it nothing changes, bit for bit.  eig_sym stays unguarded. */
static inline int FN(sq_in_window)(T ss)
{
    const double lo = sizeof(T) == 4 ? 0x1p-100 : 0x1p-900, hi = sizeof(T) == 4 ? 0x1p100 : 0x1p900;
    return (double)ss >= lo && (double)ss <= hi; /* NaN: outside */
}

/* givens1 on the pair divided by its larger magnitude (one component becomes +-1 exactly) */
static inline void FN(givens_scaled1)(T x, T y, T *c, T *s)
{
    T ax = FABS(x), ay = FABS(y);
    T m = ax > ay ? ax : ay;
    if (m == (T)0) { *c = (T)1; *s = (T)0; return; }
    T xs = x / m, ys = y / m;
    T nrm = SQRT(xs * xs + ys * ys);
    *c = xs / nrm;
    *s = -(ys / nrm);
}

static inline void FN(givens_guard1)(T x, T y, T *c, T *s)
{
    if (FN(sq_in_window)(x * x + y * y)) FN(givens1)(x, y, c, s);
    else FN(givens_scaled1)(x, y, c, s);
}

/* rotate the pair (p0[k*st], p1[k*st]), k < len : _givens_apply_* :370-402
 *   tmp = s*a0; a0 = a0*c - s*a1; a1 = a1*c + tmp */
static inline void FN(rot)(T *p0, T *p1, int st, int len, T c, T s)
{
    for (int k = 0; k < len; ++k) {
        T a0 = p0[k * st], a1 = p1[k * st];
        T tmp = s * a0;
        p0[k * st] = a0 * c - s * a1;
        p1[k * st] = a1 * c + tmp;
    }
}

/* householder_ :55-69 ; x (len m) is overwritten by the reflector, returns rho (= alpha) */
static inline T FN(householder1)(int m, T *x, int basis)
{
    T rho = x[basis];
    rho = (rho > (T)0) ? (T)1 : ((rho < (T)0) ? (T)-1 : (T)0); /* sign_ */
    rho = -rho;
    if (rho == (T)0) rho = (T)1;
    T ss = (T)0;
    for (int i = 0; i < m; ++i) ss += x[i] * x[i];
    rho *= SQRT(ss);
    x[basis] -= rho;
    ss = (T)0;
    for (int i = 0; i < m; ++i) ss += x[i] * x[i];
    T nrm = SQRT(ss);
    for (int i = 0; i < m; ++i) {
        T v = x[i] / nrm;
        x[i] = ISFINITE(v) ? v : (T)0;
    }
    return rho;
}

/* householder1 with the range guard: a vector whose sum of squares is outside the window is reflected as
 * x 2^-e, e the exponent of its largest magnitude (exact), and alpha is scaled back (one rounding, only where
 * it is subnormal).  Zero vectors and vectors with an inf or a NaN go through as they are. */
static inline T FN(householder_guard1)(int m, T *x, int basis)
{
    T ss = (T)0, big = (T)0;
    for (int i = 0; i < m; ++i) ss += x[i] * x[i];
    if (FN(sq_in_window)(ss)) return FN(householder1)(m, x, basis);
    for (int i = 0; i < m; ++i) { T v = FABS(x[i]); big = (v > big) ? v : big; }
    if (!(big > (T)0) || !ISFINITE(big)) return FN(householder1)(m, x, basis);
    int e;
    (void)frexp((double)big, &e);
    e -= 1; /* big in [2^e, 2^(e+1)) */
    for (int i = 0; i < m; ++i) x[i] = (T)ldexp((double)x[i], -e);
    T rho = FN(householder1)(m, x, basis);
    return (T)ldexp((double)rho, e);
}

/* apply P = I - 2 u u^T (u of length m) to the trailing rows / columns of the N x N matrix a
 * householder_apply_ :72-106 */
static inline void FN(householder_apply1)(int N, int m, T *a, const T *u, int left, int right)
{
    const int k0 = N - m;
    if (left) { /* a[k0:, :] -= 2 u (u^T a[k0:, :]) */
        for (int c = 0; c < N; ++c) {
            T d = (T)0;
            for (int r = 0; r < m; ++r) d += u[r] * a[(k0 + r) * N + c];
            for (int r = 0; r < m; ++r) a[(k0 + r) * N + c] -= (T)2 * (u[r] * d);
        }
    }
    if (right) { /* a[:, k0:] -= 2 (a[:, k0:] u) u^T */
        for (int r = 0; r < N; ++r) {
            T d = (T)0;
            for (int c = 0; c < m; ++c) d += a[r * N + k0 + c] * u[c];
            for (int c = 0; c < m; ++c) a[r * N + k0 + c] -= (T)2 * (d * u[c]);
        }
    }
}

/* hessenberg_ :117-141 ; upack (may be NULL): reflector k at upack[k*(N-1) .. +N-1-k) */
static inline void FN(hessenberg1)(int N, T *a, T *upack)
{
    T u[NFM_MAXM];
    for (int k = 0; k < N - 2; ++k) {
        const int m = N - k - 1;
        for (int r = 0; r < m; ++r) u[r] = a[(k + 1 + r) * N + k];
        T alpha = FN(householder_guard1)(m, u, 0);
        if (upack) for (int r = 0; r < m; ++r) upack[k * (N - 1) + r] = u[r];
        /* left: a[k+1:, k+1:] -= 2 u (u^T a[k+1:, k+1:]) */
        for (int c = k + 1; c < N; ++c) {
            T d = (T)0;
            for (int r = 0; r < m; ++r) d += u[r] * a[(k + 1 + r) * N + c];
            for (int r = 0; r < m; ++r) a[(k + 1 + r) * N + c] -= (T)2 * (u[r] * d);
        }
        /* right: a[:, k+1:] -= 2 (a[:, k+1:] u) u^T */
        for (int r = 0; r < N; ++r) {
            T d = (T)0;
            for (int c = 0; c < m; ++c) d += a[r * N + k + 1 + c] * u[c];
            for (int c = 0; c < m; ++c) a[r * N + k + 1 + c] -= (T)2 * (d * u[c]);
        }
        a[(k + 1) * N + k] = alpha;
        for (int r = k + 2; r < N; ++r) a[r * N + k] = (T)0;
    }
}

/* hessenberg_sym_lower_ :296-323 (reads/updates the LOWER triangle only); with upper != 0 the
 * same algorithm runs on the transpose (hessenberg_sym_upper_ :280-293).  fill: mirror.
 * guard: the range guard of the reflectors (the public entry point; eig_sym passes 0). */
static inline void FN(hessenberg_sym1)(int N, T *a, int upper, int fill, T *upack, int guard)
{
#define L_(i, j) (upper ? a[(j) * N + (i)] : a[(i) * N + (j)]) /* element (i,j) of the lower view */
    T u[NFM_MAXM], v[NFM_MAXM];
    for (int k = 0; k < N - 2; ++k) {
        const int m = N - k - 1, o = k + 1;
        for (int r = 0; r < m; ++r) u[r] = L_(o + r, k);
        T alpha = guard ? FN(householder_guard1)(m, u, 0) : FN(householder1)(m, u, 0);
        if (upack) for (int r = 0; r < m; ++r) upack[k * (N - 1) + r] = u[r];
        /* v = A_k u using the lower triangle (matvec_sym :201-237) */
        for (int i = 0; i < m; ++i) {
            T y = (T)0;
            for (int j = 0; j < m; ++j) y += (i >= j ? L_(o + i, o + j) : L_(o + j, o + i)) * u[j];
            v[i] = y;
        }
        T d = (T)0;
        for (int i = 0; i < m; ++i) d += u[i] * v[i];
        for (int i = 0; i < m; ++i) v[i] = (v[i] - u[i] * d) * (T)2;
        /* A_k[lower] -= (u v^T + v u^T)[lower]  (outer_sym :240-277) */
        for (int i = 0; i < m; ++i)
            for (int j = 0; j <= i; ++j) {
                T w = (i == j) ? (u[i] * v[i]) * (T)2 : (u[j] * v[i] + v[j] * u[i]);
                if (upper) a[(o + j) * N + (o + i)] -= w; else a[(o + i) * N + (o + j)] -= w;
            }
        if (upper) { a[k * N + o] = alpha; for (int r = k + 2; r < N; ++r) a[k * N + r] = (T)0; }
        else { a[o * N + k] = alpha; for (int r = k + 2; r < N; ++r) a[r * N + k] = (T)0; }
    }
#undef L_
    if (fill)
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < i; ++j) {
                if (upper) a[i * N + j] = a[j * N + i]; else a[j * N + i] = a[i * N + j];
            }
}

/* qr_hessenberg_ :432-454 ; a -> R in place, q = Q */
static inline void FN(qr_hessenberg1)(int N, T *a, T *q)
{
    for (int i = 0; i < N * N; ++i) q[i] = (T)0;
    for (int i = 0; i < N; ++i) q[i * N + i] = (T)1;
    for (int k = 0; k < N - 1; ++k) {
        T c, s;
        FN(givens_guard1)(a[k * N + k], a[(k + 1) * N + k], &c, &s);
        FN(rot)(a + k * N + k, a + (k + 1) * N + k, 1, N - k, c, s);  /* rows k, k+1, columns k: */
        FN(rot)(q + k, q + k + 1, N, k + 2, c, s);                    /* columns k, k+1, rows :k+2 */
    }
}

/* one RQ step on the leading m x m block of the N x N matrix a (and column rotations of
 * the N-row matrix u, ncols = m): _rq_hessenberg(_vectors)_jit_ :457-522
 * guard: the range guard of the rotations (the public entry point; eig_sym's sweeps pass 0) */
static inline void FN(rq_step)(int N, int m, T *a, T *u, int sym, int true_rq, int guard)
{
    T lc[NFM_MAXM], ls[NFM_MAXM];
    for (int k = 0; k < m - 1; ++k) {
        if (guard) FN(givens_guard1)(a[k * N + k], a[(k + 1) * N + k], &lc[k], &ls[k]);
        else FN(givens1)(a[k * N + k], a[(k + 1) * N + k], &lc[k], &ls[k]);
        int len = sym ? (k + 3 <= m ? 3 : m - k) : m - k;
        FN(rot)(a + k * N + k, a + (k + 1) * N + k, 1, len, lc[k], ls[k]);
    }
    for (int k = 0; k < m - 1; ++k) {
        int r0 = (true_rq && !sym) ? 0 : (k - 1 > 0 ? k - 1 : 0);
        FN(rot)(a + r0 * N + k, a + r0 * N + k + 1, N, k + 2 - r0, lc[k], ls[k]);
        if (u) FN(rot)(u + k, u + k + 1, N, N, lc[k], ls[k]);
    }
}

/* _wilkinson :558-569 on the trailing 2x2 of the active m x m block */
static inline T FN(wilkinson1)(int N, int m, const T *h)
{
    T h0 = h[(m - 2) * N + (m - 2)], h1 = h[(m - 1) * N + (m - 1)];
    T b2 = h[(m - 1) * N + (m - 2)];
    b2 = b2 * b2;
    T d = (h0 - h1) / (T)2;
    T s = (d > (T)0) ? (T)1 : ((d < (T)0) ? (T)-1 : (T)1);
    d = FABS(d) + SQRT(d * d + b2);
    if (d == (T)0) d = (T)1;
    return h1 - s * b2 / d;
}

/* _qr_explicit(_vectors)_jit_ :572-656 with sym = True, per-matrix convergence */
static inline void FN(qr_explicit1)(int N, T *h, T *u, int max_iter, double tol, int *sweeps)
{
    /* sweeps (optional, N ints): QR sweeps spent on each active block size m (index m - 1) */
    if (u) {
        for (int i = 0; i < N * N; ++i) u[i] = (T)0;
        for (int i = 0; i < N; ++i) u[i * N + i] = (T)1;
    }
    for (int m = N; m >= 2; --m) {
        double sos_prev = 0.0;
        for (int it = 0; it < max_iter; ++it) {
            if (sweeps) sweeps[m - 1] += 1;
            T sigma = FN(wilkinson1)(N, m, h);
            for (int i = 0; i < m; ++i) h[i * N + i] -= sigma;
            FN(rq_step)(N, m, h, u, 1, 0, 0);
            for (int i = 0; i < m; ++i) h[i * N + i] += sigma;
            T bb = FABS(h[(m - 1) * N + (m - 2)]), a0 = FABS(h[(m - 1) * N + (m - 1)]);
            T a1 = FABS(h[(m - 2) * N + (m - 2)]);
            T sos_lower = bb * bb, sos_diag = a0 * a0 + a1 * a1;
            /* `<=` (upstream `<`) and the NaN test: a zero off-diagonal or NaNs cannot change any more;
               upstream spins through max_iter identical iterations there (same result).  `<=` also fires
               when BOTH squares underflow to zero with the entries themselves non-zero (0 <= tol * 0): the
               stage then deflates unconverged.  The scale rule of eig_prescale1 keeps whole records out
               of that range; tiny blocks inside a unit-scale record can still meet it
               (tests/_eig_ref.py REFERENCE_EXCEEDS). */
            if ((double)sos_lower <= tol * (double)sos_diag || sos_lower != sos_lower) {
                for (int j = 0; j < m - 1; ++j) h[(m - 1) * N + j] = (T)0;
                break;
            }
            if (!u) { /* the "stuck" exit exists only in the no-vectors variant :648-653 */
                double sos_new = (double)(sos_lower / sos_diag);
                if (sos_prev != 0.0 && fabs(sos_prev - sos_new) < (tol * 1e-3) * sos_prev) break;
                sos_prev = sos_new;
            }
        }
    }
}

/* The scale rule of eig_sym (not upstream's; shared bit for bit with nfm_qr_core.hpp `eig_prescale1`).
 * The sweeps square matrix entries in T (Householder's sum of squares, Wilkinson's b^2, Givens' x^2 + y^2, the
 * convergence test e^2 <= tol (d0^2 + d1^2)), so their range is the square root of T's: outside it the squares
 * underflow or overflow and the iteration deflates at once on 0 <= tol * 0, or returns NaN.  A record whose
 * largest entry (over the triangle that is read) has an exponent outside the window [lo, hi] is therefore scaled
 * by the exact power of two that brings that entry into [1, 2), solved, and its eigenvalues are scaled back (one
 * rounding, and only where the result is subnormal); the eigenvectors do not depend on the scale.  Inside the
 * window nothing is touched: the same bits as without the rule.  Zero records and records with an inf or a
 * NaN in that triangle are left alone.
 * Returns the shift k (entries were multiplied by 2^k), 0 for none. */
#define NFM_EIG_WINDOW_LO (sizeof(T) == 4 ? -50 : -480)
#define NFM_EIG_WINDOW_HI (sizeof(T) == 4 ? 56 : 480)
static inline int FN(eig_prescale1)(int N, T *a, int upper)
{
    T mx = (T)0;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j <= i; ++j) {
            T v = FABS(upper ? a[j * N + i] : a[i * N + j]);
            if (!ISFINITE(v)) return 0;
            mx = (v > mx) ? v : mx;
        }
    if (!(mx > (T)0)) return 0;
    int e;
    (void)frexp((double)mx, &e); /* mx = f 2^e, f in [0.5, 1): exact for both types, subnormals included */
    e -= 1;                      /* mx in [2^e, 2^(e+1)) */
    if (e >= NFM_EIG_WINDOW_LO && e <= NFM_EIG_WINDOW_HI) return 0;
    for (int i = 0; i < N * N; ++i) a[i] = (T)ldexp((double)a[i], -e); /* exact, or one rounding into the subnormals */
    return -e;
}

/* _fwd_eig_sym :665-681 */
static inline void FN(eig_sym1)(int N, T *a, int upper, int compute_u, int max_iter, double tol, T *vals,
                                T *vecs, int *sweeps)
{
    T upack[NFM_MAXM * NFM_MAXM];
    const int shift = FN(eig_prescale1)(N, a, upper);
    FN(hessenberg_sym1)(N, a, upper, 1, compute_u ? upack : NULL, 0);
    FN(qr_explicit1)(N, a, compute_u ? vecs : NULL, max_iter, tol, sweeps);
    if (compute_u) /* householder_apply_(u, q, side='left', inverse=True): reflectors in reverse */
        for (int k = N - 3; k >= 0; --k) FN(householder_apply1)(N, N - k - 1, vecs, upack + k * (N - 1), 1, 0);
    for (int i = 0; i < N; ++i) vals[i] = a[i * N + i];
    if (shift != 0)
        for (int i = 0; i < N; ++i) vals[i] = (T)ldexp((double)vals[i], -shift);
}

/* ------------------------------- batch drivers ------------------------------- */
static int FN(nfm_oracle_qr_givens)(int64_t n, const T *x, const T *y, T *c, T *s)
{
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < n; ++b) FN(givens_guard1)(x[b], y[b], &c[b], &s[b]);
    return 0;
}

/* c, s: (n, N) -- one coefficient per position along the rotated rows / columns */
static int FN(nfm_oracle_qr_givens_apply)(int N, int64_t n, int side, int i, int j, T *a, const T *c, const T *s)
{
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < n; ++b) {
        T *A = a + b * N * N;
        if (side == 0 || side == 2)
            for (int k = 0; k < N; ++k) FN(rot)(A + i * N + k, A + j * N + k, 1, 1, c[b * N + k], s[b * N + k]);
        if (side == 1 || side == 2)
            for (int k = 0; k < N; ++k) FN(rot)(A + k * N + i, A + k * N + j, 1, 1, c[b * N + k], s[b * N + k]);
    }
    return 0;
}

static int FN(nfm_oracle_qr_householder)(int N, int64_t n, int basis, T *x, T *alpha)
{
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < n; ++b) alpha[b] = FN(householder_guard1)(N, x + b * N, basis);
    return 0;
}

static int FN(nfm_oracle_qr_householder_apply)(int N, int m, int64_t n, int side, T *a, const T *u)
{
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < n; ++b)
        FN(householder_apply1)(N, m, a + b * N * N, u + b * m, side == 0 || side == 2, side == 1 || side == 2);
    return 0;
}

static int FN(nfm_oracle_qr_hessenberg)(int N, int64_t n, T *a, T *upack)
{
    const int us = (N - 2 > 0 ? N - 2 : 0) * (N - 1);
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < n; ++b) FN(hessenberg1)(N, a + b * N * N, upack ? upack + b * us : NULL);
    return 0;
}

static int FN(nfm_oracle_qr_hessenberg_sym)(int N, int64_t n, int upper, int fill, T *a, T *upack)
{
    const int us = (N - 2 > 0 ? N - 2 : 0) * (N - 1);
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < n; ++b)
        FN(hessenberg_sym1)(N, a + b * N * N, upper, fill, upack ? upack + b * us : NULL, 1);
    return 0;
}

static int FN(nfm_oracle_qr_qr_hessenberg)(int N, int64_t n, T *a, T *q)
{
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < n; ++b) FN(qr_hessenberg1)(N, a + b * N * N, q + b * N * N);
    return 0;
}

static int FN(nfm_oracle_qr_rq_hessenberg)(int N, int64_t n, int sym, int true_rq, T *a, T *u)
{
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < n; ++b) FN(rq_step)(N, N, a + b * N * N, u ? u + b * N * N : NULL, sym, true_rq, 1);
    return 0;
}

static int FN(nfm_oracle_qr_eig_sym)(int N, int64_t n, int upper, int compute_u, int max_iter, double tol, T *a,
                                     T *vals, T *vecs, int *sweeps)
{
    if (sweeps)
        for (int64_t i = 0; i < n * N; ++i) sweeps[i] = 0;
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < n; ++b)
        FN(eig_sym1)(N, a + b * N * N, upper, compute_u, max_iter, tol, vals + b * N,
                     compute_u ? vecs + b * N * N : NULL, sweeps ? sweeps + b * N : NULL);
    return 0;
}
