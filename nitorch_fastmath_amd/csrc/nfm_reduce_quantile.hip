// nfm_reduce_quantile.hip -- several quantiles of every row of a contiguous (rows, red) array by the radix
// selection of nfm_reduce_median.hip, generalised from the rank (count - 1) / 2 to up to kMaxQ arbitrary ranks
// per launch plus the neighbouring order statistic that interpolation needs.  No counterpart in the reference
// (its one order statistic is `median`, `reduce.py:384-428`); the definition is the one of DESIGN 4.5b:
//
//   count = elements of the row (omitnan: its non-NaN elements); a NaN with omitnan = 0, or count = 0: NaN.
//   p = fl64(q * (count - 1)), lo = floor(p), hi = ceil(p), w = p - lo; keys ordered as the median orders them.
//   lower: v_lo; higher: v_hi; nearest: rank rint(p) (half to even); midpoint: linear with w = 0.5;
//   linear: v_lo when v_lo == v_hi (no arithmetic: equal infinities stay), else in float64
//           w < 0.5 ? a + w (b - a) : b - (b - a) (1 - w), rounded once to the dtype.
//
// q travels BY VALUE in the kernel arguments (QArgs): nothing is copied to the device, a call can be captured.
//
//   red <= 32:   8 / 16 / 32 lanes per row, ranks counted directly (median_tiny_kernel); per q the lanes of
//                rank lo and hi are found by ballot;
//   red <= 1024: the row in registers, a 256-bin LDS histogram per row (median_rows_kernel); the digit loop
//                runs once per q on the keys in registers; v_hi = v_lo when #(keys <= key_lo) > lo + 1, else
//                the smallest key above key_lo -- two reductions over the group;
//   longer rows: one streaming pass per 11-bit digit serves ALL ranks: the first pass shares one histogram
//                (no prefix chosen yet), later passes keep one 2048-bin LDS histogram per rank state (8 KiB
//                each: kMaxQ = 8 fills the 64 KiB a workgroup may ask for) and count an element in every state
//                whose prefix it matches; one wavefront per row resolves all states between passes.  One
//                successor pass then collects per state #(keys <= key_lo), the smallest key above key_lo and,
//                when positions are wanted, the first position of key_lo (a further pass finds the first
//                position of key_hi: only the autograd route asks for it).
//
// Shared with the median through nfm_reduce_select.hpp: above(), the chunk walk, the digit pick, the counting rule
// (where it leaves a kernel's code as it was) and the launch ladders.  The two register forms above and the
// first-pass histogram repeat the text of the median's kernels: built from common blocks they were scheduled
// differently and measurably slower (profiles/select_refactor.md).
#include "nfm_reduce_select.hpp"

namespace nfm {
namespace qnt {

// the selection building blocks (nfm_reduce_select.hpp)
using med::above;
using med::Key;
using med::kLongBins;
using med::launch_rows;
using med::launch_tiny;
using med::LongDigits;
using med::pick_digit_n;
using med::row_count;
using med::stream_chunk;
using med::ull;

constexpr int kMaxQ = 8; // rank states of one launch: 8 x 8 KiB of LDS histograms
struct QArgs {
    double q[kMaxQ];
};

// q[s] by selects: a dynamic index into the by-value argument could cost a private copy
__device__ __forceinline__ double q_at(const QArgs &qa, int s)
{
    double v = qa.q[0];
#pragma unroll
    for (int i = 1; i < kMaxQ; ++i) v = s == i ? qa.q[i] : v;
    return v;
}

// the ranks a quantile selects and the weight of the upper one: THE rank routine of every form, and of
// nfm_reduce_quantile_plan_host.  count >= 1, 0 <= q <= 1 (so p <= count - 1: count - 1 < 2^53 is exact).
struct Plan {
    ull lo, hi;
    double w;
};
__host__ __device__ inline Plan plan_of(double q, ull count, int interp)
{
#pragma clang fp contract(off) // p is ROUNDED before w is taken: fma(q, count - 1, -floor) would be another w
    Plan pl{0, 0, 0.0};
    if (count == 0) return pl;
    const double p = q * (double)(count - 1); // one multiplication, one rounding
    const double fl = __builtin_floor(p);
    pl.lo = (ull)fl;
    pl.hi = (ull)__builtin_ceil(p);
    pl.w = p - fl; // exact
    if (interp == NFM_QUANTILE_LOWER) {
        pl.hi = pl.lo;
        pl.w = 0.0;
    } else if (interp == NFM_QUANTILE_HIGHER) {
        pl.lo = pl.hi;
        pl.w = 0.0;
    } else if (interp == NFM_QUANTILE_NEAREST) {
        pl.lo = pl.hi = (ull)__builtin_rint(p); // round-to-nearest mode: half to even
        pl.w = 0.0;
    } else if (interp == NFM_QUANTILE_MIDPOINT) {
        pl.w = 0.5;
    }
    return pl;
}

template <typename T>
__device__ __forceinline__ T combine(typename Key<T>::U klo, typename Key<T>::U khi, double w)
{
#pragma clang fp contract(off)
    using K = Key<T>;
    if (klo == khi) return K::back(klo); // no arithmetic: two equal infinities give that infinity
    const double a = (double)K::back(klo), b = (double)K::back(khi);
    const double d = b - a;
    const double r = w < 0.5 ? a + w * d : b - d * (1.0 - w);
    return (T)r;
}

// ---------------------------------------------------------------------------------------------
// tiny rows (red <= 32): G lanes per row, one element per lane, the rank of every element counted directly
template <typename T, int G>
__global__ __launch_bounds__(256) void quantile_tiny_kernel(const T *__restrict__ x, int64_t rows, int red, int omitnan,
                                                            int interp, int nq, QArgs qa, T *__restrict__ val,
                                                            int64_t *__restrict__ pos)
{
    using K = Key<T>;
    using U = typename K::U;
    constexpr int RPW = 64 / G; // rows per wavefront
    const int lane = threadIdx.x & 63, j = lane % G, gbase = lane - j;
    const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / G;
    const bool live = row < rows && j < red;
    const T v = live ? NFM_LDG(x + row * red + j) : T(0);
    const U key = live ? K::of(v) : ~U(0);
    unsigned nan = (live && v != v) ? 1u : 0u;
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) nan += __shfl_xor(nan, off, 64);
    // (the rule of row_count, written out: through it this kernel's code is scheduled differently)
    const unsigned count = omitnan ? (unsigned)red - nan : (unsigned)red;
    const bool want_nan = (!omitnan && nan > 0) || count == 0;
    unsigned rank = 0;
    for (int t = 0; t < red; ++t) { // red is uniform; positions beyond it hold nothing
        const U kt = __shfl(key, gbase + t, 64);
        rank += (kt < key || (kt == key && t < j)) ? 1u : 0u;
    }
    const ull gmask = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << gbase;
    for (int s = 0; s < nq; ++s) {
        const Plan pl = plan_of(q_at(qa, s), count, interp);
        // exactly one live lane of the row holds each rank below count (NaN keys are the largest)
        const ull hit_lo = __ballot(live && rank == (unsigned)pl.lo) & gmask;
        const ull hit_hi = __ballot(live && rank == (unsigned)pl.hi) & gmask;
        const U klo = __shfl(key, hit_lo ? __builtin_ctzll(hit_lo) : gbase, 64);
        const U khi = __shfl(key, hit_hi ? __builtin_ctzll(hit_hi) : gbase, 64);
        const ull same_lo = __ballot(live && key == klo) & gmask;
        const ull same_hi = __ballot(live && key == khi) & gmask;
        if (j == 0 && row < rows) {
            const int64_t o = (int64_t)s * rows + row;
            val[o] = want_nan ? (T)__builtin_nanf("") : combine<T>(klo, khi, pl.w);
            if (pos) {
                pos[2 * o] = (want_nan || !same_lo) ? 0 : (int64_t)(__builtin_ctzll(same_lo) - gbase);
                pos[2 * o + 1] = (want_nan || !same_hi) ? 0 : (int64_t)(__builtin_ctzll(same_hi) - gbase);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// short rows (red <= 1024): G lanes per row, E keys per lane (median_rows_kernel); the row is read once,
// the digit loop runs once per q on the keys in registers
template <typename T, int E, int G>
__global__ __launch_bounds__(256) void quantile_rows_kernel(const T *__restrict__ x, int64_t rows, int red, int omitnan,
                                                            int interp, int nq, QArgs qa, T *__restrict__ val,
                                                            int64_t *__restrict__ pos)
{
    using K = Key<T>;
    using U = typename K::U;
    constexpr int RPW = 64 / G; // rows per wavefront
    constexpr int NB = 256 / G; // histogram bins owned by a lane
    __shared__ unsigned hist_all[4][RPW][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane / G, j = lane % G;
    unsigned *hist = hist_all[w][g];
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + w) * RPW;
    if (row0 >= rows) return; // whole wavefronts leave: no barrier below is workgroup-wide
    const int64_t row = row0 + g;
    const bool live_row = row < rows;
    const T *p = x + (live_row ? row : row0) * red; // groups past the end redo the first row (never stored)
    U key[E];
    unsigned nan = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int jj = j + G * e;
        const T v = jj < red ? NFM_LDG(p + jj) : T(0);
        key[e] = K::of(v);
        nan += (jj < red && v != v) ? 1u : 0u;
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) nan += __shfl_xor(nan, off, G);
    const auto [count, want_nan] = row_count((unsigned)red, nan, omitnan);
    for (int s = 0; s < nq; ++s) {
        // what derives from the keys alone (the digits of every pass) stays inside the loop: hoisted out of it,
        // those values cost three times the registers of median_rows_kernel and half its wavefronts per SIMD
#pragma unroll
        for (int e = 0; e < E; ++e) asm volatile("" : "+v"(key[e]));
        const Plan pl = plan_of(q_at(qa, s), count, interp);
        unsigned k = (unsigned)pl.lo;
        U prefix = 0;
#pragma unroll
        for (int d = K::digits - 1; d >= 0; --d) {
            const int shift = 8 * d;
#pragma unroll
            for (int b = 0; b < NB; ++b) hist[NB * j + b] = 0;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int jj = j + G * e;
                const bool in = jj < red && above(key[e], d, K::digits) == prefix;
                if (in) atomicAdd(&hist[(unsigned)(key[e] >> shift) & 255u], 1u);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // the digit whose cumulative count passes k, inside the group (rows with a NaN result have no
            // such digit: they go through the motions and are overridden below)
            unsigned cnt[NB], mine = 0;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                cnt[b] = hist[NB * j + b];
                mine += cnt[b];
            }
            unsigned incl = mine;
#pragma unroll
            for (int off = 1; off < G; off <<= 1) {
                const unsigned o = __shfl_up(incl, off, G);
                if (j >= off) incl += o;
            }
            const unsigned before = incl - mine;
            const bool here = before <= k && k < before + mine;
            const ull gm = (__ballot(here) >> (g * G)) & (G == 64 ? ~0ull : ((1ull << (G % 64)) - 1ull));
            const int src = gm ? __builtin_ctzll(gm) : G - 1;
            unsigned digit = 0, kk = k;
            if (j == src) {
                unsigned r = k - before, dd = 0;
#pragma unroll
                for (int b = 0; b < NB - 1; ++b)
                    if (dd == (unsigned)b && r >= cnt[b]) {
                        r -= cnt[b];
                        dd = b + 1;
                    }
                digit = NB * j + dd;
                kk = r;
            }
            digit = __shfl(digit, src, G);
            k = __shfl(kk, src, G);
            prefix = (prefix << 8) | (U)digit;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        const U klo = prefix;
        // the next order statistic: key_lo again while more than lo + 1 keys are <= it, else the smallest above
        unsigned cle = 0;
        U succ = ~U(0);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int jj = j + G * e;
            const bool in = jj < red;
            cle += (in && key[e] <= klo) ? 1u : 0u;
            succ = (in && key[e] > klo && key[e] < succ) ? key[e] : succ;
        }
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {
            cle += __shfl_xor(cle, off, G);
            const U o = __shfl_xor(succ, off, G);
            succ = o < succ ? o : succ;
        }
        const U khi = (pl.hi == pl.lo || (ull)cle > pl.lo + 1) ? klo : succ;
        int first_lo = 0x7fffffff, first_hi = 0x7fffffff;
        if (pos) { // uniform
#pragma unroll
            for (int e = E - 1; e >= 0; --e) {
                const int jj = j + G * e;
                if (jj < red && key[e] == klo) first_lo = jj;
                if (jj < red && key[e] == khi) first_hi = jj;
            }
#pragma unroll
            for (int off = G / 2; off > 0; off >>= 1) {
                const int o = __shfl_xor(first_lo, off, G), o2 = __shfl_xor(first_hi, off, G);
                first_lo = o < first_lo ? o : first_lo;
                first_hi = o2 < first_hi ? o2 : first_hi;
            }
        }
        if (j == 0 && live_row) {
            const int64_t o = (int64_t)s * rows + row;
            val[o] = want_nan ? (T)__builtin_nanf("") : combine<T>(klo, khi, pl.w);
            if (pos) {
                pos[2 * o] = (want_nan || first_lo == 0x7fffffff) ? 0 : first_lo;
                pos[2 * o + 1] = (want_nan || first_hi == 0x7fffffff) ? 0 : first_hi;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// long rows.  Workspace: QRow[rows], QState[rows * nq], then the global histograms [rows * nq][2048] of 64-bit
// counts (the first pass fills only the histogram of state 0: it is shared)
struct QRow {
    ull nan;      // NaNs in the row (counted by the first pass)
    int want_nan; // every quantile of the row is NaN
    int pad;
};
struct QState {
    ull prefix;   // digits chosen so far; in the end key_lo
    ull k;        // rank still to resolve inside the prefix
    ull cnt_le;   // #(keys <= key_lo)
    ull succ;     // smallest key above key_lo (~0: none); after quantile_resolve_kernel: key_hi
    ull first_lo; // first position of key_lo (>= red: not found)
    ull first_hi; // first position of key_hi
};
static_assert(sizeof(QRow) == 16 && sizeof(QState) == 48, "workspace layout");

static size_t workspace_need(int64_t rows, int nq)
{
    return (size_t)rows * (sizeof(QRow) + (size_t)nq * (sizeof(QState) + kLongBins * sizeof(ull)));
}

// first pass: no prefix yet, so every rank state reads the same histogram (that of state 0); counts the NaNs
template <typename T>
__global__ __launch_bounds__(256) void quantile_hist0_kernel(const T *__restrict__ x, int64_t red, int64_t chunk, int nq,
                                                             QRow *__restrict__ ri, ull *__restrict__ ghist)
{
    using K = Key<T>;
    using U = typename K::U;
    using D = LongDigits<T>;
    __shared__ unsigned hist[kLongBins];
    __shared__ unsigned nan_s;
    const int64_t row = blockIdx.y;
#pragma unroll
    for (int b = 0; b < kLongBins / 256; ++b) hist[threadIdx.x + 256 * b] = 0;
    if (threadIdx.x == 0) nan_s = 0;
    __syncthreads();
    constexpr int shift = D::shift(0);
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < red ? lo + chunk : red;
    unsigned nan = 0;
    stream_chunk<T>(x + row * red, lo, hi, [&](T v, int64_t) __attribute__((always_inline)) {
        const U key = K::of(v);
        nan += (v != v) ? 1u : 0u;
        atomicAdd(&hist[(unsigned)(key >> shift)], 1u);
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nan += __shfl_xor(nan, off, 64);
    if ((threadIdx.x & 63) == 0 && nan) atomicAdd(&nan_s, nan);
    __syncthreads();
    ull *gh = ghist + row * nq * kLongBins;
#pragma unroll
    for (int b = 0; b < kLongBins / 256; ++b) {
        const unsigned c = hist[threadIdx.x + 256 * b];
        if (c) atomicAdd(&gh[threadIdx.x + 256 * b], (ull)c); // (a block's chunk < 2^32)
    }
    if (threadIdx.x == 0 && nan_s) atomicAdd(&ri[row].nan, (ull)nan_s);
}

// later passes: one LDS histogram per rank state (nq * 8 KiB of dynamic LDS); an element is counted in every
// state whose prefix it matches
// NQ = nq rounded up to 1 / 2 / 4 / 8: the per-element loop over the states is unrolled at that length (at NQ = 1
// it is the median's loop)
template <typename T, int NQ>
__global__ __launch_bounds__(256) void quantile_hist_kernel(const T *__restrict__ x, int64_t red, int64_t chunk, int pass,
                                                            int nq, const QRow *__restrict__ ri,
                                                            const QState *__restrict__ st, ull *__restrict__ ghist)
{
    using K = Key<T>;
    using U = typename K::U;
    using D = LongDigits<T>;
    extern __shared__ unsigned qhist[]; // [nq][kLongBins]
    const int64_t row = blockIdx.y;
    if (ri[row].want_nan) return;
    const int nbins = nq * kLongBins;
    for (int b = threadIdx.x; b < nbins; b += 256) qhist[b] = 0;
    U prefix[NQ];
#pragma unroll
    for (int s = 0; s < NQ; ++s) prefix[s] = s < nq ? (U)st[row * nq + s].prefix : U(0);
    __syncthreads();
    const int shift = D::shift(pass), width = D::width(pass);
    const int up = shift + width; // bits above this digit: chosen already (pass >= 1: never the full width)
    const unsigned mask = (1u << width) - 1u;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < red ? lo + chunk : red;
    stream_chunk<T>(x + row * red, lo, hi, [&](T v, int64_t) __attribute__((always_inline)) {
        const U key = K::of(v);
        const U top = (U)(key >> up);
        const unsigned dg = (unsigned)(key >> shift) & mask;
#pragma unroll
        for (int s = 0; s < NQ; ++s)
            if ((NQ == 1 || s < nq) && top == prefix[s]) atomicAdd(&qhist[s * kLongBins + dg], 1u);
    });
    __syncthreads();
    ull *gh = ghist + row * nq * kLongBins;
    for (int b = threadIdx.x; b < nbins; b += 256) {
        const unsigned c = qhist[b];
        if (c) atomicAdd(&gh[b], (ull)c);
    }
}

// one wavefront per row: choose this pass's digit of every rank state, clear the histograms for the next pass
template <typename T>
__global__ __launch_bounds__(64) void quantile_pick_kernel(int64_t red, int pass, int omitnan, int interp, int nq, QArgs qa,
                                                           QRow *__restrict__ ri, QState *__restrict__ st,
                                                           ull *__restrict__ ghist)
{
    using D = LongDigits<T>;
    constexpr int NB = kLongBins / 64;
    const int64_t row = blockIdx.x;
    const int lane = threadIdx.x;
    QRow r = ri[row];
    const auto [count, want_nan] = row_count((ull)red, r.nan, omitnan);
    if (pass == 0) {
        r.want_nan = want_nan ? 1 : 0;
        if (lane == 0) ri[row].want_nan = r.want_nan;
    }
    if (r.want_nan) return; // no later pass touches the row
    ull *gh = ghist + row * nq * kLongBins + NB * lane;
    ull cnt[NB];
    if (pass == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            cnt[b] = gh[b];
            gh[b] = 0;
        }
    }
    for (int s = 0; s < nq; ++s) {
        QState qs;
        if (pass == 0) {
            qs.prefix = 0;
            qs.k = plan_of(q_at(qa, s), count, interp).lo;
            qs.cnt_le = 0;
            qs.succ = ~0ull;
            qs.first_lo = qs.first_hi = ~0ull;
        } else {
            qs = st[row * nq + s];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                cnt[b] = gh[(int64_t)s * kLongBins + b];
                gh[(int64_t)s * kLongBins + b] = 0;
            }
        }
        ull k = qs.k;
        const unsigned digit = pick_digit_n<NB>(cnt, k);
        qs.k = k;
        qs.prefix = (qs.prefix << D::width(pass)) | digit;
        if (lane == 0) st[row * nq + s] = qs;
    }
}

// the successor pass: per rank state #(keys <= key_lo), the smallest key above key_lo and (want_pos) the first
// position of key_lo.  which = 1: the first position of key_hi instead (after quantile_resolve_kernel)
template <typename T, int NQ>
__global__ __launch_bounds__(256) void quantile_succ_kernel(const T *__restrict__ x, int64_t red, int64_t chunk, int nq,
                                                            int want_pos, int which, const QRow *__restrict__ ri,
                                                            QState *__restrict__ st)
{
    using K = Key<T>;
    using U = typename K::U;
    const int64_t row = blockIdx.y;
    if (ri[row].want_nan) return;
    U kq[NQ], succ[NQ];
    unsigned cle[NQ];
    ull first[NQ];
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
        kq[s] = s < nq ? (U)(which ? st[row * nq + s].succ : st[row * nq + s].prefix) : U(0);
        succ[s] = ~U(0);
        cle[s] = 0;
        first[s] = ~0ull;
    }
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < red ? lo + chunk : red;
    stream_chunk<T>(x + row * red, lo, hi, [&](T v, int64_t j) __attribute__((always_inline)) {
        const U key = K::of(v);
#pragma unroll
        for (int s = 0; s < NQ; ++s) {
            if (NQ == 1 || s < nq) {
                if (!which) {
                    cle[s] += key <= kq[s] ? 1u : 0u;
                    succ[s] = (key > kq[s] && key < succ[s]) ? key : succ[s];
                }
                if (want_pos && key == kq[s] && (ull)j < first[s]) first[s] = (ull)j;
            }
        }
    });
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
        if (s < nq) { // uniform
            QState *q = st + row * nq + s;
            if (!which) {
                unsigned c = cle[s];
                U m = succ[s];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    c += __shfl_xor(c, off, 64);
                    const U o = __shfl_xor(m, off, 64);
                    m = o < m ? o : m;
                }
                if ((threadIdx.x & 63) == 0) {
                    if (c) atomicAdd(&q->cnt_le, (ull)c);
                    if (m != ~U(0)) atomicMin(&q->succ, (ull)m);
                }
            }
            if (want_pos) {
                ull f = first[s];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const ull o = __shfl_xor(f, off, 64);
                    f = o < f ? o : f;
                }
                if ((threadIdx.x & 63) == 0 && f != ~0ull) atomicMin(which ? &q->first_hi : &q->first_lo, f);
            }
        }
    }
}

// one thread per (row, state): key_hi from the counts of the successor pass, left in QState::succ
__global__ void quantile_resolve_kernel(int64_t rows, int64_t red, int omitnan, int interp, int nq, QArgs qa,
                                        const QRow *__restrict__ ri, QState *__restrict__ st)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * nq) return;
    const int64_t row = i / nq;
    const int s = (int)(i - row * nq);
    if (ri[row].want_nan) return;
    const ull count = omitnan ? (ull)red - ri[row].nan : (ull)red; // (row_count; the NaN count is loaded only when omitted)
    const Plan pl = plan_of(q_at(qa, s), count, interp);
    QState q = st[i];
    st[i].succ = (pl.hi == pl.lo || q.cnt_le > pl.lo + 1) ? q.prefix : q.succ;
}

// one thread per (row, state): combine and store.  have_hi: QState::succ holds key_hi (else key_hi = key_lo)
template <typename T>
__global__ void quantile_final_kernel(int64_t rows, int64_t red, int omitnan, int interp, int nq, QArgs qa, int have_hi,
                                      int pos_hi, const QRow *__restrict__ ri, const QState *__restrict__ st,
                                      T *__restrict__ val, int64_t *__restrict__ pos)
{
    using U = typename Key<T>::U;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * nq) return;
    const int64_t row = i / nq;
    const int s = (int)(i - row * nq);
    const int64_t o = (int64_t)s * rows + row;
    if (ri[row].want_nan) {
        val[o] = (T)__builtin_nanf("");
        if (pos) pos[2 * o] = pos[2 * o + 1] = 0;
        return;
    }
    const ull count = omitnan ? (ull)red - ri[row].nan : (ull)red; // (row_count; the NaN count is loaded only when omitted)
    const Plan pl = plan_of(q_at(qa, s), count, interp);
    const QState q = st[i];
    const U klo = (U)q.prefix, khi = have_hi ? (U)q.succ : klo;
    val[o] = combine<T>(klo, khi, pl.w);
    if (pos) {
        const ull flo = q.first_lo, fhi = (pos_hi && khi != klo) ? q.first_hi : flo;
        pos[2 * o] = flo >= (ull)red ? 0 : (int64_t)flo;
        pos[2 * o + 1] = fhi >= (ull)red ? 0 : (int64_t)fhi;
    }
}

template <typename T>
static int run(int omitnan, int interp, int64_t rows, int64_t red, int nq, const QArgs &qa, bool need_hi, const void *x,
               void *ws, size_t ws_bytes, void *val, void *pos, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    const T *xp = static_cast<const T *>(x);
    T *vp = static_cast<T *>(val);
    int64_t *pp = static_cast<int64_t *>(pos);
    if (red <= 32)
        return launch_tiny(rows, red, [&](auto, auto g, unsigned nblk) {
            hipLaunchKernelGGL((quantile_tiny_kernel<T, g()>), dim3(nblk), dim3(256), 0, s, xp, rows, (int)red, omitnan,
                               interp, nq, qa, vp, pp);
        });
    if (red <= med::kShortMax)
        return launch_rows(rows, red, [&](auto e, auto g, unsigned nblk) {
            hipLaunchKernelGGL((quantile_rows_kernel<T, e(), g()>), dim3(nblk), dim3(256), 0, s, xp, rows, (int)red,
                               omitnan, interp, nq, qa, vp, pp);
        });
    if (rows > 65535) return NFM_ESIZE; // grid.y; the facade splits (long rows are few)
    const size_t need = workspace_need(rows, nq);
    if (ws == nullptr || ws_bytes < need) return NFM_EINVAL;
    QRow *ri = static_cast<QRow *>(ws);
    QState *st = reinterpret_cast<QState *>(ri + rows);
    ull *ghist = reinterpret_cast<ull *>(st + rows * nq);
    hipError_t e = hipMemsetAsync(ws, 0, need, s);
    if (e != hipSuccess) return (int)e;
    const int64_t chunk = med::chunk_of(rows, red);
    const int64_t nch = (red + chunk - 1) / chunk;
    if (nch > 0x7fffffffLL) return NFM_ESIZE;
    const dim3 grid((unsigned)nch, (unsigned)rows);
    const size_t lds = (size_t)nq * kLongBins * sizeof(unsigned);
#define NFM_QNT_BY_NQ(CALL)       \
    do {                          \
        if (nq == 1) {            \
            constexpr int NQ = 1; \
            CALL;                 \
        } else if (nq == 2) {     \
            constexpr int NQ = 2; \
            CALL;                 \
        } else if (nq <= 4) {     \
            constexpr int NQ = 4; \
            CALL;                 \
        } else {                  \
            constexpr int NQ = kMaxQ; \
            CALL;                 \
        }                         \
    } while (0)
    for (int pass = 0; pass < LongDigits<T>::passes; ++pass) {
        if (pass == 0)
            hipLaunchKernelGGL((quantile_hist0_kernel<T>), grid, dim3(256), 0, s, xp, red, chunk, nq, ri, ghist);
        else
            NFM_QNT_BY_NQ(hipLaunchKernelGGL((quantile_hist_kernel<T, NQ>), grid, dim3(256), lds, s, xp, red, chunk, pass, nq,
                                             ri, st, ghist));
        hipLaunchKernelGGL((quantile_pick_kernel<T>), dim3((unsigned)rows), dim3(64), 0, s, red, pass, omitnan, interp, nq,
                           qa, ri, st, ghist);
    }
    const int want_pos = pos != nullptr;
    const unsigned nfin = (unsigned)((rows * nq + 255) / 256);
    if (need_hi || want_pos) { // skipped when no q needs v_hi and no position is wanted
        NFM_QNT_BY_NQ(hipLaunchKernelGGL((quantile_succ_kernel<T, NQ>), grid, dim3(256), 0, s, xp, red, chunk, nq, want_pos,
                                         0, ri, st));
        hipLaunchKernelGGL(quantile_resolve_kernel, dim3(nfin), dim3(256), 0, s, rows, red, omitnan, interp, nq, qa, ri, st);
        if (need_hi && want_pos)
            NFM_QNT_BY_NQ(hipLaunchKernelGGL((quantile_succ_kernel<T, NQ>), grid, dim3(256), 0, s, xp, red, chunk, nq, 1, 1,
                                             ri, st));
    }
    hipLaunchKernelGGL((quantile_final_kernel<T>), dim3(nfin), dim3(256), 0, s, rows, red, omitnan, interp, nq, qa,
                       (need_hi || want_pos) ? 1 : 0, (need_hi && want_pos) ? 1 : 0, ri, st, vp, pp);
#undef NFM_QNT_BY_NQ
    return launch_status();
}

static bool interp_ok(int interp) { return interp >= NFM_QUANTILE_LINEAR && interp <= NFM_QUANTILE_MIDPOINT; }
static bool q_ok(double q) { return q >= 0.0 && q <= 1.0; } // false for a NaN

} // namespace qnt
} // namespace nfm

using namespace nfm;

extern "C" {

int nfm_reduce_quantile_max_q(void) { return qnt::kMaxQ; }

size_t nfm_reduce_quantile_workspace_bytes(int64_t rows, int64_t red, int nq)
{
    if (rows <= 0 || nq < 1 || red <= med::kShortMax) return 0;
    return qnt::workspace_need(rows, nq);
}

int nfm_reduce_quantile_plan_host(double q, uint64_t count, int interp, uint64_t *lo, uint64_t *hi, double *w)
{
    if (!qnt::interp_ok(interp) || !qnt::q_ok(q) || count == 0) return NFM_EINVAL;
    if (lo == nullptr || hi == nullptr || w == nullptr) return NFM_EINVAL;
    const qnt::Plan pl = qnt::plan_of(q, count, interp);
    *lo = pl.lo;
    *hi = pl.hi;
    *w = pl.w;
    return NFM_OK;
}

int nfm_reduce_quantile(int dtype, int omitnan, int interp, int64_t rows, int64_t red, int nq, const double *q,
                        const void *x, void *workspace, size_t workspace_bytes, void *val, void *pos, void *stream)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (rows < 0 || red < 0 || nq < 1 || !qnt::interp_ok(interp)) return NFM_EINVAL;
    if (nq > qnt::kMaxQ) return NFM_ESIZE;
    if (q == nullptr) return NFM_EINVAL;
    qnt::QArgs qa;
    bool need_hi = false;
    for (int i = 0; i < qnt::kMaxQ; ++i) {
        qa.q[i] = i < nq ? q[i] : 0.0;
        if (!qnt::q_ok(qa.q[i])) return NFM_EINVAL;
        need_hi = need_hi || (qa.q[i] != 0.0 && qa.q[i] != 1.0); // q = 0 and q = 1 land on a rank at every count
    }
    need_hi = need_hi && (interp == NFM_QUANTILE_LINEAR || interp == NFM_QUANTILE_MIDPOINT);
    if (rows == 0) return NFM_OK;
    if (red == 0 || x == nullptr || val == nullptr) return NFM_EINVAL;
    return by_dtype(dtype, [&](auto t) {
        return qnt::run<decltype(t)>(omitnan ? 1 : 0, interp, rows, red, nq, qa, need_hi, x, workspace, workspace_bytes, val,
                                     pos, stream);
    });
}

} // extern "C"
