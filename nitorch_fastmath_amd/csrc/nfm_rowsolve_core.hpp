// nfm_rowsolve_core.hpp -- the device side of nfm_rowsolve.hip: A X = B for a general ('lu') or positive definite
// ('chol') matrix of order 9..16 and up to KB right-hand sides, one row of [A | B] per lane slot.  The machinery is
// that of roww_tile (nfm_rowwave_core.hpp, whose helpers are used as they are): 16 matrices per workgroup,
// G = 16 / R lanes per matrix, R rows of N + KB values per lane, fully unrolled.
#pragma once
#include "nfm_rowwave_core.hpp"

namespace nfm {
namespace rows {

using roww::MPB;

constexpr int kRowsolveMinDim = 9;
constexpr int kRowsolveMaxCols = 8; // the largest compiled width: the column cap of one launch

// the compiled widths: K columns run the next width, the columns past K are zeros made in registers
constexpr int rowsolve_width(int K) { return K <= 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : 8; }

// The form of the kernel of a (dtype, N): rows per lane, and whether the pivot row travels through the per-matrix
// LDS slot (true) or by ds_bpermute (false).  Measured on MI355X (profiles/rowsolve_forms.md: the six candidates per
// (dtype, N), both methods, K = 1 and 8, 2^18 contiguous records): the entry is the form with the smallest geometric
// mean of time / best time over those four cases; the runner-up is within 5 % everywhere, the forms not chosen are up
// to 3.2x slower (float64 16, 4 rows per lane).  A build with -DNFM_ROWSOLVE_FORM_R=r -DNFM_ROWSOLVE_FORM_LB=0|1
// compiles every case in that form (scripts/bench_rowsolve.py --build-forms / --forms times such builds).
struct RsChoice {
    int rows;
    bool lds;
};
constexpr RsChoice rowsolve_choice(bool f64, int N)
{
#if defined(NFM_ROWSOLVE_FORM_R) && defined(NFM_ROWSOLVE_FORM_LB)
    return {NFM_ROWSOLVE_FORM_R, NFM_ROWSOLVE_FORM_LB != 0};
#else
    if (f64) return N >= 16 ? RsChoice{1, false} : N >= 12 ? RsChoice{1, true} : RsChoice{2, false};
    return N >= 11 ? RsChoice{2, false} : RsChoice{4, false};
#endif
}

// row pitch of the LDS image of [A | B] (and of X on the way out): a whole, odd number of 16-byte slots
template <typename T, int N, int KB>
constexpr int pitch() { return roww::RowStride<T, N + KB>::value; }
// the pivot-row slot of a matrix: N + KB values in whole 16-byte slots
template <typename T, int N, int KB>
constexpr int slot_elems()
{
    constexpr int V = 16 / (int)sizeof(T);
    return ((N + KB + V - 1) / V) * V;
}
template <typename T, int N, int KB, bool LB>
constexpr int lds_elems() { return MPB * N * pitch<T, N, KB>() + (LB ? MPB * slot_elems<T, N, KB>() : 0); }

// One tile: the records tile0 .. tile0 + 15 of outer index blockIdx.y.
//   STR false: a (ni, N, N), b (ni, N, K) and out (ni, N, K) dense and batch-major; 16-byte accesses (element
//              accesses when a base is not 16-byte aligned).
//   STR true : every element at its operand's strides, the record index fastest across the lanes.
// Both fill the same LDS image and run the same arithmetic, so they give the same bits.  has_b == 0: the right-hand
// side is columns col0 .. col0 + K - 1 of the identity.  out may be b: a tile has read its records of b before it
// writes them.
template <typename T, int N, int KB, bool CHOL, int R, bool LB, bool STR>
__global__ __launch_bounds__(256 / R) void rowsolve_kernel(Opnd oa, Opnd ob, Opnd oo, int64_t ni, int K, int col0,
                                                           int has_b)
{
    using namespace roww;
    constexpr int G = 16 / R;    // lanes per matrix
    constexpr int NT = MPB * G;  // lanes per workgroup
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int P = pitch<T, N, KB>();
    using Vec = T __attribute__((ext_vector_type(V)));
    __shared__ __attribute__((aligned(16))) T img[lds_elems<T, N, KB, LB>()];

    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int g = tid / G, lr = tid % G;
    T *slot = img + MPB * N * P + (LB ? g * slot_elems<T, N, KB>() : 0);
    const int gbase = lane & ~(G - 1);
    const unsigned gmask = (1u << G) - 1u;
    const int64_t m0 = (int64_t)blockIdx.x * MPB;
    const int64_t o = blockIdx.y;
    const int nm = (int)((ni - m0) < MPB ? (ni - m0) : MPB);
    const T *A = reinterpret_cast<const T *>(oa.ptr), *B = reinterpret_cast<const T *>(ob.ptr);
    T *O = reinterpret_cast<T *>(oo.ptr);

    // ---- [A | B] of the tile into the LDS image: row i of matrix m at (m * N + i) * P, b from column N on
    if constexpr (STR) {
        for (int e = tid; e < MPB * N * N; e += NT) {
            const int m = e % MPB, c = e / MPB, i = c / N, j = c - i * N;
            if (m < nm) img[(m * N + i) * P + j] = A[o * oa.so + (m0 + m) * oa.si + i * oa.sr + j * oa.sc];
        }
        if (has_b) {
            for (int e = tid; e < MPB * N * KB; e += NT) {
                const int m = e % MPB, c = e / MPB, i = c / KB, j = c - i * KB;
                if (m < nm && j < K) img[(m * N + i) * P + N + j] = B[o * ob.so + (m0 + m) * ob.si + i * ob.sr + j * ob.sc];
            }
        }
    } else {
        auto stage = [&](const T *src, const int cols, const int at) {
            const int rec = N * cols, total = nm * rec;
            const bool vec_ok = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
            for (int e = tid * V; e < total; e += NT * V) {
                if (vec_ok && e + V <= total) {
                    const Vec v = NFM_LDG(reinterpret_cast<const Vec *>(src + e));
#pragma unroll
                    for (int q = 0; q < V; ++q) {
                        const int ee = e + q, m = ee / rec, rem = ee - m * rec, i = rem / cols, j = rem - i * cols;
                        img[(m * N + i) * P + at + j] = v[q];
                    }
                } else {
                    for (int ee = e; ee < total && ee < e + V; ++ee) {
                        const int m = ee / rec, rem = ee - m * rec, i = rem / cols, j = rem - i * cols;
                        img[(m * N + i) * P + at + j] = NFM_LDG(src + ee);
                    }
                }
            }
        };
        stage(A + m0 * (N * N), N, 0);
        if (has_b) stage(B + m0 * (N * K), K, N);
    }
    __syncthreads();

    // ---- my rows: row id of slot t is lr + t * G
    T row[R][N];
    T rhs[R][KB];
    bool used[R];
    int ppos[R]; // the step at which the row pivoted = the row of X it ends up holding
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const int rid = lr + t * G;
        const bool live = rid < N && g < nm;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if constexpr (CHOL) { // the lower triangle only: a[i][j] for j <= i, a[j][i] above the diagonal
                const int hi = rid > j ? rid : j, lo = rid > j ? j : rid;
                row[t][j] = live ? img[(g * N + hi) * P + lo] : T(0);
            } else {
                row[t][j] = live ? img[(g * N + rid) * P + j] : T(0);
            }
            if (!(g < nm)) row[t][j] = (rid == j) ? T(1) : T(0); // idle matrices of a ragged last tile: the identity
        }
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            if (has_b) rhs[t][j] = (live && j < K) ? img[(g * N + rid) * P + N + j] : T(0);
            else rhs[t][j] = (live && j < K && rid == col0 + j) ? T(1) : T(0);
        }
        used[t] = !(rid < N); // rows beyond the order never pivot
        ppos[t] = CHOL ? (rid < N ? rid : -1) : -1;
    }
    bool bad = false; // chol: a pivot that is not positive (NaN included)

#pragma unroll
    for (int k = 0; k < N; ++k) {
        int ts = 0, pl = 0;
        if constexpr (CHOL) { // step k pivots on row k
            ts = k / G;
            pl = k % G;
        } else { // the first unused row with the largest key; slot first, then lane (as roww_tile)
            unsigned key = 0;
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const unsigned kt = used[t] ? 0u : pivot_key(row[t][k]);
                ts = kt > key ? t : ts;
                key = kt > key ? kt : key;
            }
            const unsigned mx = groupmax<G>(key);
            const unsigned grp = (unsigned)(__ballot(key == mx) >> gbase) & gmask; // never 0: some row is unused
            pl = __builtin_ctz(grp | (1u << G));
        }
        const bool isl = lr == pl; // my lane holds the pivot row, in slot ts
        const int psrc = gbase + pl;
        // the pivot row of my lane's candidate slot (only the pivot lane's values are consumed)
        T cand[N], crhs[KB];
#pragma unroll
        for (int j = 0; j < N; ++j) cand[j] = row[0][j];
#pragma unroll
        for (int j = 0; j < KB; ++j) crhs[j] = rhs[0][j];
#pragma unroll
        for (int t = 1; t < R; ++t) {
#pragma unroll
            for (int j = 0; j < N; ++j) cand[j] = (ts == t) ? row[t][j] : cand[j];
#pragma unroll
            for (int j = 0; j < KB; ++j) crhs[j] = (ts == t) ? rhs[t][j] : crhs[j];
        }
        if constexpr (LB) {
            if (isl) {
#pragma unroll
                for (int j = k; j < N; ++j) slot[j] = cand[j];
#pragma unroll
                for (int j = 0; j < KB; ++j) slot[N + j] = crhs[j];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        auto pivot_row = [&](const T &mine, int j) -> T {
            if constexpr (LB) return slot[j];
            else return bcast(mine, psrc);
        };
        const T pv = pivot_row(cand[k], k);
        if constexpr (CHOL) bad = bad || !(pv > T(0));
        const T rp = pivot_recip(pv);
        // multipliers of my rows; 0 in the pivot row itself, so that the same fma leaves it unchanged
        T f[R];
#pragma unroll
        for (int t = 0; t < R; ++t) {
            f[t] = row[t][k] * rp;
            f[t] = (isl && ts == t) ? T(0) : f[t];
        }
        // Gauss-Jordan on [A | B]: columns k + 1 .. of A, every column of B
#pragma unroll
        for (int j = k + 1; j < N; ++j) {
            const T pj = pivot_row(cand[j], j);
#pragma unroll
            for (int t = 0; t < R; ++t) row[t][j] = roww::fma_(-f[t], pj, row[t][j]);
        }
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            const T pb = pivot_row(crhs[j], N + j);
#pragma unroll
            for (int t = 0; t < R; ++t) rhs[t][j] = roww::fma_(-f[t], pb, rhs[t][j]);
        }
        if constexpr (!CHOL) {
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const bool me = isl && ts == t;
                used[t] = used[t] || me;
                ppos[t] = me ? k : ppos[t];
            }
        }
        if constexpr (LB) { // the slot is rewritten by the next step only after every lane has read it
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }

    // ---- X: slot t holds row ppos[t], its right-hand sides over its pivot; into the image, then out
    __syncthreads(); // every lane has taken its rows out of the image
#pragma unroll
    for (int t = 0; t < R; ++t) {
        T piv = T(1); // the pivot is still at column ppos of the row
#pragma unroll
        for (int j = 0; j < N; ++j) piv = (ppos[t] == j) ? row[t][j] : piv;
        if (g < nm && ppos[t] >= 0) {
#pragma unroll
            for (int j = 0; j < KB; ++j) {
                T x = rhs[t][j] / piv;
                if constexpr (CHOL) x = bad ? __builtin_nan("") : x;
                if (j < K) img[(g * N + ppos[t]) * P + j] = x;
            }
        }
    }
    __syncthreads();
    if constexpr (STR) {
        for (int e = tid; e < MPB * N * KB; e += NT) {
            const int m = e % MPB, c = e / MPB, i = c / KB, j = c - i * KB;
            if (m < nm && j < K) O[o * oo.so + (m0 + m) * oo.si + i * oo.sr + j * oo.sc] = img[(m * N + i) * P + j];
        }
    } else {
        const int rec = N * K, total = nm * rec;
        T *dst = O + m0 * rec;
        const bool vec_ok = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
        for (int e = tid * V; e < total; e += NT * V) {
            T tmp[V];
#pragma unroll
            for (int q = 0; q < V; ++q) {
                const int ee = e + q, m = ee / rec, rem = ee - m * rec, i = rem / K, j = rem - i * K;
                tmp[q] = (ee < total) ? img[(m * N + i) * P + j] : T(0);
            }
            if (vec_ok && e + V <= total) {
                Vec v;
#pragma unroll
                for (int q = 0; q < V; ++q) v[q] = tmp[q];
                NFM_STG(v, reinterpret_cast<Vec *>(dst + e));
            } else {
#pragma unroll
                for (int q = 0; q < V; ++q)
                    if (e + q < total) NFM_STG(tmp[q], dst + e + q);
            }
        }
    }
}

} // namespace rows
} // namespace nfm
