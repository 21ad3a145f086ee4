// nfm_lstsq.hip -- X = A^+ B for one tall M x N matrix per lane (N <= 8, M up to NFM_LSTSQ_MAX_ROWS) and K
// right-hand sides: the rows of [A | B] stream past the lane's N x N triangle (Givens rotations) and the Jacobi
// routine finishes on it (nfm_lstsq_ops.hpp; reference `sugar.py`: lmdiv / solvevec / rmdiv of a non-square
// system with more rows than the 8 of nfm_svd.hip).  Without NFM_LSTSQ_PART: the entry points nfm_lstsq_solve,
// nfm_lstsq_solve_host and nfm_lstsq_max_cols.  With -DNFM_LSTSQ_PART=0..15: one object per (dtype, N), every
// K = 1..lstsq_max_k, so that the fully unrolled rotations and sweeps build in parallel: PART = dtype * 8 + N - 1.
//
// Two kernels, three movement modes (chosen on the host from the strides, the same for every lane):
//   1. lstsq_tile_kernel: A and B batch-major contiguous.  A block of kLstsqRB rows of one record is
//      kLstsqRB * N back-to-back elements: the workgroup fetches its TILE records' segments with 16-byte loads,
//      consecutive lanes on consecutive addresses of a segment, parks them in an LDS image whose record pitch is
//      an odd number of 16-byte slots (TileIO's rule: the lanes' own ds_read_b128 are conflict-free), and every
//      lane picks up its rows.  The loads of block i + 1 are issued into registers before block i is rotated in.
//   2. lstsq_lane_kernel with inner batch stride 1 (channel-first): lane t reads element (row, col) of record
//      tile0 + t, consecutive lanes on consecutive addresses -- coalesced as it stands, no LDS.
//   3. lstsq_lane_kernel with any other strides (a.mT, broadcast, padded records): the same per-lane loads.
// X is N K values per record and goes out with direct stores at the strides of `out`.
#include "nfm_lstsq_ops.hpp"
#include "nfm_solve_entry.hpp"

namespace nfm {

#define NFM_LSTSQ_ARGS                                                                                             \
    int M, int K, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *b, const nfm_operand *out,      \
        double rcond, int host, void *stream
template <int PART>
int lstsq_part(NFM_LSTSQ_ARGS);

#ifdef NFM_LSTSQ_PART

#if NFM_LSTSQ_PART < 8
using TS = float;
#else
using TS = double;
#endif
constexpr int kN = NFM_LSTSQ_PART % 8 + 1;

// bytes of one record's row block in the LDS image: whole 16-byte slots, an odd number of them
constexpr int lstsq_pitch(int elems, int elem_bytes)
{
    const int slots = elems * elem_bytes / 16;
    return (slots % 2 == 0 ? slots + 1 : slots) * 16;
}

template <typename T, int N, int K>
struct LstsqGeom {
    static constexpr int CA = kLstsqRB * N, CB = kLstsqRB * K;
    static_assert((CA * sizeof(T)) % 16 == 0 && (CB * sizeof(T)) % 16 == 0, "row blocks are whole 16-byte vectors");
    // one image of A's and B's row blocks for the tile, at most 36 KiB (pick_tile): 4+ workgroups per CU, more
    // than the registers of these kernels allow
    static constexpr int TILE = pick_tile(lstsq_pitch(CA, sizeof(T)) + lstsq_pitch(CB, sizeof(T)));
    using IA = TileIO<T, CA, TILE>;
    using IB = TileIO<T, CB, TILE>;
    static_assert(IA::kWide && IB::kWide && IA::kNVec % TILE == 0 && IB::kNVec % TILE == 0, "whole slots per lane");
    static constexpr int kLds = IA::kLdsBytes + IB::kLdsBytes;
};
constexpr int kLstsqLaneTile = 128;

// The loads of one row block of the tile: vector q of the image is vector `col` of the segment of record
// tile0 + q / kSlots, at g + rec * rec_stride + off.  `cnt` = elements of the segment inside the record (rows *
// columns: the last block may be short); a vector that crosses it is fetched element by element, what lies past
// it and the records past the end of the batch are zeros.  Nothing outside a record is read.
template <class IO, typename T>
__device__ __forceinline__ void lstsq_issue(const T *__restrict__ g, int64_t tile0, int64_t n_inner,
                                            int64_t rec_stride, int64_t off, int cnt, typename IO::Stage &st)
{
    using V = typename IO::V;
    using VG = typename IO::VG;
    const int tid = threadIdx.x;
#pragma unroll
    for (int it = 0; it < IO::kIters; ++it) {
        const int q = tid + it * (IO::kNVec / IO::kIters);
        const int row = q / IO::kSlots, col = q - row * IO::kSlots;
        const int e0 = col * IO::kVec;
        const int64_t rec = tile0 + row;
        V v;
#pragma unroll
        for (int k = 0; k < IO::kVec; ++k) v[k] = T(0);
        if (rec < n_inner) {
            const T *p = g + rec * rec_stride + off + e0;
            if (e0 + IO::kVec <= cnt) {
                v = NFM_LDG(reinterpret_cast<const VG *>(p));
            } else {
#pragma unroll
                for (int k = 0; k < IO::kVec; ++k)
                    if (e0 + k < cnt) v[k] = p[k];
            }
        }
        st.v[it] = v;
    }
}

template <typename T, int N, int K>
__device__ __forceinline__ void lstsq_store(const Opnd &out, int64_t o, int64_t i, const T (&x)[N][K])
{
    T *p = reinterpret_cast<T *>(out.ptr) + o * out.so + i * out.si;
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) p[j * out.sr + k * out.sc] = x[j][k];
}

// mode 1: A (n, M, N) and B (n, M, K) contiguous, one batch level
template <typename T, int N, int K>
__global__ __launch_bounds__((LstsqGeom<T, N, K>::TILE)) void lstsq_tile_kernel(const T *__restrict__ a,
                                                                               const T *__restrict__ b, Opnd out,
                                                                               int M, int64_t n_inner, T rc2)
{
    using G = LstsqGeom<T, N, K>;
    using IA = typename G::IA;
    using IB = typename G::IB;
    constexpr int RB = kLstsqRB;
    __shared__ __align__(16) unsigned char smem[G::kLds];
    unsigned char *lds_a = smem, *lds_b = smem + IA::kLdsBytes;
    const int64_t tile0 = (int64_t)blockIdx.x * G::TILE;
    const int64_t i = tile0 + threadIdx.x;

    LstsqState<T, N, K> st;
    lstsq_init(st);
    typename IA::Stage sa;
    typename IB::Stage sb;
    {
        const int rows = M < RB ? M : RB;
        lstsq_issue<IA, T>(a, tile0, n_inner, (int64_t)M * N, 0, rows * N, sa);
        lstsq_issue<IB, T>(b, tile0, n_inner, (int64_t)M * K, 0, rows * K, sb);
    }
    for (int m0 = 0; m0 < M; m0 += RB) { // M is a kernel argument: every lane of the grid makes the same trips
        const int rows = M - m0 < RB ? M - m0 : RB;
        IA::commit(lds_a, sa);
        IB::commit(lds_b, sb);
        __syncthreads();
        const int m1 = m0 + RB;
        if (m1 < M) { // the next block is in flight while this one is rotated in
            const int r1 = M - m1 < RB ? M - m1 : RB;
            lstsq_issue<IA, T>(a, tile0, n_inner, (int64_t)M * N, (int64_t)m1 * N, r1 * N, sa);
            lstsq_issue<IB, T>(b, tile0, n_inner, (int64_t)M * K, (int64_t)m1 * K, r1 * K, sb);
        }
        T fa[G::CA], fb[G::CB];
        IA::read_own(lds_a, fa);
        IB::read_own(lds_b, fb);
        __syncthreads(); // every lane has its rows: the image is free for the next block
        T ra[RB][N], rb[RB][K];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
#pragma unroll
            for (int c = 0; c < N; ++c) ra[r][c] = fa[r * N + c];
#pragma unroll
            for (int c = 0; c < K; ++c) rb[r][c] = fb[r * K + c];
        }
        lstsq_block<T, N, K>(st, ra, rb, rows);
    }
    T x[N][K];
    lstsq_finish<T, N, K>(st, x, rc2);
    if (i < n_inner) lstsq_store<T, N, K>(out, 0, i, x);
}

// rows m0 .. m0 + rows - 1 of one record at run-time strides (zeros for the rest of the block)
template <typename T, int N, int K, typename SA, typename SB>
__host__ __device__ __forceinline__ void lstsq_fetch(const T *pa, const SA &sa, const T *pb, const SB &sb, int m0,
                                                     int rows, T (&ra)[kLstsqRB][N], T (&rb)[kLstsqRB][K])
{
#pragma unroll
    for (int r = 0; r < kLstsqRB; ++r) {
        const bool in = r < rows;
        const int64_t m = m0 + (in ? r : 0);
#pragma unroll
        for (int c = 0; c < N; ++c) ra[r][c] = in ? pa[m * sa.sr + c * sa.sc] : T(0);
#pragma unroll
        for (int c = 0; c < K; ++c) rb[r][c] = in ? pb[m * sb.sr + c * sb.sc] : T(0);
    }
}

// modes 2 and 3: every lane fetches its own rows at the operand's strides
template <typename T, int N, int K>
__global__ __launch_bounds__(kLstsqLaneTile) void lstsq_lane_kernel(Opnd a, Opnd b, Opnd out, int M,
                                                                    int64_t n_inner, T rc2)
{
    constexpr int RB = kLstsqRB;
    const int64_t i = (int64_t)blockIdx.x * kLstsqLaneTile + threadIdx.x;
    const int64_t o = blockIdx.y;
    const bool valid = i < n_inner;
    const int64_t ii = valid ? i : 0; // lanes past the end of the batch read record 0 and store nothing
    const T *pa = reinterpret_cast<const T *>(a.ptr) + o * a.so + ii * a.si;
    const T *pb = reinterpret_cast<const T *>(b.ptr) + o * b.so + ii * b.si;

    LstsqState<T, N, K> st;
    lstsq_init(st);
    T na[RB][N], nb[RB][K];
    lstsq_fetch<T, N, K>(pa, a, pb, b, 0, M < RB ? M : RB, na, nb);
    for (int m0 = 0; m0 < M; m0 += RB) {
        const int rows = M - m0 < RB ? M - m0 : RB;
        T ra[RB][N], rb[RB][K];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
#pragma unroll
            for (int c = 0; c < N; ++c) ra[r][c] = na[r][c];
#pragma unroll
            for (int c = 0; c < K; ++c) rb[r][c] = nb[r][c];
        }
        const int m1 = m0 + RB;
        if (m1 < M) lstsq_fetch<T, N, K>(pa, a, pb, b, m1, M - m1 < RB ? M - m1 : RB, na, nb);
        lstsq_block<T, N, K>(st, ra, rb, rows);
    }
    T x[N][K];
    lstsq_finish<T, N, K>(st, x, rc2);
    if (valid) lstsq_store<T, N, K>(out, o, i, x);
}

struct HostStrides {
    int64_t sr, sc;
};

template <typename T, int N, int K>
static int lstsq_host_loop(int M, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *b,
                           const nfm_operand *out, double rcond)
{
    int most = 0;
    const HostStrides sa{a->stride_row, a->stride_col}, sb{b->stride_row, b->stride_col};
    for (int64_t o = 0; o < no; ++o)
        for (int64_t i = 0; i < ni; ++i) {
            const T *pa = static_cast<const T *>(a->ptr) + o * a->stride_outer + i * a->stride_inner;
            const T *pb = static_cast<const T *>(b->ptr) + o * b->stride_outer + i * b->stride_inner;
            LstsqState<T, N, K> st;
            lstsq_init(st);
            for (int m0 = 0; m0 < M; m0 += kLstsqRB) {
                const int rows = M - m0 < kLstsqRB ? M - m0 : kLstsqRB;
                T ra[kLstsqRB][N], rb[kLstsqRB][K];
                lstsq_fetch<T, N, K>(pa, sa, pb, sb, m0, rows, ra, rb);
                lstsq_block<T, N, K>(st, ra, rb, rows);
            }
            T x[N][K];
            const int sweeps = lstsq_finish<T, N, K>(st, x, T(rcond * rcond));
            most = sweeps > most ? sweeps : most;
            host_scatter<T>(out, o, i, N, K, &x[0][0]);
        }
    return most;
}

// records of rows x cols elements back to back, row-major (the stride of an extent of one is not looked at)
static bool lstsq_contig(const nfm_operand *op, int rows, int cols, int64_t ni)
{
    if (ni > 1 && op->stride_inner != (int64_t)rows * cols) return false;
    if (rows > 1 && op->stride_row != cols) return false;
    return cols == 1 || op->stride_col == 1;
}

template <typename T, int N, int K>
static int lstsq_launch(int M, int64_t no, int64_t ni, const nfm_operand *a, const nfm_operand *b,
                        const nfm_operand *out, double rcond, void *stream)
{
    using G = LstsqGeom<T, N, K>;
    const T rc2 = T(rcond * rcond);
    const bool tiles = no == 1 && lstsq_contig(a, M, N, ni) && lstsq_contig(b, M, K, ni);
    const int tile = tiles ? G::TILE : kLstsqLaneTile;
    const int64_t nblk = (ni + tile - 1) / tile;
    if (nblk > 0x7fffffffLL) return NFM_ESIZE;
    const Opnd oo = make_opnd(out, MODE_STRIDED);
    if (tiles)
        hipLaunchKernelGGL((lstsq_tile_kernel<T, N, K>), dim3((unsigned)nblk, 1, 1), dim3(tile, 1, 1), 0,
                           static_cast<hipStream_t>(stream), static_cast<const T *>(a->ptr),
                           static_cast<const T *>(b->ptr), oo, M, ni, rc2);
    else
        hipLaunchKernelGGL((lstsq_lane_kernel<T, N, K>), dim3((unsigned)nblk, (unsigned)no, 1), dim3(tile, 1, 1), 0,
                           static_cast<hipStream_t>(stream), make_opnd(a, MODE_STRIDED), make_opnd(b, MODE_STRIDED),
                           oo, M, ni, rc2);
    return launch_status();
}

template <>
int lstsq_part<NFM_LSTSQ_PART>(NFM_LSTSQ_ARGS)
{
    return switch_order<kLstsqMaxN>(K, NFM_ESIZE, [&](auto k) {
        constexpr int Kc = k;
        if constexpr (Kc > lstsq_max_k(sizeof(TS) == 8, kN)) return (int)NFM_ESIZE;
        else {
            if (host) return lstsq_host_loop<TS, kN, Kc>(M, no, ni, a, b, out, rcond);
            return lstsq_launch<TS, kN, Kc>(M, no, ni, a, b, out, rcond, stream);
        }
    });
}

#endif // NFM_LSTSQ_PART

} // namespace nfm

#ifndef NFM_LSTSQ_PART

using namespace nfm;

static int lstsq_entry(int dtype, int M, int N, int K, double rcond, int64_t n_outer, int64_t n_inner,
                       const nfm_operand &oa, const nfm_operand &ob, const nfm_operand &oo, int host, void *stream)
{
    const int rc = check_batch(dtype, n_outer, n_inner, {N, K}, kLstsqMaxN);
    if (rc) return rc;
    if (M < N || M > kLstsqMaxRows) return NFM_ESIZE;
    if (!(rcond >= 0.0)) return NFM_EINVAL;
    const SolveRhs rhs = check_rhs(dtype, n_outer, n_inner, K, lstsq_max_k(dtype == NFM_F64, N), 0, oa, ob, oo);
    if (!rhs.launch) return rhs.rc;
    const int part = (dtype == NFM_F64 ? 8 : 0) + N - 1;
    return switch_order<16>(part + 1, NFM_ESIZE, [&](auto p) {
        constexpr int P = p;
        return lstsq_part<P - 1>(M, K, n_outer, n_inner, &oa, rhs.b, &oo, rcond, host, stream);
    });
}

extern "C" {

int nfm_lstsq_max_cols(int dtype, int N)
{
    return max_cols_answer(dtype, {N}, kLstsqMaxN, lstsq_max_k(dtype == NFM_F64, N));
}

int nfm_lstsq_solve(int dtype, int M, int N, int K, double rcond, int64_t n_outer, int64_t n_inner,
                    const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                    const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                    void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc, void *stream)
{
    return lstsq_entry(dtype, M, N, K, rcond, n_outer, n_inner, flat_operand(a, a_so, a_si, a_sr, a_sc),
                       flat_operand(b, b_so, b_si, b_sr, b_sc), flat_operand(out, o_so, o_si, o_sr, o_sc), 0, stream);
}

int nfm_lstsq_solve_host(int dtype, int M, int N, int K, double rcond, int64_t n_outer, int64_t n_inner,
                         const void *a, int64_t a_so, int64_t a_si, int64_t a_sr, int64_t a_sc,
                         const void *b, int64_t b_so, int64_t b_si, int64_t b_sr, int64_t b_sc,
                         void *out, int64_t o_so, int64_t o_si, int64_t o_sr, int64_t o_sc)
{
    return lstsq_entry(dtype, M, N, K, rcond, n_outer, n_inner, flat_operand(a, a_so, a_si, a_sr, a_sc),
                       flat_operand(b, b_so, b_si, b_sr, b_sc), flat_operand(out, o_so, o_si, o_sr, o_sc), 1, nullptr);
}

} // extern "C"

#endif
