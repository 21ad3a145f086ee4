// nfm_reduce_select.hpp -- the radix selection building blocks that nfm_reduce_median.hip (one rank per row) and
// nfm_reduce_quantile.hip (several ranks per row) share, as forced-inline templates:
//   every length: the row counting rule (row_count), above();
//   longer rows:  the 11-bit digits of a pass over HBM (LongDigits), the walk of a chunk in 16-byte loads
//                 (stream_chunk), the 64-bit digit pick of one wavefront (pick_digit_n), the chunking of a row
//                 (chunk_of);
//   host:         the launch ladders of the two register forms (launch_tiny, launch_rows).
// The register forms themselves (red <= 32, red <= 1024) and the first-pass histogram are written out in both
// files: built from common blocks the quantile's kernels were scheduled differently and ran slower
// (profiles/select_refactor.md).
// Kept out of nfm_reduce_median.hpp so that the one-row-per-lane objects (nfm_reduce_median_lane.hip) do not
// depend on it.
#pragma once
#include "nfm_reduce_median.hpp"

namespace nfm {
namespace med {

using ull = unsigned long long;

// Keys and 64-bit counts cross lanes through the runtime's own __shfl / __shfl_xor / __shfl_up: their 64-bit
// overloads move the two halves (one value is still split by hand, in pick_digit_n).

// THE counting rule of every form: the elements of a row that count, and whether its result is NaN (a NaN that
// is not omitted, or nothing left).  C = unsigned for rows in registers, 64 bits for long rows.
template <typename C>
struct RowCount {
    C count;
    bool want_nan;
};
template <typename C>
__device__ __forceinline__ RowCount<C> row_count(C red, C nan, int omitnan)
{
    const C count = omitnan ? red - nan : red;
    return {count, (!omitnan && nan > 0) || count == 0};
}

// the part of a key above digit d (0 for the top digit: nothing chosen yet)
template <typename U>
__device__ __forceinline__ U above(U key, int d, int digits)
{
    return d + 1 < digits ? (U)(key >> (8 * (d + 1))) : U(0);
}

// ---------------------------------------------------------------------------------------------
// long rows: 11-bit digits.  Pass p (0 = most significant) covers key bits [shift, shift + width).
constexpr int kLongBits = 11, kLongBins = 1 << kLongBits;
template <typename T>
struct LongDigits {
    static constexpr int bits = 8 * (int)sizeof(T);
    static constexpr int passes = (bits + kLongBits - 1) / kLongBits;
    static __host__ __device__ constexpr int width(int p) { return p + 1 < passes ? kLongBits : bits - kLongBits * (passes - 1); }
    static __host__ __device__ constexpr int shift(int p) { return p + 1 < passes ? bits - kLongBits * (p + 1) : 0; }
};

// walk the chunk [lo, hi) of the row with a workgroup of 256: 16-byte loads over the aligned middle, elements
// at its ragged ends; f(value, position in the row)
template <typename T, typename F>
__device__ __forceinline__ void stream_chunk(const T *__restrict__ p, int64_t lo, int64_t hi, F &&f)
{
    using V = typename VecOf<T>::gtype;
    constexpr int NV = VecOf<T>::N;
    int64_t j = lo + threadIdx.x;
    const int64_t mis = (int64_t)((reinterpret_cast<uintptr_t>(p + lo) / sizeof(T)) % NV);
    const int64_t head = mis ? (NV - mis < hi - lo ? NV - mis : hi - lo) : 0;
    if (j < lo + head) f(NFM_LDG(p + j), j);
    const int64_t body0 = lo + head, nvec = (hi - body0) / NV;
    for (int64_t q = threadIdx.x; q < nvec; q += 256) {
        const V v = NFM_LDG(reinterpret_cast<const V *>(p + body0) + q);
#pragma unroll
        for (int c = 0; c < NV; ++c) f(v[c], body0 + q * NV + c);
    }
    j = body0 + nvec * NV + threadIdx.x;
    if (j < hi) f(NFM_LDG(p + j), j);
}

__device__ __forceinline__ ull wave_excl_scan64(ull v)
{
    const int lane = threadIdx.x & 63;
    ull s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const ull o = __shfl_up(s, off, 64);
        if (lane >= off) s += o;
    }
    return s - v;
}

// pick the digit whose cumulative count passes k: `cnt` = this lane's NB consecutive bins (64 * NB bins in the
// wavefront); returns the digit and reduces k to the rank inside that digit.  Counts in 64 bits: a single row
// can hold 2^33 elements -- the dim=None median of a 32 GiB tensor -- and constant data puts them all in one bin
template <int NB>
__device__ __forceinline__ unsigned pick_digit_n(const ull (&cnt)[NB], ull &k)
{
    const int lane = threadIdx.x & 63;
    ull mine = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) mine += cnt[b];
    const ull before = wave_excl_scan64(mine);
    const bool here = before <= k && k < before + mine;
    const ull m = __ballot(here);
    const int src = m ? __builtin_ctzll(m) : 63; // k < total always: exactly one lane
    unsigned digit = 0;
    ull kk = k;
    if (lane == src) {
        ull r = k - before;
        unsigned d = 0;
#pragma unroll
        for (int b = 0; b < NB - 1; ++b)
            if (d == (unsigned)b && r >= cnt[b]) {
                r -= cnt[b];
                d = b + 1;
            }
        digit = NB * lane + d;
        kk = r;
    }
    digit = __shfl(digit, src, 64);
    // (the halves by hand ONLY so that median_pick_kernel keeps the 77 registers it had and stays comparable with
    // the build before: through the 64-bit overload it allocates 76.  Replace by k = __shfl(kk, src, 64) at will.)
    const unsigned lo = __shfl((unsigned)kk, src, 64), hi = __shfl((unsigned)(kk >> 32), src, 64);
    k = ((ull)hi << 32) | lo;
    return digit;
}

constexpr int kShortMax = 1024; // longer rows are selected over HBM

inline int64_t chunk_of(int64_t rows, int64_t red)
{
    // ~2048 workgroups in flight, chunks of at least 16 Ki elements, a multiple of 1024
    int64_t per_row = (2048 + rows - 1) / rows;
    if (per_row < 1) per_row = 1;
    int64_t chunk = (red + per_row - 1) / per_row;
    if (chunk < 16384) chunk = 16384;
    return ((chunk + 1023) / 1024) * 1024;
}

// ---------------------------------------------------------------------------------------------
// the launch ladders of the register forms: workgroups of 4 wavefronts, 64 / G rows per wavefront.
// f(E, G, nblk) with E and G as std::integral_constant launches the kernel on nblk workgroups.
template <int E, int G, typename F>
inline int launch_group(int64_t rows, F &f)
{
    const int64_t nblk = (rows + 4 * (64 / G) - 1) / (4 * (64 / G));
    if (nblk > 0x7fffffffLL) return NFM_ESIZE;
    f(std::integral_constant<int, E>{}, std::integral_constant<int, G>{}, (unsigned)nblk);
    return launch_status();
}
template <typename F>
inline int launch_tiny(int64_t rows, int64_t red, F &&f) // red <= 32: one element per lane
{
    return red <= 8 ? launch_group<1, 8>(rows, f) : red <= 16 ? launch_group<1, 16>(rows, f) : launch_group<1, 32>(rows, f);
}
template <typename F>
inline int launch_rows(int64_t rows, int64_t red, F &&f) // red <= kShortMax: E keys per lane
{
    return red <= 64    ? launch_group<4, 16>(rows, f)
           : red <= 128 ? launch_group<8, 16>(rows, f)
           : red <= 256 ? launch_group<16, 16>(rows, f)
           : red <= 512 ? launch_group<16, 32>(rows, f)
                        : launch_group<16, 64>(rows, f);
}

} // namespace med
} // namespace nfm
