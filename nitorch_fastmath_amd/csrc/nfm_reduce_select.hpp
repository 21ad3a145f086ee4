// nfm_reduce_select.hpp -- the long-row radix selection machinery shared by nfm_reduce_median.hip (one rank
// per row) and nfm_reduce_quantile.hip (several ranks per row): the 11-bit digits of a pass over HBM, the
// 64-bit digit pick of one wavefront and the chunking of a row over workgroups.  Kept out of
// nfm_reduce_median.hpp so that the one-row-per-lane objects (nfm_reduce_median_lane.hip) do not depend on it.
#pragma once
#include "nfm_reduce_median.hpp"

namespace nfm {
namespace med {

// long rows: 11-bit digits.  Pass p (0 = most significant) covers key bits [shift, shift + width).
constexpr int kLongBits = 11, kLongBins = 1 << kLongBits;
template <typename T>
struct LongDigits {
    static constexpr int bits = 8 * (int)sizeof(T);
    static constexpr int passes = (bits + kLongBits - 1) / kLongBits;
    static __host__ __device__ constexpr int width(int p) { return p + 1 < passes ? kLongBits : bits - kLongBits * (passes - 1); }
    static __host__ __device__ constexpr int shift(int p) { return p + 1 < passes ? bits - kLongBits * (p + 1) : 0; }
};

__device__ __forceinline__ unsigned long long wave_excl_scan64(unsigned long long v)
{
    const int lane = threadIdx.x & 63;
    unsigned long long s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned lo = __shfl_up((unsigned)s, off, 64), hi = __shfl_up((unsigned)(s >> 32), off, 64);
        if (lane >= off) s += ((unsigned long long)hi << 32) | lo;
    }
    return s - v;
}

// pick_digit for NB consecutive bins per lane (64 * NB bins) of a LONG row: counts in 64 bits (a single row
// can hold 2^33 elements -- the dim=None median of a 32 GiB tensor -- and constant data puts them all in one bin)
template <int NB>
__device__ __forceinline__ unsigned pick_digit_n(const unsigned long long (&cnt)[NB], unsigned long long &k)
{
    const int lane = threadIdx.x & 63;
    unsigned long long mine = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) mine += cnt[b];
    const unsigned long long before = wave_excl_scan64(mine);
    const bool here = before <= k && k < before + mine;
    const unsigned long long m = __ballot(here);
    const int src = m ? __builtin_ctzll(m) : 63; // k < total always: exactly one lane
    unsigned digit = 0;
    unsigned long long kk = k;
    if (lane == src) {
        unsigned long long r = k - before;
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
    const unsigned lo = __shfl((unsigned)kk, src, 64), hi = __shfl((unsigned)(kk >> 32), src, 64);
    k = ((unsigned long long)hi << 32) | lo;
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

} // namespace med
} // namespace nfm
