// nfm_stochastic_ops.hpp -- device pieces of the stochastic estimators (reference `stochastic.py`):
// the Philox4x32-10 counter-based generator and the two probe kinds built on it.
//
// A probe element is a function of (seed, element index e) alone:
//   Rademacher: counter (e / 128, 0, 0), bit (e % 128) % 32 of word (e % 128) / 32 -> +1 (set) / -1;
//   Gaussian:   counter (e / 4, 0, 1), words (w0, w1) and (w2, w3) are two Box-Muller pairs,
//               u = (2 (w >> 9) + 1) 2^-24 (exact in float32, never 0 or 1), r = sqrt(-2 ln u_a),
//               elements 0..3 of the counter are r0 cos, r0 sin, r1 cos, r1 sin of 2 pi u_b.
// Both dtypes use the same 23-bit uniforms: a float32 probe is the rounded float64 probe to a few ulps.
#pragma once
#include "nfm_common.hpp"

namespace nfm {
namespace stoch {

struct U4 {
    uint32_t w0, w1, w2, w3;
};

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__host__ __device__ inline U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1)
{
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c.w0, p1 = (uint64_t)M1 * c.w2;
        c = U4{(uint32_t)(p1 >> 32) ^ c.w1 ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w3 ^ k1, (uint32_t)p0};
        k0 += W0;
        k1 += W1;
    }
    return c;
}

// the 128 Rademacher bits of group g (elements 128 g .. 128 g + 127)
__device__ __forceinline__ U4 rademacher_group(uint64_t g, uint32_t k0, uint32_t k1)
{
    return philox4x32_10(U4{(uint32_t)g, (uint32_t)(g >> 32), 0u, 0u}, k0, k1);
}

template <typename T>
__device__ __forceinline__ T sign_of_bit(uint32_t bit)
{
    return bit ? T(1) : T(-1);
}

__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float &c, float &s)
{
    const float ua = (float)(2u * (wa >> 9) + 1u) * 0x1p-24f, ub = (float)(2u * (wb >> 9) + 1u) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(ua));
    float sn, cs;
    sincospif(2.0f * ub, &sn, &cs);
    c = r * cs;
    s = r * sn;
}
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, double &c, double &s)
{
    const double ua = (double)(2u * (wa >> 9) + 1u) * 0x1p-24, ub = (double)(2u * (wb >> 9) + 1u) * 0x1p-24;
    const double r = sqrt(-2.0 * log(ua));
    double sn, cs;
    sincospi(2.0 * ub, &sn, &cs);
    c = r * cs;
    s = r * sn;
}

// the 4 Gaussian elements of quad g (elements 4 g .. 4 g + 3)
template <typename T>
__device__ __forceinline__ void gaussian_quad(uint64_t g, uint32_t k0, uint32_t k1, T &e0, T &e1, T &e2, T &e3)
{
    const U4 w = philox4x32_10(U4{(uint32_t)g, (uint32_t)(g >> 32), 0u, 1u}, k0, k1);
    box_muller(w.w0, w.w1, e0, e1);
    box_muller(w.w2, w.w3, e2, e3);
}

} // namespace stoch
} // namespace nfm
