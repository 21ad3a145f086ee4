// nfm_rt_mm.hpp -- what nfm_rt.hip (entry points, argument check) and nfm_rt_mm.hip (the matrix-instruction
// kernel for long axes) share.
#pragma once
#include "nfm_rt_ops.hpp"

namespace nfm {
namespace rt {

struct Args {
    Plan p;
    int64_t outer, inner;
    const void *x;
    void *o;
};

constexpr size_t kLdsPlain = 64 * 1024, kLdsOptIn = 160 * 1024;

constexpr int table_len(int P) { return (P + 3) & ~3; } // keeps what follows 16-byte aligned

// the checked, non-empty call on the MFMA tile kernel (nfm_rt_mm.hip): any N in 1..NFM_RT_MAX_N
int dispatch_mm(int dtype, const Args &a, void *stream);

} // namespace rt
} // namespace nfm
