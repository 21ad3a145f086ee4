// nfm_polar.hip -- singular value and polar decompositions of small square matrices, one record per lane through
// rec_kernel (batchsvdvals, batchsvd, batchpolar and the gradient of batchpolar; an extension of `batched`, no
// counterpart in the reference).  The arithmetic is in nfm_polar_ops.hpp; this file holds the caps, the launchers
// and the entry points.
#include "nfm_record_kernel.hpp"
#include "nfm_polar_ops.hpp"

// This file is compiled 33 times (-DNFM_POLAR_PART=0..32).  Part 0: the entry points, the caps and the host loop.
// Parts 1..32: the kernels of one (dtype, op, pair of orders):
// part = 1 + dtype * 16 + op * 4 + pair, pair p = orders 2p + 1 and 2p + 2.
#ifndef NFM_POLAR_PART
#error "compile with -DNFM_POLAR_PART=0..32"
#endif

namespace nfm {

enum { POLAR_VALS = 0, POLAR_FULL = 1, POLAR_POLAR = 2, POLAR_BWD = 3 };

// The compiled caps: the largest order of each (dtype, op) whose kernels have no private segment in any layout kind
// (profiles/polar_table.md lists the registers of every instantiation).  Orders above take the caller's own route.
// (the backward kernel holds A, U, both cotangents and their products: float32 8 x 8 needs 100 bytes of scratch in its
// channel-first form, float64 from 6 x 6 on in every form; float64 8 x 8 polar holds A, U and the 2 N^2 results: 52 bytes
// in its channel-first form)
constexpr int kPolarCap[2][4] = {{8, 8, 8, 7}, {8, 8, 7, 5}}; // [dtype][op]
constexpr bool polar_fits(bool f64, int op, int N) { return N >= 1 && N <= kPolarCap[f64 ? 1 : 0][op]; }

// one launcher per part: (N, a, gr, gp, out)
#define NFM_POLAR_ARGS                                                                                                 \
    int N, const nfm_operand *a, const nfm_operand *gr, const nfm_operand *gp, const nfm_operand *o, int64_t no,        \
        int64_t ni, const polar::BwdParams &q, void *stream
template <int PART>
int polar_part(NFM_POLAR_ARGS);

#if NFM_POLAR_PART >= 1
template <>
int polar_part<NFM_POLAR_PART>(NFM_POLAR_ARGS)
{
    constexpr int part = NFM_POLAR_PART - 1;
    constexpr bool F64 = part / 16 != 0;
    constexpr int OP = (part / 4) % 4;
    constexpr int N0 = 2 * (part % 4) + 1;
    using T = std::conditional_t<F64, double, float>;
    auto run = [&](auto n) -> int {
        constexpr int M = decltype(n)::value;
        if constexpr (polar_fits(F64, OP, M)) {
            const polar::NoParams none{0};
            if constexpr (OP == POLAR_VALS)
                return rec_launch<T, SvdValsOp<T, M>>(a, nullptr, nullptr, o, no, ni, none, stream);
            else if constexpr (OP == POLAR_FULL)
                return rec_launch<T, SvdFullOp<T, M>>(a, nullptr, nullptr, o, no, ni, none, stream);
            else if constexpr (OP == POLAR_POLAR)
                return rec_launch<T, PolarOp<T, M>>(a, nullptr, nullptr, o, no, ni, none, stream);
            else
                return rec_launch<T, PolarBwdOp<T, M>>(a, gr, gp, o, no, ni, q, stream);
        } else {
            return NFM_ESIZE;
        }
    };
    if (N == N0) return run(std::integral_constant<int, N0>{});
    if (N == N0 + 1) return run(std::integral_constant<int, N0 + 1>{});
    return NFM_ESIZE;
}
#endif

} // namespace nfm

#if NFM_POLAR_PART == 0
using namespace nfm;

static int polar_check(int dtype, int N, int op, int64_t n_outer, int64_t n_inner)
{
    const int rc = check_batch(dtype, n_outer, n_inner, {N});
    if (rc) return rc;
    if (!polar_fits(dtype == NFM_F64, op, N)) return NFM_ESIZE;
    return NFM_OK;
}

static int polar_dispatch(int dtype, int N, int op, const nfm_operand *a, const nfm_operand *gr, const nfm_operand *gp,
                          const nfm_operand *o, int64_t no, int64_t ni, const polar::BwdParams &q, void *stream)
{
    const int part = (dtype == NFM_F64 ? 16 : 0) + op * 4 + (N - 1) / 2;
    return switch_order<32>(part + 1, NFM_ESIZE, [&](auto p) {
        constexpr int P = p;
        return polar_part<P>(N, a, gr, gp, o, no, ni, q, stream);
    });
}

static int polar_forward(int dtype, int N, int op, int64_t n_outer, int64_t n_inner, const nfm_operand *a,
                         const nfm_operand *out, void *stream)
{
    int rc = polar_check(dtype, N, op, n_outer, n_inner);
    if (rc) return rc;
    if ((rc = check_operands(dtype, n_outer, n_inner, {a, out}))) return rc;
    return polar_dispatch(dtype, N, op, a, nullptr, nullptr, out, n_outer, n_inner, polar::BwdParams{0, 0}, stream);
}

// the record routine on n contiguous row-major host records; the largest sweep count
template <typename T, int N>
static int polar_host_loop(int op, int64_t n, const T *a, const T *gr, const T *gp, T *out)
{
    constexpr int NN = N * N;
    const polar::BwdParams q{gr != nullptr, gp != nullptr};
    int most = 0;
    for (int64_t i = 0; i < n; ++i) {
        int s;
        if (op == POLAR_VALS) s = polar::vals_flat<T, N>(a + i * NN, out + i * N);
        else if (op == POLAR_FULL) s = polar::full_flat<T, N>(a + i * NN, out + i * (N + 2 * NN));
        else if (op == POLAR_POLAR) s = polar::polar_flat<T, N>(a + i * NN, out + i * 2 * NN);
        else
            s = polar::polar_bwd_flat<T, N>(a + i * NN, gr ? gr + i * NN : a, gp ? gp + i * NN : a, out + i * NN, q);
        most = s > most ? s : most;
    }
    return most;
}

extern "C" {

int nfm_batch_svdvals(int dtype, int N, int64_t n_outer, int64_t n_inner, const nfm_operand *a, const nfm_operand *out,
                      void *stream)
{
    return polar_forward(dtype, N, POLAR_VALS, n_outer, n_inner, a, out, stream);
}

int nfm_batch_svd(int dtype, int N, int64_t n_outer, int64_t n_inner, const nfm_operand *a, const nfm_operand *out,
                  void *stream)
{
    return polar_forward(dtype, N, POLAR_FULL, n_outer, n_inner, a, out, stream);
}

int nfm_batch_polar(int dtype, int N, int64_t n_outer, int64_t n_inner, const nfm_operand *a, const nfm_operand *out,
                    void *stream)
{
    return polar_forward(dtype, N, POLAR_POLAR, n_outer, n_inner, a, out, stream);
}

int nfm_batch_polar_backward(int dtype, int N, int64_t n_outer, int64_t n_inner, const nfm_operand *a,
                             const nfm_operand *gr, const nfm_operand *gp, const nfm_operand *ga, void *stream)
{
    int rc = polar_check(dtype, N, POLAR_BWD, n_outer, n_inner);
    if (rc) return rc;
    if (gr == nullptr && gp == nullptr) return NFM_EINVAL;
    if ((rc = check_operands(dtype, n_outer, n_inner, {a, {gr, gr != nullptr}, {gp, gp != nullptr}, ga}))) return rc;
    // an absent cotangent: the kernel is handed A a second time and told not to look at it
    const polar::BwdParams q{gr != nullptr, gp != nullptr};
    return polar_dispatch(dtype, N, POLAR_BWD, a, gr ? gr : a, gp ? gp : a, ga, n_outer, n_inner, q, stream);
}

int nfm_polar_max_order(int dtype, int op)
{
    if ((dtype != NFM_F32 && dtype != NFM_F64) || op < 0 || op > 3) return 0;
    return kPolarCap[dtype == NFM_F64 ? 1 : 0][op];
}

int nfm_polar_host(int dtype, int op, int N, int64_t n, const void *a, const void *gr, const void *gp, void *out)
{
    if (dtype != NFM_F32 && dtype != NFM_F64) return NFM_EDTYPE;
    if (n < 0 || op < 0 || op > 3) return NFM_EINVAL;
    if (N < 1 || N > NFM_SVD_MAX_DIM) return NFM_ESIZE;
    if (n > 0 && (a == nullptr || out == nullptr)) return NFM_EINVAL;
    if (op == POLAR_BWD && gr == nullptr && gp == nullptr) return NFM_EINVAL;
    return switch_order<NFM_SVD_MAX_DIM>(N, NFM_ESIZE, [&](auto m) {
        constexpr int M = m;
        return by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return polar_host_loop<T, M>(op, n, static_cast<const T *>(a), static_cast<const T *>(gr),
                                         static_cast<const T *>(gp), static_cast<T *>(out));
        });
    });
}

} // extern "C"
#endif
