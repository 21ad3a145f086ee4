// nfm_spectral.hpp -- the per-lane blocks that sym_funm (nfm_symfun.hip) and the pencil kernels (nfm_sympencil.hip,
// nfm_sympencil_ops.hpp) share: the sweeps' arguments, the expansion of a compact record with the bad-record rule
// and the recomposition U diag(f) U^T.  Still in two places, because the kernels built from a
// shared block lost a wave per SIMD or gained a private segment (profiles/spectral_refactor.md): SymFunOp writes the
// recomposition out, and the three steps of the Daleckii-Krein gradient X [(Z^T G Z) o F] X^T are written out in
// SymFunBwdOp and in PencilFunBwdOp (its congruence a third time, without the halving, in sympencil::whiten).  A
// change to the compact convention or to the accumulation order goes to those places too; each names its twin.
#pragma once
#include "nfm_qr_core.hpp"
#include "nfm_symfun_ops.hpp"

namespace nfm {
namespace spectral {

// the sweeps' arguments: those of eig_sym's defaults (the fast sweeps floor tol at the working precision)
constexpr int kMaxIter = 1024;
constexpr double kTol = 1e-32;

// compact record -> the (mirrored) matrix eig_sym1 reads; true for a record with an entry that is not finite, which
// is replaced by the identity (its result is NaN anyway, and the sweeps of a NaN matrix would run to max_iter)
template <typename T, int N>
__device__ __forceinline__ bool expand(const T (&r)[sym_k(N)], T (&a)[N][N])
{
    bool bad = false;
#pragma unroll
    for (int k = 0; k < sym_k(N); ++k) bad |= !symfun::finite_t(r[k]);
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) a[i][j] = bad ? T(i == j) : r[sym_idx(N, i, j)];
    return bad;
}

// compact U diag(f) U^T, off-diagonal components times OFF (2 for a gradient); NaN if bad
template <typename T, int N, int OFF>
__device__ __forceinline__ void recompose(const T (&u)[N][N], const T (&f)[N], bool bad, T *o)
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T t[N];
#pragma unroll
        for (int k = 0; k < N; ++k) t[k] = u[i][k] * f[k];
#pragma unroll
        for (int j = i; j < N; ++j) {
            T y = t[0] * u[j][0];
#pragma unroll
            for (int k = 1; k < N; ++k) y = qr::fma_t(t[k], u[j][k], y);
            o[sym_idx(N, i, j)] = bad ? symfun::nan_t<T>() : (OFF == 1 || i == j ? y : T(OFF) * y);
        }
    }
}

} // namespace spectral
} // namespace nfm
