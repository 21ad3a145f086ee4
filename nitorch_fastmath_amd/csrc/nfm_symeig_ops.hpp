// nfm_symeig_ops.hpp -- what sym_eigvals / sym_eigh add to a decomposition in deflation order: the sort of the
// eigenpairs, the sign rule of the eigenvectors and the gap weights of the gradient, for ONE record.  Everything is
// __host__ __device__: the kernels of nfm_symeig.hip and the CPU entry nfm_sym_eigh_host_finish run the same source, so
// the host tests check the order, the signs and the gap rule the GPU applies.
//
// The sort is a fixed compare-exchange network over (key, value, column), taken with selects at LITERAL indices only
// (the pairs are template arguments): a register matrix indexed by a run-time rank goes to scratch memory (see
// for_lower_static in nfm_qr_core.hpp and the header of nfm_spectral.hpp for what that costs here).  The order is a
// wave-uniform run-time member of Params: it only chooses the key.
//   ascending   key = value
//   descending  key = -value
//   abs         key = |value|, ties by the value ascending (|l1| <= |l2| <= ..., the Frangi / Sato convention)
// Ties of the key are broken by the sign (of the key; of the value for 'abs'), so that -0.0 sorts before +0.0 in
// ascending order and after it in descending order: the order is total on the bit patterns, 'descending' is the exact
// reverse of 'ascending' and 'abs' a permutation of the same bits.
#pragma once
#include "nfm_symfun_ops.hpp"

namespace nfm {
namespace symeig {

struct OrderParams {
    int order; // NFM_EIGH_ASCENDING / _DESCENDING / _ABS
};

constexpr bool order_ok(int order) { return order >= NFM_EIGH_ASCENDING && order <= NFM_EIGH_ABS; }

template <typename T>
NFM_HD T copysign_t(T m, T s)
{
    return T(__builtin_copysign(double(m), double(s)));
}
template <>
NFM_HD float copysign_t<float>(float m, float s)
{
    return __builtin_copysignf(m, s);
}

template <typename T>
NFM_HD T key_of(int order, T lam)
{
    return order == NFM_EIGH_ABS ? symfun::abs_t(lam) : (order == NFM_EIGH_DESCENDING ? -lam : lam);
}

// The networks: the shortest known for each order (1, 3, 5, 9, 12, 16, 19 exchanges; the 0-1 principle over all 2^N
// inputs checks them in tests/test_symeig_host.py through nfm_sym_eigh_host_finish).
template <int N>
struct Net;
template <>
struct Net<1> {
    static constexpr int len = 0;
    static constexpr int at[1][2] = {{0, 0}};
};
template <>
struct Net<2> {
    static constexpr int len = 1;
    static constexpr int at[len][2] = {{0, 1}};
};
template <>
struct Net<3> {
    static constexpr int len = 3;
    static constexpr int at[len][2] = {{0, 2}, {0, 1}, {1, 2}};
};
template <>
struct Net<4> {
    static constexpr int len = 5;
    static constexpr int at[len][2] = {{0, 2}, {1, 3}, {0, 1}, {2, 3}, {1, 2}};
};
template <>
struct Net<5> {
    static constexpr int len = 9;
    static constexpr int at[len][2] = {{0, 3}, {1, 4}, {0, 2}, {1, 3}, {0, 1}, {2, 4}, {1, 2}, {3, 4}, {2, 3}};
};
template <>
struct Net<6> {
    static constexpr int len = 12;
    static constexpr int at[len][2] = {{0, 5}, {1, 3}, {2, 4}, {1, 2}, {3, 4}, {0, 3},
                                       {2, 5}, {0, 1}, {2, 3}, {4, 5}, {1, 2}, {3, 4}};
};
template <>
struct Net<7> {
    static constexpr int len = 16;
    static constexpr int at[len][2] = {{0, 6}, {2, 3}, {4, 5}, {0, 2}, {1, 4}, {3, 6}, {0, 1}, {2, 5},
                                       {3, 4}, {1, 2}, {4, 6}, {2, 3}, {4, 5}, {1, 2}, {3, 4}, {5, 6}};
};
template <>
struct Net<8> {
    static constexpr int len = 19;
    static constexpr int at[len][2] = {{0, 2}, {1, 3}, {4, 6}, {5, 7}, {0, 4}, {1, 5}, {2, 6}, {3, 7}, {0, 1}, {2, 3},
                                       {4, 5}, {6, 7}, {2, 4}, {3, 5}, {1, 4}, {3, 6}, {1, 2}, {3, 4}, {5, 6}};
};

// one exchange of the pairs I < J: after it (key, tie) of I is not above that of J
template <typename T, int N, bool WITH_U, int I, int J>
NFM_HD void exchange(bool abs_order, T (&key)[N], T (&lam)[N], T (&u)[WITH_U ? N : 1][WITH_U ? N : 1])
{
    const T ti = copysign_t(T(1), abs_order ? lam[I] : key[I]), tj = copysign_t(T(1), abs_order ? lam[J] : key[J]);
    const bool sw = key[I] > key[J] || (key[I] == key[J] && ti > tj);
    const T ki = key[I], li = lam[I];
    key[I] = sw ? key[J] : ki;
    key[J] = sw ? ki : key[J];
    lam[I] = sw ? lam[J] : li;
    lam[J] = sw ? li : lam[J];
    if constexpr (WITH_U) {
#pragma unroll
        for (int r = 0; r < N; ++r) {
            const T x = u[r][I];
            u[r][I] = sw ? u[r][J] : x;
            u[r][J] = sw ? x : u[r][J];
        }
    }
}

template <typename T, int N, bool WITH_U, int C = 0>
NFM_HD void run_net(bool abs_order, T (&key)[N], T (&lam)[N], T (&u)[WITH_U ? N : 1][WITH_U ? N : 1])
{
    if constexpr (C < Net<N>::len) {
        exchange<T, N, WITH_U, Net<N>::at[C][0], Net<N>::at[C][1]>(abs_order, key, lam, u);
        run_net<T, N, WITH_U, C + 1>(abs_order, key, lam, u);
    }
}

// sort the eigenvalues (and the columns of u with them) into `order`
template <typename T, int N, bool WITH_U>
NFM_HD void sort_pairs(int order, T (&lam)[N], T (&u)[WITH_U ? N : 1][WITH_U ? N : 1])
{
    T key[N];
#pragma unroll
    for (int k = 0; k < N; ++k) key[k] = key_of(order, lam[k]);
    run_net<T, N, WITH_U>(order == NFM_EIGH_ABS, key, lam, u);
}

// the sign rule: the component of largest magnitude of every column is positive (the first such component among
// exact ties)
template <typename T, int N>
NFM_HD void fix_signs(T (&u)[N][N])
{
#pragma unroll
    for (int k = 0; k < N; ++k) {
        T m = symfun::abs_t(u[0][k]), top = u[0][k];
#pragma unroll
        for (int r = 1; r < N; ++r) {
            const T v = symfun::abs_t(u[r][k]);
            const bool up = v > m;
            top = up ? u[r][k] : top;
            m = up ? v : m;
        }
        const bool flip = top < T(0);
#pragma unroll
        for (int r = 0; r < N; ++r) u[r][k] = flip ? -u[r][k] : u[r][k];
    }
}

template <typename T>
struct Eps;
template <>
struct Eps<float> {
    static constexpr float value = 1.1920928955078125e-07f; // 2^-23
};
template <>
struct Eps<double> {
    static constexpr double value = 2.220446049250313080847263336181640625e-16; // 2^-52
};

// THE GAP RULE.  Eigenvalues closer than 16 n eps max_i |l_i| -- the bar the sweeps are held to -- are numerically
// one eigenspace: their pair gets the weight 0 instead of 1 / (l_l - l_k).
template <typename T, int N>
NFM_HD T gap_tol(const T (&lam)[N])
{
    T m = symfun::abs_t(lam[0]);
#pragma unroll
    for (int k = 1; k < N; ++k) {
        const T v = symfun::abs_t(lam[k]);
        m = v > m ? v : m;
    }
    return T(16 * N) * Eps<T>::value * m;
}
// 1 / (l_l - l_k) under the gap rule, k != l
template <typename T>
NFM_HD T gap_weight(T lk, T ll, T tol)
{
    const T d = ll - lk;
    return symfun::abs_t(d) <= tol ? T(0) : T(1) / d;
}

} // namespace symeig
} // namespace nfm
