// svr_rank_select.hpp -- the median of an odd number N of values by a fixed sequence of compare-exchanges on statically indexed
// values (svr_filter.hip).  T is an unsigned integer, or a vector of them (a packed pair of u16: its two halves are
// then selected independently by the same instructions, v_pk_min_u16 / v_pk_max_u16).
//
// The scheme is "forgetful selection": the median of N = 2 m + 1 values is neither the smallest nor the largest of any m + 2 of them,
// so take m + 2 values, move their smallest and largest to the two ends (minmax_ends), forget both, admit the next value, and go on
// with one value fewer; after m rounds three are left and their middle one is the median.  minmax_ends<K> pairs value i with value
// K - 1 - i -- after which the smallest is in the lower half and the largest in the upper half (the middle value of an odd K counts to
// both) -- and then scans each half: K / 2 + 2 ((K - 1) / 2) compare-exchanges, at most 3 K / 2.  N = 7 / 19 / 27 take 13 / 79 / 153 of them.
#pragma once

namespace svr_rank {

template <typename T> __host__ __device__ inline T rank_min(T a, T b) { return __builtin_elementwise_min(a, b); }
template <typename T> __host__ __device__ inline T rank_max(T a, T b) { return __builtin_elementwise_max(a, b); }

template <typename T>
__host__ __device__ inline void cex(T& lo, T& hi)
{
    const T a = rank_min(lo, hi);
    hi = rank_max(lo, hi);
    lo = a;
}

// afterwards v[0] is the smallest and v[K - 1] the largest of v[0 .. K - 1]; the rest is a permutation of the rest
template <int K, typename T>
__host__ __device__ inline void minmax_ends(T* v)
{
#pragma unroll
    for (int i = 0; i < K / 2; ++i) cex(v[i], v[K - 1 - i]);
#pragma unroll
    for (int i = 1; i <= (K - 1) / 2; ++i) cex(v[0], v[i]);
#pragma unroll
    for (int i = K / 2; i < K - 1; ++i) cex(v[i], v[K - 1]);
}

template <int K, int NEXT, typename T>
__host__ __device__ inline T forget(T* v, const T* w)
{
    minmax_ends<K>(v);
    if constexpr (K == 3) {
        return v[1];
    } else {
        v[0] = w[NEXT];                                   // the smallest is forgotten; the largest, v[K - 1], falls off the end
        return forget<K - 1, NEXT + 1>(v, w);
    }
}

// the value of rank N / 2 (0-based) of w[0 .. N - 1], N odd and >= 3
template <int N, typename T>
__host__ __device__ inline T median(const T* w)
{
    static_assert(N % 2 == 1 && N >= 3, "an odd count");
    constexpr int K0 = N / 2 + 2;
    T v[K0];
#pragma unroll
    for (int i = 0; i < K0; ++i) v[i] = w[i];
    return forget<K0, K0>(v, w);
}

} // namespace svr_rank
