// wave_ops.hpp -- the device side's shared vocabulary: integer sums, prefix sums and ranks over a wave (64 lanes) and over a
// workgroup.  What the entry layer (common.hpp) is to the host side of an operator, this is to its kernels: a new kernel uses these
// and writes none of its own.  INTEGER types only: an integer sum is the same in any order, so every caller gets bit-identical
// results by construction; a floating-point reduction's order is part of its result and stays with its operator.
//
// The workgroup primitives (block_*, workgroup_exclusive_scan) are called by EVERY thread of a one-dimensional workgroup of exactly NT
// threads, from uniform control flow; their LDS is declared inside.  Each ends with a barrier, so that a second call -- the next
// trip of a loop -- cannot write that LDS before the slowest wave of the first call has read it.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <type_traits>

namespace obia {

// set bits of the ballot below this lane (mbcnt: no 64-bit shift by a register, tools/check_shift64.py)
__device__ __forceinline__ int lanes_below(unsigned long long ballot) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// the sum of v over the wave's 64 lanes, in every lane
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
    static_assert(std::is_integral_v<T>, "integer types only");
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the sum of v over this lane and the lanes below it
template <typename T> __device__ __forceinline__ T wave_inclusive_scan(T v) {
    static_assert(std::is_integral_v<T>, "integer types only");
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

template <int NT> constexpr bool is_block_size = NT % 64 == 0 && NT >= 64 && NT <= 1024;

// s_w[w] = wave w's value; returns the sum of the waves before the caller's, `total` = the sum of all.  The first barrier publishes
// s_w; the SECOND is the one that makes two calls in a row safe (no wave rewrites s_w while another still reads it).
template <int NT, typename T> __device__ __forceinline__ T waves_before(T *s_w, bool writer, T mine, T &total) {
    const int wv = threadIdx.x >> 6;
    if (writer) s_w[wv] = mine;
    __syncthreads();
    T before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const T c = s_w[w];
        if (w < wv) before += c;
        tot += c;
    }
    total = tot;
    __syncthreads();
    return before;
}

// the sum of v over the workgroup, in every thread
template <int NT, typename T> __device__ __forceinline__ T block_sum(T v) {
    static_assert(std::is_integral_v<T> && is_block_size<NT>, "integer types, whole waves up to 1024 threads");
    __shared__ T s_w[NT / 64];
    T total;
    (void)waves_before<NT>(s_w, (threadIdx.x & 63) == 0, wave_sum(v), total);
    return total;
}

// the sum of v over the threads before the caller; `total` = the workgroup's sum, in every thread
template <int NT, typename T> __device__ __forceinline__ T block_exclusive_scan(T v, T &total) {
    static_assert(std::is_integral_v<T> && is_block_size<NT>, "integer types, whole waves up to 1024 threads");
    __shared__ T s_w[NT / 64];
    const T inc = wave_inclusive_scan(v);
    return waves_before<NT>(s_w, (threadIdx.x & 63) == 63, inc, total) + inc - v;
}

// the number of threads before the caller whose flag is set; `total` = the workgroup's set flags, in every thread
template <int NT> __device__ __forceinline__ int block_flag_rank(bool flag, int &total) {
    static_assert(is_block_size<NT>, "whole waves up to 1024 threads");
    __shared__ int s_w[NT / 64];
    const unsigned long long bal = __ballot(flag);
    return waves_before<NT>(s_w, (threadIdx.x & 63) == 0, (int)__popcll(bal), total) + lanes_below(bal);
}

// out[i] = in[0] + ... + in[i - 1] for i < n, *total = the sum of all, by ONE workgroup of NT threads.  in == out is allowed;
// n == 0 writes only *total = 0.  Thread t owns the ceil(n / NT) consecutive elements from t * ceil(n / NT), clamped to n: it adds
// them up, the partial sums are scanned over the workgroup in Total's type, and it walks its elements again.  The offsets are stored
// narrowed to Out (a long long total with int offsets: the caller knows that every offset fits).
template <int NT, typename In, typename Out, typename Total>
__device__ __forceinline__ void workgroup_exclusive_scan(const In *in, Out *out, long long n, Total *total) {
    static_assert(std::is_integral_v<In> && std::is_integral_v<Out> && std::is_integral_v<Total>, "integer types only");
    const long long per = (n + NT - 1) / NT;
    const long long lo = min(n, (long long)threadIdx.x * per), hi = min(n, lo + per);
    Total s = 0;
    for (long long i = lo; i < hi; ++i) s += in[i];
    Total all;
    Total run = block_exclusive_scan<NT>(s, all);
    for (long long i = lo; i < hi; ++i) {
        const In v = in[i];
        out[i] = (Out)run;
        run += v;
    }
    if (threadIdx.x == 0) *total = all;
}

}  // namespace obia
#endif
