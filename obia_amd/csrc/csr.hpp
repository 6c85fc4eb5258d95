// csr.hpp -- a CSR the caller passes (obia_adjacency.h: "A CSR THE CALLER PASSES"), for the table kernels of adjacency.hip and
// merging.hip: how an entry point lists its buffers, how it hands them to a kernel, and how a kernel reads them defensively.
//
// The namespace without a name is meant: the kernels that take a Csr are local to their translation unit, and so is what they take.
#pragma once
#include "common.hpp"

namespace obia {
namespace {

struct Csr {
    const long long *indptr; const int *neighbor; const long long *border;
    int N; long long nnz;
};
// indptr whenever there is a row, neighbor (and border, where the call takes it) whenever there is an entry
[[maybe_unused]] Buffers &list_csr(Buffers &b, const int64_t *indptr, const int32_t *neighbor, int32_t N, int64_t nnz) {
    return b.in(indptr, N > 0).in(neighbor, nnz > 0);
}
[[maybe_unused]] Buffers &list_csr(Buffers &b, const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t N, int64_t nnz) {
    return list_csr(b, indptr, neighbor, N, nnz).in(border, nnz > 0);
}
[[maybe_unused]] Csr csr_of(const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t N, int64_t nnz) {
    return Csr{reinterpret_cast<const long long *>(indptr), neighbor, reinterpret_cast<const long long *>(border), N, (long long)nnz};
}

__device__ __forceinline__ void row_range(const Csr &G, int i, long long &lo, long long &hi) {
    lo = G.indptr[i];
    hi = G.indptr[i + 1];
    if (lo < 0) lo = 0;
    if (hi > G.nnz) hi = G.nnz;
}
// the row of entry e: the largest i in 0 .. N - 1 with indptr[i] <= e (N >= 1)
__device__ __forceinline__ int row_of(const Csr &G, long long e) {
    int lo = 0, hi = G.N;                                        // indptr[lo] <= e < indptr[hi], by convention at the ends
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (G.indptr[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ bool is_real(const Csr &G, int j) { return j >= 0 && j < G.N; }

}  // namespace
}  // namespace obia
