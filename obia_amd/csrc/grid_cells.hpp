// grid_cells.hpp -- the neighbourhood walk on the uniform grid of include/obia_seed_table.h, shared by seed_table.hip and boxes.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace obia {

// f(q) for every q in the 3 x 3 cells around the cell `key`: per grid row at most 32 steps of a binary search and a run of < n rows
template <typename F> __device__ __forceinline__ void for_cells(const long long *__restrict__ skey, int n, long long key, long long ncx,
                                                                F &&f) {
    for (int dy = -1; dy <= 1; ++dy) {
        const long long k0 = key + dy * ncx - 1, k1 = k0 + 2;
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (skey[mid] < k0) lo = mid + 1; else hi = mid;
        }
        for (int q = lo; q < n && skey[q] <= k1; ++q) f(q);
    }
}

}  // namespace obia
