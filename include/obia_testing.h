/* obia_testing.h -- entry points that exist for the test suite: internal pieces of libobia_hip.so that no operator exposes on its
 * own, driven directly.  Not part of the operator ABI (include/obia_hip.h); bound by obia_amd/_lib.py as a table of its own.   */
#ifndef OBIA_TESTING_H
#define OBIA_TESTING_H

#include "obia_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The clear kernel that stands for several fills next to each other in stream order (a tile batch's buffers): sets
 * the `bytes[i]` bytes at device address `dev_ptrs[i]` to `values[i]` (its low byte), for i < n, and waits.  The three arrays are
 * host memory.  Sixteen ranges are one launch; more are split, one range alone is a plain fill.  Any address, any length (0: nothing
 * is written); nothing outside a range is touched.  OBIA_E_INVALID for a null array, n < 0, a negative length or a null address
 * with a length above 0.                                                                                                          */
int obia_test_clear_ranges_dev(obia_ctx *ctx, void *const *dev_ptrs, const int64_t *bytes, const int32_t *values, int n);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_TESTING_H */
