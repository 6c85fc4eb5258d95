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

/* The plan of a batch's sweeps (obia_amd/csrc/slic_sweep_plan.hpp: plan_sweeps) as text, for a batch made up from shapes.  No
 * context and no GPU: pure host code.
 *   problems     n_problems rows {H, W, K, sy, sx, n_valid, grid_n}: window size, centroids, window steps, valid pixels, the n the
 *                seeds were laid out for by the grid rule (0: none).  Sweep tiles, bins and the running offsets follow from them.
 *   settings     {C, masked, max_iter, prepass_iter, prepass_only, exit_on_fixed_point, slic_zero, direct, col_lb (colour boxes
 *                present), fuse_features (raster and keys present), mask already packed}
 *   repeat       the batch runs again with every sweep storing its labels
 *   switches     {OBIA_DEBUG_SYNC, OBIA_PREP_GROUPED, OBIA_PREPASS_VISITS set (0 / 1); OBIA_PREPASS_SHARE (0: off);
 *                OBIA_PREPASS_GROUPS, OBIA_SWEEP_GROUPS (0, 1, 2)} -- given here, not read from the environment
 *   residencies  {spatial kernel, colour kernel}: workgroups the device holds at once
 *   text         receives one command per line in queue order, every launch with its stream ("s0": the context's, "s1": the side
 *                stream), zero-terminated; OBIA_E_INVALID when text_bytes is too small.
 * Returns what the driver would: OBIA_E_UNSUPPORTED / OBIA_E_INVALID with the error text for a batch it refuses.                  */
int obia_test_sweep_plan(const int64_t *problems, int n_problems, const int32_t *settings, int repeat, const int32_t *switches,
                         const int64_t *residencies, char *text, int64_t text_bytes);

/* The grid of a clamped launch (obia_amd/csrc/launch_grids.hpp) by its name there.  No context and no GPU: pure host code.
 *   name     a launch of the table in launch_grids.hpp, e.g. "flat", "image_rows", "cost_sobel"
 *   sizes    the n_sizes sizes that launch's function takes, in its order (obia_test_launch_grid_names lists them), each in
 *            1 .. 2^31 - 1: a raster side, a row count, or a flat count (`np`, the problems of a batch: 65535 at the most); products are
 *            formed in 64 bits
 *   out4     receives {grid.x, grid.y, trips.x, trips.y}: the workgroups per axis and, per axis, the trips of the stride loop of the
 *            workgroup with the most work -- 1 up to the clamp, 2 from one unit of work past it.  A unit is what the launch
 *            expression gives one workgroup per trip (256 elements or chunks, a row, a tile row, a box).
 * OBIA_E_INVALID with the error text for an unknown name, a wrong n_sizes or a size out of range.                                */
int obia_test_launch_grid(const char *name, const int64_t *sizes, int n_sizes, int64_t *out4);

/* The names obia_test_launch_grid knows, one per line: "name size size ...", zero-terminated; OBIA_E_INVALID when text_bytes is too
 * small.                                                                                                                        */
int obia_test_launch_grid_names(char *text, int64_t text_bytes);

/* The largest number of new ids of one obia_tiler_import_seam that is ranked by the one-workgroup sort in LDS; an import that
 * brings more is ranked by counting.  A constant of the build: no context and no GPU.                                           */
int obia_test_seam_sort_limit(void);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_TESTING_H */
