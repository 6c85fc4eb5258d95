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

/* The connectivity stage (obia_amd/csrc/cc.hip: enforce_connectivity_batch) on a batch of label maps, as the tiler calls it but with
 * every setting the caller's: the same entry layer and argument checks as obia_enforce_connectivity_i32_dev, per problem.
 *   labels_in     device memory: the label maps back to back in problem order, each H * W int32 in row-major order
 *   problems      host memory: n_problems rows {H, W, min_size, max_size} (max_size below 1 counts as 1); a problem's pixels start at
 *                 the sum of H * W of the rows before it
 *   start_label   0 or 1; start_label - 1 marks a masked pixel
 *   labels_out    device memory of the same layout; n_labels_out (host, nullable) receives the number of surviving components
 * The rule it pins: problems do not see each other -- equal labels on the last row of one and the first row of the next stay two
 * components -- and surviving components (size >= the min_size of their problem, after the cut at its max_size) are numbered from
 * start_label over the WHOLE batch, in problem order and within a problem in raster order of their first pixel.  A small component
 * takes the final label of the neighbour the reference's walk meets last; one that never finds a labelled neighbour is the literal 0
 * (with start_label 1 that is the masked label; with start_label 0 it is also the label of the batch's first surviving component).
 * OBIA_E_INVALID, before any device work, for a null pointer, n_problems outside 1 .. 65535, a shape below 1 and a batch of 2^31
 * pixels or more.                                                                                                                  */
int obia_test_enforce_connectivity_batch_dev(obia_ctx *ctx, const int32_t *labels_in, const int64_t *problems, int n_problems,
                                             int start_label, int32_t *labels_out, int *n_labels_out);

/* What the last enforce_connectivity_batch of the context decided (through whichever entry point: a SLIC call, the tiler, the stage
 * alone): reset at the start of that function, filled with profiling on or off, all zero before the first call.  `out` receives
 * OBIA_TEST_CC_REPORT_FIELDS values, in this order:
 *    0  problems
 *    1  pixels
 *    2  surviving components
 *    3  small components (below their problem's min_size)
 *    4  pixels of the small components
 *    5  components cut at max_size (those of at least max_size pixels in the first count; 0: no cut ran, and 2 .. 4 are the first
 *       count's -- otherwise they are the counts after the cut)
 *    6  code[] used (0 / 1): the dense one-word-per-pixel pass
 *    7  evaluation: 0 none (no small component), 1 walks (cc_small_bfs_kernel), 2 pixel lists (cc_settle_eval_kernel)
 *    8  side the settle rounds started on: 0 from below, 1 from above (0 when no round ran)
 *    9  rounds run from below
 *   10  rounds run from above
 *   11  visited map reallocated by this call (0 / 1)
 * A round is one evaluation launch and its read-back.  OBIA_E_INVALID for a null context, a null `out` or n below the field count. */
#define OBIA_TEST_CC_REPORT_FIELDS 12
int obia_test_cc_report(obia_ctx *ctx, int64_t *out, int n);

/* A used context with KNOWN contents (tests/test_gpu_workspace_history.py): every workspace buffer comes from a bump allocator that
 * keeps its memory between calls, so an operator must write each buffer before it reads it.  Waits for the context's stream and
 * side stream, makes the arena ONE block of at least reserve_bytes (it allocates, then resets: several blocks are merged, so the
 * next call's frame neither frees nor grows as long as the operator needs no more than the block), and sets every byte of the block
 * -- its whole size, not reserve_bytes -- to `byte`.  The pinned host areas are filled too: the read-back buffer, the upload ring
 * when no upload is queued, the deferred read-back's landing area when none is pending.  The visited map of the connectivity
 * stage is NOT touched: its contract is "all zero between calls", and visited_nonzero_out (nullable) receives the number of its
 * words that are not zero -- 0 when the map does not exist or is flagged dirty (the next call clears it).  held_out (nullable)
 * receives obia_workspace_bytes().  Plain fills only: hipMemsetAsync and host memset.
 * OBIA_E_INVALID for a null context, a byte outside 0 .. 255, a negative reserve_bytes and a context held by an open tiler session
 * (nothing is touched); OBIA_E_NOMEM when the block cannot be allocated.                                                          */
int obia_test_poison_workspace_dev(obia_ctx *ctx, int64_t reserve_bytes, int byte, int64_t *held_out, int64_t *visited_nonzero_out);

/* The visited map's count alone, as obia_test_poison_workspace_dev reports it, with nothing written: waits for the context's
 * streams and counts.  Reads only, so a context held by a session is served.  OBIA_E_INVALID for a null context or output.       */
int obia_test_visited_nonzero(obia_ctx *ctx, int64_t *visited_nonzero_out);

/* One primitive of obia_amd/csrc/wave_ops.hpp -- the integer sums, prefix sums and ranks every kernel of the library shares -- on n
 * int32 values in device memory, with `nt` threads per workgroup; waits.  `op`:
 *   0  workgroup_exclusive_scan, int32 -> int32 IN PLACE, int64 total        nt 1024
 *   1  workgroup_exclusive_scan, int32 -> int32 out of place, int32 total    nt 1024
 *   2  workgroup_exclusive_scan, int32 -> int64                              nt 256, 1024
 *   3  block_exclusive_scan                                                  nt 256, 1024
 *   4  block_sum (every thread's result is its workgroup's sum)              nt 256, 1024
 *   5  block_flag_rank of in[i] != 0                                         nt 256
 *   6  block_exclusive_scan of in[i], then at once of in[i] + 1: the second  nt 256, 1024
 * Ops 0 .. 2 run ONE workgroup: out[i] = in[0] + ... + in[i - 1], totals_out[0] = the sum (n = 0 writes only that).  Ops 3 .. 6 run
 * ceil(n / nt) workgroups, workgroup g on in[g * nt ..): out[i] = the result of element i's thread, totals_out[g] = the total the
 * primitive hands back (the last workgroup may be partial: its spare threads take part with nothing; n = 0 writes nothing).
 * Results are widened to int64: out holds n, totals_out one per workgroup.  No workspace is taken.
 * The (op, nt) pairs served are EXACTLY the instantiations the library's own kernels use, as listed above: another nt, or another
 * op, is OBIA_E_INVALID, and so are a null or misaligned buffer, out == totals_out and a negative n.                            */
int obia_test_wave_ops_dev(obia_ctx *ctx, int op, int nt, const int32_t *in, int64_t n, int64_t *out, int64_t *totals_out);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_TESTING_H */
