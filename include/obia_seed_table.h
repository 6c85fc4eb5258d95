/*
 * obia_seed_table.h -- the table options of the canonical seeds (obia_amd/csrc/seed_table.hip): heights sampled from a raster, the
 * adaptive-radius pre-clustering (stage 1), the per-cluster passes behind the height split and the trim, and the non-maximum
 * suppression inside a cluster.  obia/utils/seeds.py:105-136, 193-213, 233-253 of the reference; DESIGN.md 3.5q.
 *
 * The conventions are those of obia_hip.h (status codes, one context per stream, the output contract).  Every pointer is a DEVICE
 * pointer unless it says HOST.  Buffers need only the alignment of their element type.  Inputs and outputs of one call must not
 * overlap.  Every call returns with its work done.  n is the number of seeds, 1 .. 2^31 - 1 (OBIA_E_INVALID otherwise); every output
 * has n elements and every one of them is written.
 *
 * The distance predicate, everywhere: seed j lies in the ball of radius r around seed i when, in float64 and uncontracted,
 *     dx = x_i - x_j, dy = y_i - y_j, dx * dx + dy * dy <= r * r.
 *
 * THE GRID.  A ball is searched on a uniform grid whose cell side is not smaller than the largest radius in play, so it lies within
 * the 3 x 3 cells around its centre.  The grid takes memory in proportion to n, whatever the extent: the caller sorts the seeds by
 * the cell key  key = (cy - cy0 + 1) * ncx + (cx - cx0 + 1),  cx0 / cy0 the smallest cell indices and ncx = cxmax - cx0 + 3 (one empty
 * column on either side, so that key - 1 and key + 1 never leave a row), and hands over the table IN THAT ORDER with the sorted keys;
 * a cell's run is found by binary search.  The keys must ascend; keys that do not give wrong answers and no access out of bounds.
 *
 * obia_seedtab_cells_dev   : cx_out, cy_out (n) int32 = floor(x / side), floor(y / side) in float64, clamped to +-2^30; side > 0.
 * obia_seedtab_sample_dev  : chm (H, W) float32; inv6 (HOST, 6 doubles: ra rb rc rd re rf of the inverse geotransform).  For every
 *     point col = floor((ra x + rb y) + rc), row = floor((rd x + re y) + rf); height_out (n) float32 = chm[row, col] and valid_out (n)
 *     bytes = 1 when the pixel is inside the raster and not NaN, else NaN and 0.
 * obia_seedtab_stage1_dev  : xs, ys (n) float64, hs (n) float32, orig (n) int32 the row of the unsorted table, key (n) int64, all in
 *     cell order.  eps_i = min(max(eps_scale * h_i, min_eps), max_eps) in float32 (the three are given as float32), then float64;
 *     the cell side must be >= max_eps.  eligible(i): the ball of eps_i around i holds at least min_samples seeds (itself included) and,
 *     when z_thresh >= 0, max - min of their heights, subtracted in float32, does not exceed z_thresh.  With d(i, j) <= eps_i meaning
 *     that j lies in the ball of i, and "<" the order of orig:
 *         fired(i) = eligible(i) and no i' < i with fired(i') and d(i', i) <= eps_i'
 *     fired_out (n) bytes 0 / 1; owner_out (n) int32 = the largest orig among the fired i with d(i, j) <= eps_i, -1 when there is none.
 *     Both in cell order.  Decided in rounds: a round decides every seed whose eligible earlier coverers are all decided; the lowest
 *     undecided seed always is, so n rounds suffice, and the count does not depend on the schedule (a round reads only what the round
 *     before it wrote).  OBIA_E_INTERNAL when n rounds did not suffice: a defect.  rounds_out (HOST int32, may be NULL).
 * obia_seedtab_last_work   : work_out (HOST, 2 x int64): rounds and seeds of the calling thread's last obia_seedtab_stage1_dev that
 *     returned OBIA_OK.
 * obia_seedtab_segments_dev: cluster (n) int32 ascending and, inside a run of equal values, heights (n) float32 descending: the table
 *     sorted by (cluster, height descending, row).  rank_out (n) int32: position inside the run; size_out (n) int32: its length;
 *     part_out (n) bytes: 1 when dz_merge > 0, the run's first height minus its last (float32) exceeds dz_merge and the row's height
 *     exceeds the run's median, else 0.  The median of an even run is the mean of the two middle heights taken in float32 (pandas'
 *     median of a float32 column).  A run is found by binary search: one cluster of n rows costs what n clusters of one row cost.
 * obia_seedtab_nms_dev     : xs, ys, hs, cluster (n) int32, pos (n) int32 -- the row's position in the (cluster, height descending,
 *     row) order -- and key, all in cell order; r_i = scale * (double)h_i when that exceeds base, else base; the cell side must be
 *     >= every r_i.  keep_out (n) bytes, cell order: 0 when some i of the same cluster with pos_i > pos_j has d(i, j) <= r_i, else 1.
 */
#ifndef OBIA_SEED_TABLE_H
#define OBIA_SEED_TABLE_H

#include "obia_crowns.h"

#ifdef __cplusplus
extern "C" {
#endif

int obia_seedtab_cells_dev(obia_ctx *ctx, const double *xs, const double *ys, int64_t n, double side, int32_t *cx_out, int32_t *cy_out);
int obia_seedtab_sample_dev(obia_ctx *ctx, const double *xs, const double *ys, int64_t n, const float *chm, int H, int W,
                            const double *inv6, float *height_out, uint8_t *valid_out);
int obia_seedtab_stage1_dev(obia_ctx *ctx, const double *xs, const double *ys, const float *hs, const int32_t *orig, const int64_t *key,
                            int64_t n, int64_t ncx, float eps_scale, float min_eps, float max_eps, float z_thresh, int min_samples,
                            uint8_t *fired_out, int32_t *owner_out, int32_t *rounds_out);
int obia_seedtab_last_work(obia_ctx *ctx, int64_t *work_out);
int obia_seedtab_segments_dev(obia_ctx *ctx, const int32_t *cluster, const float *heights, int64_t n, float dz_merge, int32_t *rank_out,
                              int32_t *size_out, uint8_t *part_out);
int obia_seedtab_nms_dev(obia_ctx *ctx, const double *xs, const double *ys, const float *hs, const int32_t *cluster, const int32_t *pos,
                         const int64_t *key, int64_t n, int64_t ncx, double base, double scale, uint8_t *keep_out);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_SEED_TABLE_H */
