/*
 * obia_points.h -- point clouds (obia_amd/csrc/points.hip): points become a canopy height model and a density raster, points are
 * joined to the segments of a label raster, and the five point-cloud columns of the objects table (pai, fhd, ch, mean_intensity,
 * variance_intensity) are formed from the join.  segment_statistics.py:332-389 of the reference keeps the radiometric pair
 * (np.mean / np.var of Intensity); its structural code is gone (:326-329 raises), so the structural definitions below are this
 * project's.  DESIGN.md 3.5s.
 *
 * The conventions are those of obia_hip.h (status codes, one context per stream).  Every pointer is a DEVICE pointer unless it says
 * HOST.  Buffers need only the alignment of their element type.  Inputs, states and outputs of one call must not overlap.  Every call
 * returns with its work done.
 *
 * A CLOUD.  x, y (n) float64 map coordinates, z (n) float32 height above ground, intensity (n) uint16 or NULL.  0 <= n < 2^31 per
 * call (n >= 2^31: OBIA_E_UNSUPPORTED); n == 0 does nothing.  inv6: HOST, six doubles [a, b, d, e, xoff, yoff] of the INVERSE
 * transform in the layout of obia_sample_labels_i32_dev.
 *
 * THE PIXEL RULE (obia_sample_labels_i32_dev's).  In float64, separate multiplies and adds, left to right:
 *     col = floor(a * X + b * Y + xoff),   row = floor(d * X + e * Y + yoff);
 * the point is inside the raster when 0 <= col < W and 0 <= row < H, and its pixel is (row, col).  A NaN or infinite coordinate is
 * outside.
 *
 * THE KEY of a float32 z (zonal.hip's): its bits with the sign bit set when z >= 0, all bits inverted otherwise -- unsigned order is
 * numeric order, and no finite z has the key 0.
 *
 * STATE.  The accumulating calls ADD to caller-owned arrays that start all zero; a cloud may be cut into any number of calls in any
 * order.  Every sum is an integer and every update an integer atomic, so the state does not depend on the order of the points, on
 * the cut or on the schedule.  A uint32 count wraps past 2^32 - 1: the caller keeps the total below that.
 *
 * obia_points_rasters_dev : zkey (H, W) uint32: the maximum key over the pixel's points with finite z, 0: none;  count (H, W) uint32:
 *     every point inside the raster, whatever its z.
 * obia_points_rasters_finish_dev : chm (H, W) float32: the z behind zkey, NaN where zkey == 0;  density (H, W) float32 =
 *     (float)count / (float)pixel_area (one IEEE float32 division), pixel_area = |a e - b d| of the FORWARD transform, finite and > 0.
 *     Writes every element of both outputs.
 * obia_points_segments_dev : labels (H, W) int32; the row of a point is s = label of its pixel - start_label, points with s outside
 *     [0, N) have no row.  N >= 0 (no pointer may be NULL even then), 1 <= nz <= OBIA_POINTS_MAX_NZ and N * nz < 2^31
 *     (OBIA_E_UNSUPPORTED beyond); dz finite and > 0 (OBIA_E_INVALID otherwise).
 *         profile (N, nz) uint32 : bin j = (int)floor((double)z / dz), only for finite z with z >= 0 and j < nz;
 *         top (N) uint32         : the maximum key of z over the points that entered the profile;
 *         n_int (N) uint32, s1 (N) uint64, s2 (N) uint64 : count, sum and sum of squares of the intensity over EVERY point with a
 *                                  row, whatever its z; untouched when intensity is NULL;
 *         counters (4) uint64    : points outside the raster; inside without a row; with a row but not in the profile; in the profile.
 *     One workgroup takes OBIA_POINTS_CHUNK consecutive points at a time and sums equal (row, bin) keys and equal rows in two LDS
 *     hash tables (OBIA_POINTS_TABLE and OBIA_POINTS_ROWS slots), then flushes one global atomic per occupied slot and value.  A key
 *     that finds no slot within OBIA_POINTS_PROBES probes goes to global memory directly, so a chunk with more distinct keys than
 *     slots is as right as any other.
 * obia_points_segment_columns_dev : reads the state, writes (N) columns; one lane per segment, sums over j ascending from 0.
 *     With c[j] the profile of a segment, j0 = (int)ceil(min_height / dz) in float64 clamped to 0 .. nz, n_all = sum c[j],
 *     n_below = sum over j < j0, n_can = n_all - n_below, all float64 arithmetic, log the device library's:
 *         n_points (int64) = n_all
 *         ch   = the float32 behind top, widened; NaN when n_all == 0
 *         pai  = log((double)n_all / (double)n_below) / k; NaN when n_all == 0 or n_below == 0
 *         fhd  = -(sum over j >= j0 with c[j] > 0 of p * log(p)), p = (double)c[j] / (double)n_can, added from 0.0; NaN when n_can == 0
 *         mean_intensity     = (double)s1 / (double)n_int
 *         variance_intensity = (double)(n_int * s2 - s1 * s1) / ((double)n_int * (double)n_int), the numerator exact in 128 bits and
 *                              converted as (double)high * 2^64 + (double)low; both NaN when n_int == 0
 *         pad (N, nz) float64 or NULL: with E_j = sum over i <= j of c[i], T_j = E_j - c[j]:
 *                              NaN where E_j == 0;  0 where c[j] == 0 < E_j;  NaN where T_j == 0 < c[j];
 *                              log((double)E_j / (double)T_j) / (k * dz) otherwise.
 *     min_height finite, k finite and > 0, dz finite and > 0: OBIA_E_INVALID otherwise.  Writes every element of every output.
 */
#ifndef OBIA_POINTS_H
#define OBIA_POINTS_H

#include "obia_hip.h"

#define OBIA_POINTS_MAX_NZ 4096
#define OBIA_POINTS_CHUNK 2048
#define OBIA_POINTS_TABLE 2048
#define OBIA_POINTS_ROWS 512
#define OBIA_POINTS_PROBES 8

#ifdef __cplusplus
extern "C" {
#endif

int obia_points_rasters_dev(obia_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, const double *inv6, int H, int W,
                            uint32_t *zkey, uint32_t *count);
int obia_points_rasters_finish_dev(obia_ctx *ctx, const uint32_t *zkey, const uint32_t *count, int H, int W, double pixel_area, float *chm,
                                   float *density);
int obia_points_segments_dev(obia_ctx *ctx, const double *x, const double *y, const float *z, const uint16_t *intensity, int64_t n,
                             const double *inv6, const int32_t *labels, int H, int W, int32_t start_label, int32_t N, int32_t nz, double dz,
                             uint32_t *profile, uint32_t *top, uint32_t *n_int, uint64_t *s1, uint64_t *s2, uint64_t *counters);
int obia_points_segment_columns_dev(obia_ctx *ctx, const uint32_t *profile, const uint32_t *top, const uint32_t *n_int, const uint64_t *s1,
                                    const uint64_t *s2, int32_t N, int32_t nz, double dz, double min_height, double k, int64_t *n_points,
                                    double *ch, double *pai, double *fhd, double *mean_intensity, double *variance_intensity, double *pad);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_POINTS_H */
