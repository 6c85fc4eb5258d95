/*
 * obia_ground.h -- height above ground from raw elevations (obia_amd/csrc/ground.hip): every point of a cloud against the k nearest
 * ground points, or against a terrain raster.  The definitions are this project's, modelled on PDAL's filters.hag_nn and
 * filters.hag_dtm; they are NOT compared with PDAL anywhere.  DESIGN.md 3.5t.
 *
 * The conventions are those of obia_hip.h (status codes, one context per stream).  Every pointer is a DEVICE pointer unless it says
 * HOST.  Buffers need only the alignment of their element type.  Inputs and outputs of one call must not overlap.  Every call returns
 * with its work done.
 *
 * THE GROUND SET.  gx, gy, gz (ng) float64, all finite, 1 <= ng < 2^31, and gidx (ng) int32: the index i of each ground point in the
 * caller's order.  The arrays are stored in CELL ORDER of a uniform grid of ncx x ncy cells of `side`:
 *     cell of a point = (floor(gy / side) - cy0) * ncx + (floor(gx / side) - cx0)   (float64 division, obia_seedtab_cells_dev's),
 * every cell of the ground set inside the grid, points of one cell in any order.  cell_start (ncx * ncy + 1) int32: the points of
 * cell k are the positions cell_start[k] .. cell_start[k + 1] - 1.  side finite and > 0, |v / side| < 2^30 for every ground
 * coordinate v, ncx, ncy >= 1 and ncx * ncy <= 4 ng + 16 (memory is O(ng); OBIA_E_INVALID otherwise).  The caller builds the index
 * (obia_amd.pointcloud.GroundIndex); the kernel trusts its contents but never reads outside cell_start[0 .. ncx * ncy] and
 * positions 0 .. ng - 1.
 *
 * A QUERY (x, y) float64 with 1 <= count <= OBIA_GROUND_MAX_COUNT and max_distance >= 0 (0: no limit).  All float64, separate
 * multiplies and adds, nothing contracted:
 *     d2_i = (x - gx_i) * (x - gx_i) + (y - gy_i) * (y - gy_i)
 * The neighbours are the `count` smallest by the pair (d2_i, i) among those with d2_i <= max_distance * max_distance (the product
 * formed once; the test applies only when max_distance > 0); m is how many there are.  zg is
 *     NaN                                         when x or y is not finite, or m == 0;
 *     gz of the first neighbour                   when m == 1 or its d2 == 0;
 *     (sum_j gz_j / d2_j) / (sum_j 1 / d2_j)      otherwise: both sums from 0.0, j in neighbour order, a term one division, one add.
 * hag = (float)(z - zg), one rounding.  Every NaN that is written is the quiet NaN 0x7ff8000000000000 / 0x7fc00000.
 *
 * obia_ground_query_dev : x, y (n) float64; z (n) float64 with hag (n) float32, or both NULL; zg (n) float64; m (n) uint8 or NULL.
 *     0 <= n < 2^31 (n >= 2^31: OBIA_E_UNSUPPORTED); n == 0 does nothing.  Writes every element of every output given.  One lane per
 *     query walks the rings of cells around the query's cell (clamped into the grid) and stops after ring r >= 1 when it holds `count`
 *     neighbours whose worst d2 < (r side)^2 (1 - 2^-20), when max_distance > 0 and that bound exceeds max_distance^2, or when the ring
 *     covered the grid (DESIGN.md 3.5t has the argument).  A ring costs two steps and its cells inside the grid, so a query costs
 *     O(ncx + ncy + cells) = O(ng) at the worst, whatever the shape of the grid.
 * obia_ground_dtm_dev : zg = dtm[row, col] by THE PIXEL RULE of obia_points.h (inv6: HOST, the INVERSE transform), widened; NaN
 *     when the point is outside the (H, W) float32 raster or the pixel is not finite.  z (n) float64; zg (n) float64 or NULL; hag (n)
 *     float32.  n as above.
 */
#ifndef OBIA_GROUND_H
#define OBIA_GROUND_H

#include "obia_hip.h"

#define OBIA_GROUND_MAX_COUNT 8

#ifdef __cplusplus
extern "C" {
#endif

int obia_ground_query_dev(obia_ctx *ctx, const double *gx, const double *gy, const double *gz, const int32_t *gidx, int64_t ng,
                          const int32_t *cell_start, int64_t ncx, int64_t ncy, int64_t cx0, int64_t cy0, double side, const double *x,
                          const double *y, const double *z, int64_t n, int32_t count, double max_distance, double *zg, float *hag,
                          uint8_t *m);
int obia_ground_dtm_dev(obia_ctx *ctx, const double *x, const double *y, const double *z, int64_t n, const double *inv6,
                        const float *dtm, int H, int W, double *zg, float *hag);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_GROUND_H */
