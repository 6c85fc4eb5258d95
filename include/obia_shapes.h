/*
 * obia_shapes.h -- how large, how elongated and which way round every segment of a label raster is (obia_amd/csrc/shapes.hip): one
 * pass over the raster gives, per segment, the area, the first and second raw moments of its pixel indices, its perimeter in pixel
 * edges and its bounding box, all as integers.  Everything an object-based feature table derives from them (centroid, central
 * moments, axis lengths, eccentricity, orientation, extent, compactness, ...) is a table of N rows and is left to the caller
 * (obia_amd/shapes.py).  The reference has no counterpart.  DESIGN.md 3.5w.
 *
 * The conventions are those of obia_adjacency.h (status codes, one context per stream, a null context refused with "null context").
 * Every pointer is a DEVICE pointer.  Buffers need only the alignment of their element type.  Inputs and outputs of one call must
 * not overlap.  Every buffer is the caller's: the call takes no memory from the context's workspace, allocates nothing, and stages
 * nothing on the host.  The call returns with its work done and with every element of both outputs written; a call that is refused
 * writes nothing.  Only integer atomics are used and no floating-point value exists anywhere, so every result is the same bits for
 * every schedule of the workgroups.
 *
 * SEGMENTS (obia_adjacency.h, word for word)
 *   - `labels` is (H, W) int32.
 *   - Label `l` is segment `i = l - start_label` when `0 <= i < N` (`N = n_labels`, as in `zonal_stats`).
 *   - Every other value is BACKGROUND.
 *   - A label that occurs in several places is one row; its sums add and its box is the box of all its pixels.
 *
 * THE SUMS: sums_out is (N, OBIA_SHAPE_SUMS) int64.  With r, c the row and column index of a pixel of the segment:
 *     column 0  n        the area in pixels
 *     column 1  sum r
 *     column 2  sum c
 *     column 3  sum r^2
 *     column 4  sum c^2
 *     column 5  sum r c
 *     column 6  the perimeter in pixel edges: the edges of the segment's pixels whose other side is another segment, background or
 *               outside the raster.  It is the row sum of the adjacency graph's `border` (obia_adjacency.h, PIXEL EDGES), bit for bit.
 *
 * THE BOX: box_out is (N, 4) int32, (r0, c0, r1, c1), half-open: rows r0 .. r1 - 1 and columns c0 .. c1 - 1 hold the segment.
 *
 * A row without pixels is all zeros in both tables.
 *
 * NO SUM OVERFLOWS.  With M = max(H, W), every pixel index is at most M - 1, so every term r, c, r^2, c^2 or r c of a pixel is at
 * most (M - 1)^2 < M^2, and a segment has at most H W pixels: every sum of every labelling is below M^2 H W.  The call is refused
 * when M^2 H W >= 2^63 and served otherwise, so a served call cannot overflow an int64, whatever the labels.  (Every partial sum a
 * tile adds is a sum of non-negative terms of the final sum, so nothing wraps on the way either.)  A raster of 1 x 2^21 pixels is the
 * smallest that is refused for this reason (a 1 x (2^21 - 1) one is served); for a raster with max(H, W) < 2^16 the limit H * W < 2^31
 * comes first, so the rule bears on long thin rasters only.
 *
 * TILES.  The raster is cut into the tiles of obia_adjacency.h (OBIA_ADJ_TILE_H x OBIA_ADJ_TILE_W).  A workgroup reduces every run
 * of equal labels of a tile row in closed form, adds the runs into a table in LDS keyed by segment (OBIA_SHAPE_TABLE slots; a tile
 * holds at most OBIA_ADJ_TILE_H * OBIA_ADJ_TILE_W = 512 segments, so THERE IS NO OVERFLOW PATH), and flushes every occupied slot
 * once, moved to raster coordinates, with 64-bit integer atomic adds and 32-bit integer atomic maxima.
 *
 * REFUSALS.  OBIA_E_UNSUPPORTED: H * W >= 2^31; max(H, W)^2 * H * W >= 2^63.  OBIA_E_INVALID: a null context, n_labels < 0 or
 * > 2^31 - 3, H or W < 1, a null, misaligned or overlapping buffer.  A buffer of no elements (N == 0) may be null.
 */
#ifndef OBIA_SHAPES_H
#define OBIA_SHAPES_H

#include "obia_hip.h"

#define OBIA_SHAPE_SUMS 7        /* columns of sums_out */
#define OBIA_SHAPE_TABLE 1024    /* slots of the LDS table of one workgroup: a power of two above OBIA_ADJ_TILE_H * OBIA_ADJ_TILE_W */

#ifdef __cplusplus
extern "C" {
#endif

int obia_shape_sums_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, int32_t start_label, int32_t n_labels, int64_t *sums_out,
                        int32_t *box_out);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_SHAPES_H */
