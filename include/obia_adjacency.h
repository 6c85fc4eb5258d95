/*
 * obia_adjacency.h -- which segments of a label raster touch each other (obia_amd/csrc/adjacency.hip): the shared pixel edges of
 * every pair of 4-adjacent segments, counted tile by tile into hash tables in LDS, and what a table of about 3 N entries then
 * answers: a distance per edge, statistics of a segment's neighbours, its border to every class, its best neighbour, the connected
 * components of a link rule, and the relabelling that merges them.  The reference has no counterpart.  DESIGN.md 3.5v.
 *
 * The conventions are those of obia_boxes.h (status codes, one context per stream, a null context refused with "null context").
 * Every pointer is a DEVICE pointer unless it says HOST.  Buffers need only the alignment of their element type.  Inputs and outputs
 * of one call must not overlap.  Every buffer is the caller's: no call takes memory from the context's workspace, allocates, or
 * stages on the host.  Every call returns with its work done; a call that is refused writes nothing.  Only integer atomics are used
 * and no floating-point atomic anywhere, so every result is the same bits for every schedule of the workgroups.
 *
 * SEGMENTS
 *   - `labels` is (H, W) int32.
 *   - Label `l` is segment `i = l - start_label` when `0 <= i < N` (`N = n_labels`, as in `zonal_stats`).
 *   - Every other value is BACKGROUND.
 *   - 4-connectivity only.
 *
 * PIXEL EDGES
 *   - Pixel (r, c) OWNS its right edge to (r, c+1) and its lower edge to (r+1, c).
 *   - On the frame it also owns the frame edge itself: left for c = 0, top for r = 0, right for c = W-1, bottom for r = H-1.
 *   - An edge with a segment pixel of `i` on one side and something else on the other is a border edge of `i`.  The other side is
 *     one of:
 *       - segment `j != i`;
 *       - background, written as pseudo-neighbour `N`;
 *       - outside the raster, written as pseudo-neighbour `N + 1`.
 *   - Edges between two pixels of one segment count nothing.  Edges between two non-segments count nothing.
 *
 * TILES
 *   - The raster is cut into tiles of `OBIA_ADJ_TILE_H x OBIA_ADJ_TILE_W` pixels, numbered row-major.
 *   - An edge belongs to the tile of the pixel that owns it.  The kernel therefore reads one halo column and one halo row.
 *   - The LDS table of a workgroup has room for every edge a tile can own, so THERE IS NO OVERFLOW PATH AND NO PASS COUNT.
 *     (A pixel owns at most three distinct undirected pairs: its right edge, its lower edge, and -- whichever frame edges it owns --
 *     the one pair (segment, outside).  A tile therefore holds at most 3 * OBIA_ADJ_TILE_H * OBIA_ADJ_TILE_W = 1536 pairs, in a table
 *     of OBIA_ADJ_TABLE = 2048 slots.)
 *
 * THE GRAPH
 *   - The graph is a symmetric CSR over rows 0 .. N-1.
 *       - `indptr` is (N+1) int64.
 *       - `neighbor` is (nnz) int32, ASCENDING INSIDE A ROW.  The real neighbours `j < N` come first, then `N` if present, then
 *         `N+1` if present.
 *       - `border` is (nnz) int64, the number of shared pixel edges.
 *   - It follows that `border[i->j] == border[j->i]`.
 *   - The perimeter of `i` in pixel edges is the sum of its row.
 *   - A label that occurs in several places is one row; its counts add.
 *   - Nothing is floating point up to here.
 *
 * PER-EDGE DISTANCE
 *   - `d2[i->j] = sum_f (v_if - v_jf)^2` over `values` (N, F) float64, in float64.
 *   - It is added from 0.0 in ascending `f`: `d = a - b; t = d*d; acc = acc + t`, nothing contracted.
 *   - NaN propagates.
 *   - It is defined for real neighbours only; pseudo entries get NaN.
 *   - It is squared on purpose: no `sqrt` on the device, so the restatement can hold it to the bit.  Python squares the user's
 *     threshold.
 *
 * NEIGHBOUR STATISTICS
 *   For every (i, f), walk the real neighbours `j` of row `i` IN CSR ORDER.  Skip those whose `v_jf` is NaN.
 *   - `w = (double)border`.
 *   - `sw = sw + w`.
 *   - `s = s + w*v_jf`.
 *   - `mn` and `mx` are the running minimum and maximum of `v_jf`.
 *   - `used` is the number of neighbours not skipped.
 *   - `nb_mean = s / sw`.
 *   - With `used == 0`, mean, min and max are the quiet NaN.
 *   The order is part of the definition, so one lane owns one (i, f).  The table is about 3 N long, so this is not a hot path.
 *
 * BORDER TO CLASS
 *   - `out[i, k]` is the sum of `border` over real neighbours `j` with `classes[j] == k`, int64.
 *   - Classes outside 0 .. K-1 add nothing.
 *   - Every element is written.
 *
 * BEST NEIGHBOUR
 *   - `best[i]` is the real neighbour of the smallest `d2` that is not NaN.  Ties go to the first in CSR order, which is the lowest
 *     index.  It is -1 when there is none.
 *   - `best_d2[i]` is that value, or NaN.
 *
 * COMPONENTS
 *   - Each directed entry carries one byte, `link`.
 *   - `i` and `j` are linked when the byte of `i->j` OR of `j->i` is non-zero.  Pseudo entries are never linked.
 *   - `root[i]` is the smallest index of `i`'s component.  This is the invariant of the union-find in `seeds.hip`, "roots are the
 *     smallest members".
 *
 * Every NaN that is written is the quiet NaN 0x7ff8000000000000, whatever NaN went in or arose.  -0 is a number like any other:
 * the running minimum and maximum replace the held value only on a strict comparison, so of two zeros the first in CSR order stays.
 *
 * A CSR THE CALLER PASSES is read defensively: a row is the entries max(indptr[i], 0) .. min(indptr[i+1], nnz) - 1, and an entry
 * whose neighbour is outside 0 .. N-1 is a pseudo entry.  A CSR that is not one gives numbers without meaning, never an access out
 * of bounds.
 *
 * REFUSALS.  OBIA_E_UNSUPPORTED: H * W >= 2^31, npx >= 2^31, nnz >= 2^31, total >= 2^31, N * F or N * K >= 2^31.  OBIA_E_INVALID: a
 * null context, n_labels < 0 or > 2^31 - 3 (N + 1 is a neighbour), H or W < 1, F < 1, K < 1, nnz < 0, a null, misaligned or
 * overlapping buffer.  A buffer of no elements (N == 0, nnz == 0, total == 0) may be null.
 *
 * obia_adj_tile_count_dev : count_out (n_tiles) int32, n_tiles = ceil(H / OBIA_ADJ_TILE_H) * ceil(W / OBIA_ADJ_TILE_W): the
 *     distinct directed (segment, other) records of every tile.  Writes every element.
 * obia_adj_tile_write_dev : offset (n_tiles) int64, the exclusive prefix sum of the counts, and total, their sum.  key_out (total)
 *     int64 and edges_out (total) int32: the records of tile t go to rows offset[t] .. offset[t] + count[t] - 1, in no particular
 *     order inside a tile.  A record is directed: key = src * (N + 2) + dst, edges = the shared pixel edges the tile owns.  A real
 *     pair is written in both directions, a pseudo pair only from the segment.  `work` is OBIA_ADJ_WORK int32 of scratch, the
 *     caller's like everything else; what it holds afterwards is not specified.  offset[0] != 0, offset[t] + count[t] !=
 *     offset[t + 1], or the last != total: OBIA_E_INVALID ("offset and total are not those of the count").  That refusal comes after
 *     the pass: rows INSIDE key_out and edges_out may have been written by then, nothing outside them.
 * obia_adj_edge_d2_dev : values (N, F) float64 -> d2_out (nnz) float64.  Writes every element.
 * obia_adj_neighbor_stats_dev : values (N, F) float64 -> mean_out, min_out, max_out (N, F) float64 and used_out (N, F) int32.
 * obia_adj_class_border_dev : classes (N) int32 -> out (N, K) int64.
 * obia_adj_best_neighbor_dev : d2 (nnz) float64 -> best_out (N) int32, best_d2_out (N) float64.
 * obia_adj_components_dev : link (nnz) uint8 -> root_out (N) int32.
 * obia_adj_relabel_dev : out = map[l - start_label] for a segment, map (N) int32; a background value below start_label is kept; a
 *     value >= start_label + N becomes start_label - 1.  labels, out (npx) int32, npx >= 1.  (obia_boxes_dissolve_dev is another
 *     rule: ids from 1, a table with a row 0, assigned + 1, every background 0.)
 */
#ifndef OBIA_ADJACENCY_H
#define OBIA_ADJACENCY_H

#include "obia_hip.h"

#define OBIA_ADJ_TILE_H 16      /* rows of a tile */
#define OBIA_ADJ_TILE_W 32      /* columns of a tile */
#define OBIA_ADJ_TABLE 2048     /* slots of the LDS table of one workgroup: a power of two above 3 * TILE_H * TILE_W */
#define OBIA_ADJ_WORK 4         /* int32 of scratch obia_adj_tile_write_dev asks for */

#ifdef __cplusplus
extern "C" {
#endif

int obia_adj_tile_count_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, int32_t start_label, int32_t n_labels, int32_t *count_out);
int obia_adj_tile_write_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, int32_t start_label, int32_t n_labels, const int64_t *offset,
                            int64_t total, int64_t *key_out, int32_t *edges_out, int32_t *work);
int obia_adj_edge_d2_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, int32_t n_labels, int64_t nnz, const double *values,
                         int F, double *d2_out);
int obia_adj_neighbor_stats_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t n_labels,
                                int64_t nnz, const double *values, int F, double *mean_out, double *min_out, double *max_out,
                                int32_t *used_out);
int obia_adj_class_border_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t n_labels,
                              int64_t nnz, const int32_t *classes, int K, int64_t *out);
int obia_adj_best_neighbor_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, int32_t n_labels, int64_t nnz,
                               const double *d2, int32_t *best_out, double *best_d2_out);
int obia_adj_components_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, int32_t n_labels, int64_t nnz,
                            const uint8_t *link, int32_t *root_out);
int obia_adj_relabel_dev(obia_ctx *ctx, const int32_t *labels, int64_t npx, int32_t start_label, int32_t n_labels, const int32_t *map,
                         int32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_ADJACENCY_H */
