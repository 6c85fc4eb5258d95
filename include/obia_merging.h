/*
 * obia_merging.h -- region merging on the segment graph alone (obia_amd/csrc/merging.hip): the fusion cost of every edge, the merge
 * of the node tables of disjoint pairs, and the contraction of the CSR under a `root` column.  After the first pass over the raster
 * (graph, shapes, zonal statistics) a merge round needs nothing but these tables: every quantity of a union follows from its two
 * members' rows and the border they share.  The reference has no counterpart.  The definitions are this project's, modelled on the
 * fusion criterion of Baatz and Schaepe (2000), "multiresolution segmentation", and are compared with eCognition or any other
 * implementation nowhere.  DESIGN.md 3.5x.
 *
 * The conventions are those of obia_adjacency.h (status codes, one context per stream, a null context refused with "null context").
 * Every pointer is a DEVICE pointer.  Buffers need only the alignment of their element type.  Inputs and outputs of one call must
 * not overlap.  Every buffer is the caller's: no call takes memory from the context's workspace, allocates, or stages on the host.
 * Every call returns with its work done; a call that is refused writes nothing.  Only integer atomics are used and no floating-point
 * atomic anywhere, so every result is the same bits for every schedule of the workgroups.
 *
 * THE GRAPH is the CSR of obia_adjacency.h over rows 0 .. N-1 (`N = n_labels`): `indptr` (N+1) int64, `neighbor` (nnz) int32 ascending
 * inside a row with the pseudo-neighbours N (background) and N+1 (outside the raster) last, `border` (nnz) int64.  It is read
 * defensively, as there: a row is the entries max(indptr[i], 0) .. min(indptr[i+1], nnz) - 1, an entry whose neighbour is outside
 * 0 .. N-1 is a pseudo entry.  Tables that are not what they should be give numbers without meaning, never an access out of bounds.
 *
 * THE NODE TABLES.  `area` (N) int64, pixels; `mean` and `m2` (N, F) float64, the per-band mean and `variance * area`; `perimeter`
 * (N) int64, pixel edges; `box` (N, 4) int32, (r0, c0, r1, c1), half-open.  An EMPTY row is zeros in the integer tables and the quiet
 * NaN in `mean` and `m2`.
 *
 * FUSION COST of a real entry i -> j.  All arithmetic is float64, every operation separate, nothing contracted, the square roots
 * correctly rounded.  With a = min(i, j), b = max(i, j) -- so cost[i->j] and cost[j->i] are the same bits -- and `w` = band_weights:
 *     fa = (double)area[a]; fb = (double)area[b]; fm = fa + fb
 *     colour = 0.0; for f ascending:
 *         d  = mean[b,f] - mean[a,f]
 *         mm = (m2[a,f] + m2[b,f]) + (d*d) * ((fa*fb)/fm)
 *         h  = fm*sqrt(mm/fm) - (fa*sqrt(m2[a,f]/fa) + fb*sqrt(m2[b,f]/fb))
 *         colour = colour + w[f]*h
 *     la = (double)perimeter[a]; lb = (double)perimeter[b]; lm = (double)(perimeter[a] + perimeter[b] - 2*border)   (the integer first)
 *     ba, bb, bm = 2.0*(double)(height + width) of box a, of box b, of the union box (the integer sum first)
 *     hc = fm*(lm/sqrt(fm)) - (fa*(la/sqrt(fa)) + fb*(lb/sqrt(fb)))
 *     hs = fm*(lm/bm) - (fa*(la/ba) + fb*(lb/bb))
 *     cost = w_color*colour + (1.0 - w_color)*(w_compact*hc + (1.0 - w_compact)*hs)
 * `border` is the entry's own.  A pseudo entry gets the quiet NaN.  Whatever NaN arises is written as 0x7ff8000000000000.
 *
 * MERGE OF PAIRS.  `partner` is (N) int32.  Row i has the partner p = partner[i] when 0 <= p < N, p != i and partner[p] == i;
 * everything else (-1, an index outside 0 .. N-1, a partner that does not point back) counts as no partner, and the row is copied.
 * For a pair a < b, row a of the outputs becomes the union and row b becomes empty:
 *     fm, d, mm as above; mean[a,f] = mean[a,f] + d*(fb/fm); m2[a,f] = mm; area[a] = area[a] + area[b]
 *     perimeter[a] = perimeter[a] + perimeter[b] - 2*border(a, b), the border looked up in row a, 0 when b is not in the row
 *     box[a] = (min r0, min c0, max r1, max c1)
 * Every element of the five output tables is written.
 *
 * CONTRACTION.  `root` is (N) int32 with root[root[i]] == root[i]: the row every row goes to.  The new row r is built from the
 * entries of every row i with root[i] == r: a real neighbour j is mapped to root[j], a pseudo neighbour (outside 0 .. N-1) is kept as
 * N (j == N) or N+1 (every other), entries that would point from r to r are dropped, equal neighbours are combined and their
 * borders add, and the row is sorted ascending with the pseudo entries last.  Every other row is empty.  A row i whose root[i] is
 * outside 0 .. N-1 is left out, and so is an entry whose neighbour's root is.  NO ROW IS EVER DROPPED OR TRUNCATED, whatever its
 * length.  It runs as three calls with torch's prefix sums between them:
 *   - obia_merge_contract_rows_dev: raw_count_out (N) int64, the entries of all rows that go to r (before anything is combined).
 *     Writes every element.  The caller forms raw_ptr (N+1) int64, its exclusive prefix sum with the total last.
 *   - obia_merge_contract_count_dev: gathers the mapped entries of row r into key_work / border_work at raw_ptr[r] .. raw_ptr[r+1]-1,
 *     sorts and combines them there, and writes count_out (N) int32, the length of the new row r.  Writes every element of
 *     count_out.  key_work (nnz) int32, border_work (nnz) int64 and cursor_work (N) int32 are scratch, the caller's like everything
 *     else; what the first two hold afterwards is for the write pass only.  Rows of up to 8 and up to 32 gathered entries are sorted
 *     by groups of 8 and of 32 lanes in registers, longer ones by a workgroup: up to OBIA_MERGE_ROW_CAP entries in LDS, above that in
 *     place in the scratch, by the same network with the same result.
 *   - obia_merge_contract_write_dev: indptr_out (N+1) int64 is an INPUT, the exclusive prefix sum of count with the total, nnz_out,
 *     last.  neighbor_out (nnz_out) int32 and border_out (nnz_out) int64 get row r at indptr_out[r] .. indptr_out[r] + count[r] - 1.
 *     With indptr_out that of the count, every element is written.
 *
 * REFUSALS.  OBIA_E_UNSUPPORTED: nnz >= 2^31, nnz_out >= 2^31, N * F >= 2^31.  OBIA_E_INVALID: a null context, n_labels < 0 or
 * > 2^31 - 3, F < 1, nnz < 0, nnz_out < 0, a null, misaligned or overlapping buffer.  A buffer of no elements may be null.
 */
#ifndef OBIA_MERGING_H
#define OBIA_MERGING_H

#include "obia_hip.h"

#define OBIA_MERGE_ROW_CAP 2048   /* gathered entries of a row one workgroup sorts in LDS; a longer row is sorted in the scratch */

#ifdef __cplusplus
extern "C" {
#endif

int obia_merge_cost_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t n_labels, int64_t nnz,
                        const int64_t *area, const double *mean, const double *m2, int F, const double *band_weights,
                        const int64_t *perimeter, const int32_t *box, double w_color, double w_compact, double *cost_out);
int obia_merge_pairs_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t n_labels, int64_t nnz,
                         const int32_t *partner, const int64_t *area, const double *mean, const double *m2, int F, const int64_t *perimeter,
                         const int32_t *box, int64_t *area_out, double *mean_out, double *m2_out, int64_t *perimeter_out, int32_t *box_out);
int obia_merge_contract_rows_dev(obia_ctx *ctx, const int64_t *indptr, int32_t n_labels, int64_t nnz, const int32_t *root,
                                 int64_t *raw_count_out);
int obia_merge_contract_count_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t n_labels,
                                  int64_t nnz, const int32_t *root, const int64_t *raw_ptr, int32_t *key_work, int64_t *border_work,
                                  int32_t *cursor_work, int32_t *count_out);
int obia_merge_contract_write_dev(obia_ctx *ctx, int32_t n_labels, int64_t nnz, const int64_t *raw_ptr, const int32_t *count,
                                  const int32_t *key_work, const int64_t *border_work, const int64_t *indptr_out, int64_t nnz_out,
                                  int32_t *neighbor_out, int64_t *border_out);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_MERGING_H */
