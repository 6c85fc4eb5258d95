/*
 * obia_boxes.h -- segments and detection boxes (obia_amd/csrc/boxes.hip): the area every segment of a label raster shares with every
 * axis-aligned box, the box that wins each segment, the dissolve of a label raster by that assignment, the IoU of two box tables and
 * the greedy non-maximum suppression of one.  notebooks/deepfor2.ipynb (assign_fid), obia/detection/utils.py:63-81 and
 * obia/utils/utils.py:70-145 of the reference; DESIGN.md 3.5r.
 *
 * The conventions are those of obia_hip.h (status codes, one context per stream, the output contract).  Every pointer is a DEVICE
 * pointer unless it says HOST.  Buffers need only the alignment of their element type.  Inputs and outputs of one call must not
 * overlap.  Every call returns with its work done.  n is the number of boxes, 1 .. 2^31 - 1 (OBIA_E_INVALID otherwise).
 *
 * BOXES.  boxes (n, 4) float64, rows (x0, y0, x1, y1) in pixel-corner coordinates: pixel (r, c) is the closed square
 * [c, c + 1] x [r, r + 1].  Every value finite, x0 <= x1, y0 <= y1: OBIA_E_NONFINITE / OBIA_E_INVALID otherwise, nothing written.
 *
 * THE OVERLAP RULE.  labels (H, W) int32; ids outside 1 .. n_labels are background.  The footprint of a box is the columns
 * max(0, ceil(x0) - 1) .. min(W - 1, floor(x1)) and the rows likewise: the pixels whose closed square meets the closed box.  A
 * footprint of 2^31 pixels or more: OBIA_E_UNSUPPORTED.  A footprint column c is of class
 *     Z, weight 0                          when c + 1 == x0 or c == x1,
 *     L, weight fl(min(x1, c + 1) - x0)    when c < x0,
 *     R, weight fl(x1 - c)                 when c + 1 > x1 and it is not L,
 *     I, weight exactly 1.0                otherwise,
 * and a row of class Z / T / B / I by the same rule on y.  For a (segment, box) pair n_ab counts the segment's footprint pixels of
 * column class a and row class b, meets all of them (Z included), and in float64, nothing contracted,
 *     area = sum over b in (T, I, B), inside it over a in (L, I, R), of fl(fl(wx_a * wy_b) * (double)n_ab),
 * added left to right from 0.0 (a class without pixels adds nothing).  A pair exists when meets > 0; its area may be 0.
 *
 * OBIA_BOXES_TABLE: one workgroup walks one box and counts into a hash table of that many labels in LDS.  A footprint with more
 * distinct labels is redone in P passes, pass p counting the labels with label mod P == p, P doubling until every pass fits.  The
 * results do not depend on P, on the schedule or on the run: they are integer counts and integer atomics on bit patterns.  A box with
 * P passes reads its footprint P times; ids that share a factor 2^k are not parted until P exceeds 2^k, so renumber sparse ids first.
 *
 * obia_boxes_assign_dev      : assigned_out (n_labels + 1) int32: the box of the largest area of every segment, ties to the lowest box
 *     index, -1 when no pair exists; area_out (n_labels + 1) float64: that area, 0.0 when there is none.  Element 0 is -1 / 0.0.
 * obia_boxes_pair_count_dev  : count_out (n) int64: the pairs of every box; passes_out (n) int32: the P its footprint needed.
 * obia_boxes_pair_write_dev  : offset (n) int64: the exclusive prefix sum of the counts, total their sum (>= 1), passes (n) int32 as
 *     the count returned them; the pairs of box b are written to rows offset[b] .. offset[b] + count[b] - 1 of box_out, segment_out,
 *     meets_out (total) int32 and area_out (total) float64, in no particular order inside a box.  Tables that are not those of the
 *     count: OBIA_E_INVALID, no access out of bounds, the outputs unspecified.
 * obia_boxes_dissolve_dev    : out (npx) int32 = assigned[label] + 1 where the label is in 1 .. n_labels and assigned, else 0;
 *     assigned (n_labels + 1) int32, values < 0 mean none.  npx >= 1.
 * obia_boxes_iou_dev         : a (na, 4), b (nb, 4) float64 boxes (x0, y0, x1, y1), not checked; out (na, nb) float64, in this order
 *         iw = max(0, min(ax1, bx1) - max(ax0, bx0)), ih likewise, inter = iw * ih,
 *         iou = inter / (((areaA + areaB) - inter) + 1e-6),       area = (x1 - x0) * (y1 - y0).
 *     na, nb >= 1, na * nb < 2^62.
 * obia_boxes_nms_dev         : boxes (n, 4) as above, pos (n) int32 the rank of every box in the order of suppression (a permutation
 *     of 0 .. n - 1), group (n) int32 or NULL, key (n) int64 -- the cell keys of (x0, y0) on the uniform grid of obia_seed_table.h, cell
 *     side >= the largest box side -- all in cell order.  keep_out (n) bytes 0 / 1, cell order:
 *         kept(i) = no j with pos_j < pos_i, kept(j), group_j == group_i and iou(j, i) > iou_threshold.
 *     iou_threshold >= 0 (so that only boxes that overlap suppress each other).  Decided in rounds as obia_seedtab_stage1_dev is: a
 *     round decides every box whose earlier overlapping boxes are all decided; OBIA_E_INTERNAL when n rounds did not suffice.
 *     rounds_out (HOST int32, may be NULL).
 */
#ifndef OBIA_BOXES_H
#define OBIA_BOXES_H

#include "obia_seed_table.h"

#define OBIA_BOXES_TABLE 256

#ifdef __cplusplus
extern "C" {
#endif

int obia_boxes_assign_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, const double *boxes, int64_t n, int32_t n_labels,
                          int32_t *assigned_out, double *area_out);
int obia_boxes_pair_count_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, const double *boxes, int64_t n, int32_t n_labels,
                              int64_t *count_out, int32_t *passes_out);
int obia_boxes_pair_write_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, const double *boxes, int64_t n, int32_t n_labels,
                              const int64_t *offset, const int32_t *passes, int64_t total, int32_t *box_out, int32_t *segment_out,
                              double *area_out, int32_t *meets_out);
int obia_boxes_dissolve_dev(obia_ctx *ctx, const int32_t *labels, int64_t npx, const int32_t *assigned, int32_t n_labels, int32_t *out);
int obia_boxes_iou_dev(obia_ctx *ctx, const double *a, int64_t na, const double *b, int64_t nb, double *out);
int obia_boxes_nms_dev(obia_ctx *ctx, const double *boxes, const int32_t *pos, const int32_t *group, const int64_t *key, int64_t n,
                       int64_t ncx, double iou_threshold, uint8_t *keep_out, int32_t *rounds_out);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_BOXES_H */
