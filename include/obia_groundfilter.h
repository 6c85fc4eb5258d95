/*
 * obia_groundfilter.h -- ground points of an unclassified cloud (obia_amd/csrc/groundfilter.hip): the cell minimum of a cloud on a
 * raster, grey erosion / dilation / opening of a float32 plane with a square window, the threshold raster of a progressive
 * morphological filter, and the one test of every point against it.  The definitions are this project's, modelled on Zhang et al.
 * 2003 and PDAL's filters.pmf; they are NOT compared with PDAL anywhere.  DESIGN.md 3.5u.
 *
 * The conventions are those of obia_ground.h (status codes, one context per stream, a null context refused).  Every pointer is a
 * DEVICE pointer unless it says HOST.  Buffers need only the alignment of their element type.  Inputs, outputs and scratch planes of
 * one call must not overlap.  Every buffer is the caller's, scratch planes included: no call takes memory from the context's
 * workspace.  Every call returns with its work done; a call that is refused writes nothing.  n >= 2^31 or H * W >= 2^31:
 * OBIA_E_UNSUPPORTED.  No floating-point atomic is used anywhere, so every result is the same bits for every order of the points,
 * every cut of the cloud into calls and every schedule of the workgroups.
 *
 * THE GRID.  An (H, W) raster with the HOST array inv6, the INVERSE transform, and THE PIXEL RULE of obia_points.h, unchanged:
 *     col = floor(inv6[0] x + inv6[1] y + inv6[4]),  row = floor(inv6[2] x + inv6[3] y + inv6[5])     (float64, nothing contracted)
 * a point is inside when 0 <= col < W and 0 <= row < H; a NaN or infinite coordinate is outside.
 *
 * A PLANE is (H, W) float32.  NaN means EMPTY: no point, no value.  +inf and -inf are DATA, not empties: they take part in every
 * minimum and maximum as the numbers they are, and a window that holds nothing else gives +-inf, not NaN.  -0 is read as +0 (every
 * value is loaded as v + 0.0f), so no plane that is written holds a -0 and minimum and maximum never have to order the two zeros.
 * Every NaN that is written is the quiet NaN 0x7fc00000.
 *
 * THE CELL MINIMUM.  zmin[cell] = the minimum of (float)z + 0.0f over the points inside the cell whose z (float64) is finite; EMPTY
 * when there is none.  (A finite z beyond the float32 range becomes +-inf, which is data.)  Rounding commutes with the minimum, so
 * this is the rounded minimum of the z themselves.  The accumulating state is a caller-owned uint32 plane of ORDER KEYS, cleared to 0
 * = empty: key(v) = ~k(v) with k the order-preserving key of a float32 (bits | 0x80000000 when the sign bit is clear, ~bits otherwise),
 * so a LARGER key is a SMALLER value and the update is an integer atomic maximum.  No value has the key 0.
 * obia_gf_cell_min_dev : x, y, z (n) float64; 0 <= n < 2^31, n == 0 does nothing; ADDS the points to `keys` (H, W) uint32: a second
 *     call continues the first.  A point loads the key before the atomic and issues the atomic only when it would lower the value.
 * obia_gf_cell_min_finish_dev : keys (H, W) -> zmin (H, W) float32; writes every element.
 *
 * GREY EROSION (op 0) AND DILATION (op 1) with radius r, 1 <= r <= OBIA_MORPH_MAX_RADIUS (larger: OBIA_E_UNSUPPORTED; r < 1 or
 * another op: OBIA_E_INVALID): the minimum (maximum) over the (2r + 1)^2 window around the cell, clipped to the raster, of the cells
 * that are not EMPTY; EMPTY where the clipped window holds none.  An OPENING is the erosion, then the dilation of the eroded plane:
 * an empty cell with neighbours that are not empty is therefore filled.  On planes without NaN, infinities and -0 this is
 * scipy.ndimage.grey_erosion / grey_dilation / grey_opening(size=(2r + 1, 2r + 1)) at their default mode, bit for bit.
 * obia_morph_filter_dev : src -> dst (H, W) through the scratch plane tmp (H, W): two line passes, along the rows into tmp, then
 *     along the columns into dst.  Writes every element of dst; what tmp holds afterwards is not specified.
 *
 * THE THRESHOLD RASTER of a schedule radii[k], dh[k] (HOST arrays, int32 and float64), k = 0 .. K - 1, 1 <= K <= OBIA_GF_MAX_STEPS,
 * every radius as above, every dh finite and >= 0:
 *     S_0 = zmin,  S_k+1 = opening(S_k, radii[k]),  T = min over k of (S_k+1 + (float)dh[k])
 * one float32 addition per step, EMPTY terms ignored by the minimum: T is EMPTY only where every S_k+1 is.
 * obia_gf_threshold_dev : zmin -> surface = S_K and thresh = T, (H, W) float32 each, through the scratch planes tmp0 and tmp1.  The
 *     loop over the steps runs in the library: 4 K line passes, the addition and the minimum folded into the last pass of each step.
 *     Writes every element of surface and thresh.
 *
 * CLASSIFICATION.  A point is GROUND iff it is inside the raster, its z is finite and z <= (double)thresh[cell]; an EMPTY threshold
 * fails.  obia_gf_classify_dev : x, y, z (n) float64, n as above; flags (n) uint8: 1 ground, 0 not, every element written;
 *     counters (4) uint64, ADDED to (the caller clears them): points outside the raster, inside with a z that is not finite, rejected,
 *     ground.
 */
#ifndef OBIA_GROUNDFILTER_H
#define OBIA_GROUNDFILTER_H

#include "obia_hip.h"

#define OBIA_MORPH_MAX_RADIUS 127
#define OBIA_GF_MAX_STEPS 16
#define OBIA_MORPH_ROW_TILE 1024   /* cells of a row one workgroup filters per trip */
#define OBIA_MORPH_COL_TILE 128    /* cells of a column (of OBIA_MORPH_COL_LANES columns side by side) one workgroup filters per trip */
#define OBIA_MORPH_COL_LANES 32

#ifdef __cplusplus
extern "C" {
#endif

int obia_gf_cell_min_dev(obia_ctx *ctx, const double *x, const double *y, const double *z, int64_t n, const double *inv6, int H, int W,
                         uint32_t *keys);
int obia_gf_cell_min_finish_dev(obia_ctx *ctx, const uint32_t *keys, int H, int W, float *zmin);
int obia_morph_filter_dev(obia_ctx *ctx, const float *src, int H, int W, int radius, int op, float *tmp, float *dst);
int obia_gf_threshold_dev(obia_ctx *ctx, const float *zmin, int H, int W, const int32_t *radii, const double *dh, int K, float *tmp0,
                          float *tmp1, float *surface, float *thresh);
int obia_gf_classify_dev(obia_ctx *ctx, const double *x, const double *y, const double *z, int64_t n, const double *inv6,
                         const float *thresh, int H, int W, uint8_t *flags, uint64_t *counters);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_GROUNDFILTER_H */
