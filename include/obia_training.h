/*
 * obia_training.h -- the training-tile passes of libobia_hip.so (obia_amd/csrc/training.hip): what obia.utils.training.tile_and_process
 * (training.py:16-338) does to a tile beside the stretch and CLAHE of obia_image.h -- Gaussian blur of a uint8 image, the 3 x 3 chamfer
 * distance transform, darkening + hard / feathered blend, and the min-max scaling of its rescale=False branch.  DESIGN.md 3.5o.
 *
 * The conventions are those of obia_hip.h, obia_image.h and obia_sharpness.h (status codes, one context per stream, the output
 * contract).  Every pointer is a DEVICE pointer; every call is asynchronous on the context's stream and none reads anything back.
 * Buffers need only the alignment of their element type: uint8 images start at any byte (a row of 3 W bytes is rarely a multiple of
 * four), int32 / float32 planes at a multiple of 4, the int64 counters at a multiple of 8.  The counters are cleared by the call itself.
 * Integer atomics only (those counters): two runs agree bit for bit.  Inputs and outputs of one call must not overlap.
 *
 * Images are interleaved (H, W, 3) or (H, W) uint8.  cv2.GaussianBlur and cv2.distanceTransform are RESTATED from OpenCV's algorithms;
 * they are not compared with cv2 anywhere.
 *
 * obia_train_blur_u8_dev    : cv2.GaussianBlur(src, (kx, ky), 0) for uint8 as integer arithmetic.  wx (kx int32) and wy (ky int32) are
 *                             the per-axis weights, each summing to 256 (obia_amd.training.gaussian_weights builds them on the host).
 *                             S = sum_y sum_x wy * wx * p over the window, out = (S + 32768) >> 16; the horizontal pass is exact in 16
 *                             bits, the total below 2^24.  Border: BORDER_REFLECT_101 applied repeatedly (period 2 (n - 1); a side of 1
 *                             reads index 0), so a side shorter than k / 2 is legal.  kx, ky odd in 1 .. OBIA_TRAIN_MAX_KSIZE, nch 1
 *                             or 3; anything else OBIA_E_INVALID.
 * obia_train_distance_dev   : cv2.distanceTransform(src, DIST_L2, 3) restated: the fixed-point chamfer distance to the nearest zero
 *                             pixel.  HV = 62587, DG = 89738 (0.955 and 1.3693 in 16.16), DIST_MAX = (2^31 - 1) >> 2.  t = min over the
 *                             zero pixels at offset (dx, dy) with |dx| <= R and |dy| <= R of HV * (max - min) + DG * min, max / min of
 *                             |dx|, |dy|; dist = (float)t * 2^-16; a pixel with no zero pixel in that window gets DIST_MAX (8192.0f).
 *                             R >= max(H, W) - 1 is the full transform; 0 <= R.  Pass 1 writes into `work` (H * W int32) the distance
 *                             along the row to the row's nearest zero pixel, capped at R + 1; pass 2 takes the minimum over the rows.
 *                             H, W <= OBIA_TRAIN_MAX_SIDE (OBIA_E_UNSUPPORTED beyond it): no finite distance reaches DIST_MAX.
 * obia_train_compose_u8_dev : three channels.  bg = darken_lut[blurred] (256 bytes).  dist == NULL: out = mask ? tile : bg.  Else, in
 *                             float32 and uncontracted: alpha = clip(1.0f - dist / (float)feather, 0, 1), o = (alpha * tile) +
 *                             ((1.0f - alpha) * bg), clipped to 0 .. 255 and truncated (feather > 0 then, OBIA_E_INVALID otherwise).
 *                             bad_mask_out (int64, not NULL): the mask bytes other than 0 and 1.
 * obia_train_minmax_u8_dev  : mn, mx over all n float32 values; all zeros when they are equal, else clip((255.0f * (x - mn)) /
 *                             (mx - mn), 0, 255) in float32, truncated.  Two kernels: the first leaves partial minima and maxima in
 *                             `work` (OBIA_TRAIN_MINMAX_WORK floats), the second reduces them and scales.  nonfinite_out (int64, not
 *                             NULL): the NaN / +-inf among the values (out is then without meaning).
 */
#ifndef OBIA_TRAINING_H
#define OBIA_TRAINING_H

#include "obia_hip.h"

#define OBIA_TRAIN_MAX_KSIZE 31
#define OBIA_TRAIN_MAX_SIDE 4096
#define OBIA_TRAIN_MINMAX_WORK 512

#ifdef __cplusplus
extern "C" {
#endif

int obia_train_blur_u8_dev(obia_ctx *ctx, const uint8_t *src, int H, int W, int nch, int kx, int ky, const int32_t *wx, const int32_t *wy,
                           uint8_t *out);
int obia_train_distance_dev(obia_ctx *ctx, const uint8_t *src, int H, int W, int R, int32_t *work, float *dist_out);
int obia_train_compose_u8_dev(obia_ctx *ctx, const uint8_t *tile, const uint8_t *blurred, const uint8_t *mask, const float *dist, int H,
                              int W, const uint8_t *darken_lut, double feather, uint8_t *out, int64_t *bad_mask_out);
int obia_train_minmax_u8_dev(obia_ctx *ctx, const float *x, int64_t n, float *work, uint8_t *out, int64_t *nonfinite_out);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_TRAINING_H */
