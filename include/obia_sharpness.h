/*
 * obia_sharpness.h -- the sharpness raster of libobia_hip.so (obia_amd/csrc/sharpness.hip): the passes behind
 * obia.utils.image.rgb_to_gray / variance_of_laplacian / laplacian (image.py:97-136).  DESIGN.md 3.5n.
 *
 * The conventions are those of obia_hip.h and obia_image.h (status codes, one context per stream, the output contract).  Every pointer
 * is a DEVICE pointer except `bands3` (HOST, three ints); every call is asynchronous on the context's stream and none reads anything
 * back.  The float planes only have to be 4-byte aligned: every load and store is one float wide, so a plane that starts 1 or 3 floats
 * off a 16-byte boundary is as good as any.  `nonfinite_out` (int64, 8-byte aligned, may be NULL) is cleared by the call itself.
 * Integer atomics only (that counter): two runs agree bit for bit.  Input and output planes of one call must not overlap.
 *
 * All arithmetic is float32 unless it says double; nothing is contracted into a fused multiply-add.
 *
 * Limits: 1 <= H * W < 2^32 - 1 (the percentile select's limit; OBIA_E_UNSUPPORTED beyond it), 1 <= win <= OBIA_SHARP_MAX_WIN
 * (OBIA_E_UNSUPPORTED beyond it: the first window of a line is summed sample by sample by one lane).
 *
 * obia_sharp_gray_lap_dev    : (H, W, C) float32 raster, three band indices -> lap_out (H, W).  Per band mn = min,
 *                              rng = (max - mn) + 1e-8f, v = (x - mn) / rng; gray = (v0 * 0.299f + v1 * 0.587f) + v2 * 0.114f;
 *                              lap = the Laplacian below of gray.  nonfinite_out: the NaN / +-inf among the H * W * 3 values read
 *                              (lap_out is then without meaning).  Workspace: none beside the context's arena (48 KiB).
 * obia_sharp_laplacian_dev   : cv2.Laplacian(gray, CV_32F, ksize=3) restated: ((((2a + 2b) + (-8c)) + 2d) + 2e) with a, b the upper-left
 *                              and upper-right neighbours, c the centre, d, e the lower-left and lower-right; BORDER_REFLECT_101
 *                              (index -1 reads 1, index n reads n - 2, a line of one reads 0).  nonfinite_out: those of `gray`.
 * obia_sharp_box_dev         : scipy.ndimage.uniform_filter(plane, size=win) of a float32 plane, bit for bit: axis 0 into `work`
 *                              (H * W floats), axis 1 from there into `out`.  Per line of n samples x under `reflect` extension (the edge
 *                              sample duplicated; period 2 n, so any win is legal), s1 = win / 2, s2 = win - s1 - 1, in double:
 *                              tmp = sum of x(-s1 .. s2) in ascending order, out[0] = (float)(tmp / win), then for ll = 1 .. n - 1
 *                              tmp += (x(ll + s2) - x(ll - s1 - 1)), out[ll] = (float)(tmp / win); one lane walks one line, tmp is never
 *                              re-seeded.  win = 1 copies (SciPy skips an axis of size 1).  nonfinite_out: those of `plane`.
 *                              Workspace: ONE plane of H * W floats.
 * obia_sharp_variance_dev    : mean = box(lap), mean2 = box((float)(lap * lap)), out = mean2 - (float)(mean * mean); both recurrences in
 *                              one walk, lap * lap is never stored.  Workspace: TWO planes of H * W floats (`work`, contiguous).
 * obia_sharp_stretch_f32_dev : out[i] = (float) clip(((double)x[i] - lo) / (hi - lo), 0, 1); IEEE division, a NaN passes the clip:
 *                              hi == lo gives NaN where x == lo, 0 below, 1 above.
 *
 * obia.utils.image.laplacian end to end therefore needs at most THREE H * W float32 planes beside its output: lap and the two work
 * planes of the variance.
 */
#ifndef OBIA_SHARPNESS_H
#define OBIA_SHARPNESS_H

#include "obia_hip.h"

#define OBIA_SHARP_MAX_WIN 65536

#ifdef __cplusplus
extern "C" {
#endif

int obia_sharp_gray_lap_dev(obia_ctx *ctx, const float *raster, int H, int W, int C, const int32_t *bands3, float *lap_out,
                            int64_t *nonfinite_out);
int obia_sharp_laplacian_dev(obia_ctx *ctx, const float *gray, int H, int W, float *lap_out, int64_t *nonfinite_out);
int obia_sharp_box_dev(obia_ctx *ctx, const float *plane, int H, int W, int win, float *work, float *out, int64_t *nonfinite_out);
int obia_sharp_variance_dev(obia_ctx *ctx, const float *lap, int H, int W, int win, float *work, float *out);
int obia_sharp_stretch_f32_dev(obia_ctx *ctx, const float *plane, int64_t n, double lo, double hi, float *out);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_SHARPNESS_H */
