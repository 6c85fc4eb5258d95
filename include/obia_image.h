/*
 * obia_image.h -- the image-preview entry points of libobia_hip.so (obia_amd/csrc/image.hip): the passes behind
 * obia.handlers.geotif.Image.to_image (geotif.py:46-75), obia.utils.image.rescale_to_8bit / apply_histogram_equalization /
 * apply_clahe (image.py:8-94) and obia.segmentation.segment.Segments.to_segmented_image (segment.py:41-53).
 *
 * The conventions are those of obia_hip.h (status codes, one context per stream, the output contract).  Every pointer is a DEVICE
 * pointer, every call is asynchronous on the context's stream and none reads anything back.  A buffer only has to be aligned to its
 * element: the uint8 rasters may start at ANY byte (a row slab, `flat[1:]`); the kernels store whole dwords where the address
 * allows and single bytes at the heads and tails.  Integer atomics only: two runs agree bit for bit.
 *
 * These declarations live beside obia_hip.h, not in it: the binding table of obia_hip.h is pinned by the guarded-output registry of
 * the test suite, this one by tests/test_image_cpu.py and tests/test_gpu_image_buffers.py.  OBIA_ABI_VERSION is unchanged.
 *
 * obia_image_stretch_u8_dev : out[i] = (uint8) clip(255 * (x[i] - lo) / (hi - lo), 0, 255) in float64, multiply before divide,
 *                             truncated; float32 (is_f64 = 0) or float64 plane of n elements; lo == hi writes zeros.
 * obia_image_gray_hist_dev  : uint8 pixels, nch = 3 (RGB interleaved; grey = (9798 R + 19235 G + 3735 B + 16384) >> 15) or nch = 1
 *                             (the plane is the grey plane) -> gray_out [n] (may be NULL) and hist256_out [256] int64, which the
 *                             call clears itself.  1 <= n < 2^31.
 * obia_image_lut_u8_dev     : out[i * rep + r] = lut256[in[i]] for r < rep; rep = 1 or 3 (grey replicated to three channels).
 * obia_image_clahe_u8_dev   : CLAHE (clip limit 2.0, 8 x 8 tiles) of channel `ch` of an interleaved (H, W, nch) uint8 raster into the
 *                             same channel of `out` (same layout, a different buffer); the other channels of `out` are not touched.
 *                             H, W >= 8; a padded tile of more than 46340^2 pixels is refused (OBIA_E_UNSUPPORTED).
 * obia_image_boundaries_dev : skimage.segmentation.find_boundaries(labels, mode="outer", background=0, connectivity=1) as 0 / 1.
 * obia_image_mark_u8_dev    : (H, W, nch) uint8 image, nch = 3 or 1 (grey, replicated), and its label raster -> (H, W, 3) uint8:
 *                             rgb3 (HOST, three bytes) at the boundary pixels of obia_image_boundaries_dev, table256[v] elsewhere.
 */
#ifndef OBIA_IMAGE_H
#define OBIA_IMAGE_H

#include "obia_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int obia_image_stretch_u8_dev(obia_ctx *ctx, const void *plane, int is_f64, int64_t n, double lo, double hi, uint8_t *out);
int obia_image_gray_hist_dev(obia_ctx *ctx, const uint8_t *pixels, int nch, int64_t n, uint8_t *gray_out, int64_t *hist256_out);
int obia_image_lut_u8_dev(obia_ctx *ctx, const uint8_t *in, int64_t n, const uint8_t *lut256, int rep, uint8_t *out);
int obia_image_clahe_u8_dev(obia_ctx *ctx, const uint8_t *in, int H, int W, int nch, int ch, uint8_t *out);
int obia_image_boundaries_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, uint8_t *out);
int obia_image_mark_u8_dev(obia_ctx *ctx, const uint8_t *image, int nch, const int32_t *labels, int H, int W,
                           const uint8_t *table256, const uint8_t *rgb3, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_IMAGE_H */
