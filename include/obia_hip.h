/*
 * obia_hip.h -- C ABI of libobia_hip.so: the MI355X (gfx950) tiled-SLIC + zonal-statistics path
 * that drops in behind obia.segmentation.segment(method="slic") and
 * obia.utils.tiling.create_tiled_segments.
 *
 * The reference (iosefa/obia) is pure Python and has no FFI of its own; the boundary is defined by
 * its call sites.  Each entry point below names the reference interface it replaces (file:line
 * under /root/reference).  Plain pointers and sizes only -- no torch / numpy types.
 *
 * Conventions
 *   - every function returns 0 on success, a negative OBIA_E_* code on failure;
 *     obia_last_error() returns a thread-local message for the last failure.  No C++ exception
 *     crosses this ABI.
 *   - one obia_ctx per (device, stream).  A context is NOT thread-safe; independent contexts may
 *     run concurrently.  A context owns a growing device workspace that is reused across calls
 *     (no hipMalloc in the steady state).
 *   - `*_dev` functions take DEVICE pointers valid on the context's device and enqueue work on
 *     the context's stream; they synchronise the stream only where they return a host scalar.
 *     Functions without the suffix take HOST pointers and do H2D / D2H themselves.
 *   - images are (H, W, C) float32, band-interleaved, C-contiguous -- the layout of
 *     obia.handlers.geotif.Image.img_data (geotif.py:100, tiling.py:47).  Labels are int32.
 *   - alignment: a buffer only has to be aligned to its ELEMENT (4 bytes for float32 / int32, 8 for float64 / int64, 1 for
 *     uint8 masks), so a contiguous view at any element offset of an allocation -- `flat[1:]`, a row slab `img[r0:r1]` -- is
 *     a valid argument, for inputs and outputs alike, and gives the result the aligned buffer gives (the wide-load kernels
 *     are chosen per call from the pointers; tests/test_gpu_pointer_alignment.py, DESIGN.md "Buffer alignment").  The
 *     exceptions say so where they are declared and need 16 bytes: `hwc8` of obia_cost_bands_f32_dev, `plane` of
 *     obia_cost_select_dev and the flag plane of obia_seeds_peaks_dev / obia_seeds_peaks_gather_dev; they refuse a
 *     misaligned pointer with OBIA_E_INVALID before anything is launched.  The Python side never sends one: obia_amd.cost
 *     copies a misaligned raster or plane to an aligned buffer first, and obia_amd.seeds allocates the flag plane itself.
 *   - outputs: a call that returns OBIA_OK has written EVERY element of every non-null output buffer it documents -- the caller need
 *     not clear them, and what they held before does not reach the result -- and has written nothing outside them and nothing to
 *     its inputs.  The elements a call leaves as they were are named where the output is declared (rows at and above K of the stage
 *     buffers, entries at and above the returned counts of the polygon buffers, `smooth_out` with sigma == 0); a refused call writes
 *     nothing outside its outputs and promises nothing about their contents (tests/test_gpu_output_guards.py, DESIGN.md "Output
 *     buffers").
 */
#ifndef OBIA_HIP_H
#define OBIA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OBIA_ABI_VERSION 2   /* 2 (round 3): obia_slic_params grew sigma_zyx, spacing_zyx */

#define OBIA_OK 0
#define OBIA_E_INVALID (-1)     /* bad argument (Python side raises ValueError)                     */
#define OBIA_E_HIP (-2)         /* HIP runtime error                                                */
#define OBIA_E_NOMEM (-3)
#define OBIA_E_UNSUPPORTED (-4) /* valid in the reference, not implemented here (NotImplementedError) */
#define OBIA_E_EMPTY (-5)       /* empty / fully masked input (the reference raises ValueError; the tiler
                                   catches it per tile, tiling.py:149-150)                          */
#define OBIA_E_NONFINITE (-6)   /* constant band (0/0 in normalize_band) or NaN/inf input           */

typedef struct obia_ctx obia_ctx;

int obia_abi_version(void);
const char *obia_last_error(void);

/* Create a context on `device_id` with its own HIP stream / on a caller-owned hipStream_t. */
obia_ctx *obia_create(int device_id);
obia_ctx *obia_create_on_stream(int device_id, void *hip_stream);
/* A context that an open tiler session holds (obia_tiler_create, below) is NOT destroyed: the call sets the error text and returns,
 * nothing the session uses is freed.  obia_tiler_destroy comes first, then obia_destroy.                                         */
void obia_destroy(obia_ctx *ctx);
int obia_synchronize(obia_ctx *ctx);
/* bytes of device workspace currently held by the context */
int64_t obia_workspace_bytes(obia_ctx *ctx);

/* SLIC parameters: the keyword arguments obia forwards untouched to skimage.segmentation.slic
 * (segment.py:86 -> segment_boundaries.py:51; tiling.py:137-143). */
typedef struct obia_slic_params {
    double compactness;            /* doubles: Python floats, so 1/compactness and int(factor*size)   */
    double min_size_factor;        /* round exactly as in the reference                               */
    double max_size_factor;
    int32_t n_segments;
    int32_t max_num_iter;          /* scikit-image `max_num_iter` (`max_iter` before 0.19)            */
    int32_t convert2lab;           /* -1 auto (Lab iff C == 3), 0, 1                                  */
    int32_t enforce_connectivity;
    int32_t slic_zero;             /* 1 = SLIC-zero: colour term / max colour distance of the cluster  */
    int32_t start_label;           /* 0 or 1                                                          */
    int32_t normalize_bands;       /* 1: apply normalize_band (segment_boundaries.py:11-16,32-33) to
                                      every band before segmenting, as create_segments does           */
    int32_t exit_on_fixed_point;   /* 1: stop sweeping a raster / tile as soon as a sweep starts from centroid
                                      records that are bit-identical to those of the previous sweep: every
                                      later sweep would reproduce the same labels and the same centroids, so
                                      the result is bit-identical to running all max_num_iter sweeps (the
                                      reference's own `if change == 0: break` intends this but never fires).
                                      0: always run max_num_iter sweeps.  Default 0.                    */
    int32_t reserved;              /* (keeps the doubles below 8-byte aligned; 0)                          */
    double sigma_zyx[3];           /* scikit-image `sigma`: Gaussian pre-smoothing per axis (depth, row, column) of the
                                      (1, H, W, C) image slic() builds -- scipy.ndimage.gaussian_filter, mode 'reflect',
                                      truncate 4, applied after the Lab conversion and before `* 1/compactness`
                                      (slic_superpixels.py; a scalar `sigma` is the same value three times: the one-plane
                                      depth axis is filtered too).  0 = none, the default.  A caller that mirrors slic()
                                      divides a SCALAR sigma by the spacing first and passes a sequence as it is.       */
    double spacing_zyx[3];         /* scikit-image `spacing`: voxel size per axis (depth, row, column); the row / column
                                      differences are scaled by it before they are squared (_slic.pyx: dy = (sy * (cy - y))^2).
                                      (1, 1, 1) = the default.  Anything else takes the direct (unstaged) sweep path: exact,
                                      not tuned -- anisotropic pixels are rare in rasters.                              */
} obia_slic_params;

void obia_slic_default_params(obia_slic_params *p);

/* ---- B1: segmentation operator --------------------------------------------------------------------
 * Replaces  `segments = slic(img_to_segment, **kwargs)`  (segment_boundaries.py:48-51) together with
 * the per-band normalisation in front of it (segment_boundaries.py:32-33, when normalize_bands=1).
 *   img        (H,W,C) float32; not modified
 *   mask       (H,W) uint8, nullable; 0 = excluded (labelled start_label-1)
 *   labels_out (H,W) int32: consecutive labels from start_label (after connectivity enforcement)
 *   n_labels_out  host int: number of labels produced
 * With a mask the maskSLIC structure of the reference is kept (spatial-only pre-pass, then the
 * main pass) but seeding uses the deterministic masked-grid rule documented in DESIGN.md.            */
int obia_slic_f32(obia_ctx *ctx, const float *img_hwc, int H, int W, int C, const uint8_t *mask,
                  const obia_slic_params *params, int32_t *labels_out, int *n_labels_out);
int obia_slic_f32_dev(obia_ctx *ctx, const float *img_hwc, int H, int W, int C, const uint8_t *mask,
                      const obia_slic_params *params, int32_t *labels_out, int *n_labels_out);

/* Stage-level entry points (device pointers), used by the parity tests to compare each stage with
 * the oracle: labels before connectivity enforcement, and connectivity enforcement alone
 * (restates _enforce_label_connectivity_cython, slic_superpixels.py:320-328).                        */
int obia_slic_assign_only_f32_dev(obia_ctx *ctx, const float *img_hwc, int H, int W, int C,
                                  const uint8_t *mask, const obia_slic_params *params,
                                  int32_t *labels_pre_out, int *n_centroids_out);
int obia_enforce_connectivity_i32_dev(obia_ctx *ctx, const int32_t *labels_in, int H, int W,
                                      int min_size, int max_size, int start_label,
                                      int32_t *labels_out, int *n_labels_out);

/* B1 with caller-supplied initial centroids instead of the library's seeding rule: the output of scikit-image's
 * own `_get_mask_centroids(mask, n_segments)` (slic_superpixels.py:14-68: RandomState / kmeans2 / pdist --
 * obia_mask_centroids_dev below restates everything after the random picks) or of `_get_grid_centroids` (:71-104).  Everything after
 * the seeding is the reference's: `step = max(steps)` (:288), spatial-only pre-pass when a mask is given (:310-314),
 * main pass, connectivity with segment_size = mask.sum() / n_centroids (:321-326).  This is how the maskSLIC path
 * every tile of create_tiled_segments takes (tiling.py:121-143) is pinned on scikit-image output.
 *   seeds->yx        HOST pointer, n x (y, x) float64 centroid positions in pixel coordinates
 *   seeds->steps_zyx the `steps` array returned with them (depth axis first; 1.0 for a 2-D image)
 *   params->n_segments is not used for seeding (K = seeds->n)
 *   stage 0: final labels (n_out = number of labels); 1: labels before connectivity (n_out = K).               */
typedef struct obia_slic_seeds {
    const double *yx;
    double steps_zyx[3];
    int32_t n;
    int32_t reserved;
} obia_slic_seeds;
int obia_slic_seeded_f32_dev(obia_ctx *ctx, const float *img_hwc, int H, int W, int C, const uint8_t *mask,
                             const obia_slic_params *params, const obia_slic_seeds *seeds, int stage,
                             int32_t *labels_out, int *n_out);

/* maskSLIC seeds as scikit-image 0.18 computes them (`_get_mask_centroids`, slic_superpixels.py:14-68), bit for bit, from the random
 * picks on: the picks come from NumPy's `RandomState(123)` and stay the caller's (obia_amd.segmentation.mask_centroids draws them).
 * "Rank" = position of a valid pixel among the mask's valid pixels in row-major order.
 *   1. code book = the pixels of rank picks[0..n_picks): the initial centroids; points = the pixels of rank dense_picks[0..n_dense),
 *      or every valid pixel when dense_picks is null
 *   2. `iters` iterations (scikit-image: 5) of scipy.cluster.vq.kmeans2: every point joins the FIRST centroid at the least
 *      ((0 + dz*dz) + dy*dy) + dx*dx (float64, separate multiply and add); a centroid becomes sum / count of its points, one
 *      division per coordinate; a centroid without points stays where it is
 *   3. per centroid the FIRST other centroid at the least sqrt(squared distance) (pdist + argmin: roots are compared);
 *      steps = abs(centroids - centroids[closest]).mean(0), columns summed in row order
 * The sums are 64-bit integer atomics, so two calls agree bit for bit.  One lane per point (step 2) or centroid (step 3) scans the
 * code book through LDS, OBIA_MASK_SEEDS_CHUNK centroids at a time: brute force, n_points * n_picks distances per iteration.
 *   mask                  DEVICE (H, W) uint8, any non-zero byte = valid
 *   picks, dense_picks    HOST int64, strictly ascending, every value in [0, n_valid)
 *   centroids_yx_out      HOST (n_picks, 2) float64 (y, x): the layout obia_slic_seeds.yx takes
 *   steps_zyx_out         HOST 3 float64, depth axis first (0 for the one-plane depth axis): obia_slic_seeds.steps_zyx
 * OBIA_E_INVALID: a null pointer, n_picks < 1, n_dense < 1 with dense_picks given, iters < 0, an unsorted or out-of-range pick.    */
#define OBIA_MASK_SEEDS_CHUNK 1024
int obia_mask_centroids_dev(obia_ctx *ctx, const uint8_t *mask, int H, int W, const int64_t *picks, int32_t n_picks,
                            const int64_t *dense_picks, int64_t n_dense, int iters, double *centroids_yx_out,
                            double *steps_zyx_out);

/* SLIC stage by stage (tests and diagnostics): the call of obia_slic_assign_only_f32_dev -- the same function runs both, so the same
 * settings, layout, candidate lists, colour bound and repeat on orphans -- that also hands out what the stages produced.  `seeds` is
 * nullable (the library's seeding rule).  Every pointer of `stages` is a nullable DEVICE buffer; the scalars are written on return.
 *   features   (H, W, C) float32: the features the sweeps read -- normalise -> Lab -> Gaussian -> * float32(1 / compactness) -- taken
 *              out of the sweeps' own plane layout and divided by `prescale` (a power of two: exact)
 *   seeds_yx   (K, 2) float32: the initial centroid positions
 *   centroids  (K, 2 + C) float32: cy, cx, colours / prescale of the records the LAST sweep assigned from.  With max_num_iter = N these
 *              are the centroids of sweep N and labels_pre the labels of sweep N; the sums are integers, so a run with another N
 *              reproduces the earlier sweeps exactly.  Needs max_num_iter >= 1.
 *   labels_pre (H, W) int32: labels before connectivity
 *   centroid_capacity  rows that seeds_yx / centroids hold (K above it is OBIA_E_INVALID; H * W always suffices); rows at and above K
 *              are not written
 *   prepass_only  1 with a mask: stop after the spatial-only pre-pass, so that centroids / labels_pre are those of its last sweep
 *              (sweep max_num_iter, or prepass_iters when that is given) (labels_pre: what that sweep assigns; the full run never stores them).  The centroids the colour pass
 *              starts from are `centroids` of a full run with max_num_iter = 1.
 *   prepass_iters  with a mask: sweeps of the spatial pre-pass; 0 = max_num_iter, as every other entry point runs it.  Colour sweeps
 *              N - 1 and N after the SAME pre-pass come from two runs with this count fixed and max_num_iter = N - 1, N.
 *   K, step, prescale, fscale  out: centroid count; `step` of _slic_cython; the power of two folded into the planes and the centroid
 *              colours; the power of two the colour sums are truncated at, in units of the handed-out features: a pixel adds
 *              (int)(feature * fscale) to its centroid's 64-bit sum -- the largest power of two with max|feature| * fscale < 2^29.  */
typedef struct obia_slic_stages {
    float *features;
    float *seeds_yx;
    float *centroids;
    int32_t *labels_pre;
    int32_t centroid_capacity;
    int32_t prepass_only;
    int32_t prepass_iters;
    int32_t K;
    double step;
    double prescale;
    double fscale;
} obia_slic_stages;
int obia_slic_stages_f32_dev(obia_ctx *ctx, const float *img_hwc, int H, int W, int C, const uint8_t *mask,
                             const obia_slic_params *params, const obia_slic_seeds *seeds, obia_slic_stages *stages);

/* ---- B2: zonal-statistics operator ----------------------------------------------------------------
 * Replaces the per-segment loop crop_image_to_bbox -> mask_image_with_polygon ->
 * calculate_spectral_stats (segment_statistics.py:475-491, :143-172; utils/utils.py:37-67), batched
 * over all segments: "pixels inside polygon p" == "pixels carrying label p" (SURVEY.md 3.3).
 *   raw     (H,W,C) float32 RAW (un-normalised) raster
 *   labels  (H,W) int32; labels outside [start_label, start_label+n_labels) are ignored
 *   bands   n_bands band indices (nullable = all C bands)
 *   outputs: count[n_labels] int64; mean/var [n_labels*n_bands] float64 (var: ddof 0);
 *            min/max [n_labels*n_bands] float32.  Empty label -> NaN (segment_statistics.py:150-162). */
int obia_zonal_stats_f32(obia_ctx *ctx, const float *raw_hwc, const int32_t *labels_hw, int H, int W, int C,
                         const int32_t *bands, int n_bands, int n_labels, int start_label,
                         int64_t *count_out, double *mean_out, double *var_out, float *min_out, float *max_out);
int obia_zonal_stats_f32_dev(obia_ctx *ctx, const float *raw_hwc, const int32_t *labels_hw, int H, int W, int C,
                             const int32_t *bands, int n_bands, int n_labels, int start_label,
                             int64_t *count_out, double *mean_out, double *var_out, float *min_out, float *max_out);

/* ---- B2 (next row f2): skewness and kurtosis per (label, band) ---------------------------------------------------
 * Completes calculate_spectral_stats (segment_statistics.py:173-175: scipy.stats.skew / kurtosis with their defaults,
 * bias=True, fisher=True; NaN for nearly constant data as scipy >= 1.9 does, with float32 eps).  Second pass over
 * (labels, raw) with the per-label means as pivots (central power sums in float64).
 *   var_out (may be NULL): receives the central m2 of this pass -- the variance about the first pass's mean, which
 *   replaces the first pass's variance (same value within float64 rounding, no shift conversions) -- at EVERY entry: NaN
 *   for an empty label and for a band without a valid pixel, like skew_out and kurt_out, so a fresh buffer is as good as
 *   the first pass's table
 *   _dev : mean_dev = the mean table of obia_zonal_stats_f32_dev [n_labels*n_bands]; outputs on the device
 *   host : runs both passes itself; outputs [n_labels*n_bands] float64 on the host                              */
int obia_zonal_moments_f32_dev(obia_ctx *ctx, const float *raw_hwc, const int32_t *labels_hw, int H, int W, int C,
                               const int32_t *bands, int n_bands, int n_labels, int start_label,
                               const double *mean_dev, double *skew_out, double *kurt_out, double *var_out);
int obia_zonal_moments_f32(obia_ctx *ctx, const float *raw_hwc, const int32_t *labels_hw, int H, int W, int C,
                           const int32_t *bands, int n_bands, int n_labels, int start_label,
                           double *skew_out, double *kurt_out, double *var_out);

/* ---- next row f1: label raster -> polygon rings ------------------------------------------------------------------
 * Replaces the vectorisation loop of create_segments (segment_boundaries.py:59-77: per segment id a full-raster
 * mask + rasterio.features.shapes / GDAL polygonize, 4-connected) with one pass over the label raster.
 *   labels      (H,W) int32 on the device; labels < start_label (masked pixels, -1 / 0) get no polygon
 *   rings       every closed chain of pixel edges around a label, the label on the RIGHT of the direction of travel
 *               (exterior rings clockwise on screen, holes counter-clockwise), in raster order of the ring's smallest
 *               corner; ring r owns vertices [ring_offset[r], ring_offset[r+1]) of xy
 *   xy          (x, y) int32 pixel-CORNER coordinates, (0,0) = top-left corner of the raster; vertices only where the
 *               direction changes; first vertex repeated at the end.  Map coordinates = affine * (x, y).
 *   ring_label  label of the ring; ring_is_hole 1 for an interior ring of that label.
 * Two calls: _count returns the sizes, _rings fills caller-allocated DEVICE buffers of at least that capacity
 * (ring_offset holds n_rings + 1 entries; entries at and above the returned counts are not written, and a capacity below
 * the count is OBIA_E_NOMEM before anything is written).  A label is one 4-connected component (the output of B1 / B3). */
int obia_polygon_count_i32_dev(obia_ctx *ctx, const int32_t *labels_hw, int H, int W, int start_label,
                               int64_t *n_rings_out, int64_t *n_vertices_out);
int obia_polygon_rings_i32_dev(obia_ctx *ctx, const int32_t *labels_hw, int H, int W, int start_label,
                               int64_t cap_rings, int64_t cap_vertices, int32_t *ring_label, uint8_t *ring_is_hole,
                               int64_t *ring_offset, int32_t *xy, int64_t *n_rings_out, int64_t *n_vertices_out);

/* ---- row f4, the way back: polygon rings -> label raster -----------------------------------------------------------
 * Replaces rasterio.features.rasterize(shapes, fill, all_touched=False) of rasterise_slic_gpkg (utils/cost.py:51-86).
 *   xy_pix       (V, 2) double PIXEL coordinates (x = column axis, y = row axis, (0,0) = top-left corner of the raster)
 *   ring_offset  (n_rings + 1) int64, starts at 0, never decreases; ring r owns vertices [ring_offset[r], ring_offset[r+1])
 *                and is closed by an edge from its last vertex to its first (a repeated first vertex adds nothing)
 *   ring_shape   (n_rings) int32, non-decreasing: the shape every ring belongs to (exterior rings and holes alike)
 *   shape_value  (n_shapes) int32 burn value of every shape
 *   out_hw       (H, W) int32 on the device
 * An edge (x0,y0)->(x1,y1) counts for the pixel centre (xc, yc) = (c + 0.5, r + 0.5) when (y0 <= yc) != (y1 <= yc) and
 * x0 + (yc - y0) * (x1 - x0) / (y1 - y0) <= xc (doubles, this order, no contraction); a shape covers the pixel iff an odd
 * number of its edges count; the pixel gets the value of the LAST covering shape in input order, else `fill`.  Rings may
 * lie outside the raster.  H * W, V, n_rings or n_shapes at or above 2^31: OBIA_E_UNSUPPORTED.
 * obia_rasterize_info (developer aid): info[0], info[1] = shapes the last call of this process handled one wave each /
 * sent to the banded large-shape path; info[2], info[3] = the most edges and the longest bounding-box side (pixel
 * centres) of the one-wave path.                                                                                      */
int obia_rasterize_polygons_dev(obia_ctx *ctx, const double *xy_pix, const int64_t *ring_offset, int64_t n_rings,
                                const int32_t *ring_shape, const int32_t *shape_value, int64_t n_shapes,
                                int H, int W, int32_t fill, int32_t *out_hw);
int obia_rasterize_info(int64_t info[4]);

/* ---- next row f4: consumers of the label raster -----------------------------------------------------------------
 * obia_label_edges_u8_dev   : `slic_edge` (obia/utils/cost.py:44-48): edge[y][x] = 1 when the label differs from the
 *                             pixel below or from the pixel to the right; n_edge_out = number of edge pixels (the
 *                             percentile normalisation of cost.py:21-26 on a 0/1 image only needs that count).
 * obia_sample_labels_i32_dev: the point-in-segment join of `label_segments` (obia/utils/utils.py:12-34) on a label
 *                             raster.  inverse_affine6 = [a, b, d, e, xoff, yoff] (HOST pointer) maps map coordinates
 *                             to pixel-corner coordinates (col = a*X + b*Y + xoff, row = d*X + e*Y + yoff); the point
 *                             takes the label of pixel (floor(row), floor(col)), `outside_value` outside the raster.
 *                             points_xy [n][2] float64 and labels_out [n] are DEVICE pointers.                     */
int obia_label_edges_u8_dev(obia_ctx *ctx, const int32_t *labels_hw, int H, int W, uint8_t *edge_out_hw, int64_t *n_edge_out);
int obia_sample_labels_i32_dev(obia_ctx *ctx, const int32_t *labels_hw, int H, int W, const double *inverse_affine6,
                               const double *points_xy, int64_t n_points, int outside_value, int32_t *labels_out);

/* ---- cost surface (obia/utils/cost.py: make_cost_surface and its layers) ------------------------------------------
 * All pointers are DEVICE pointers unless marked HOST; every call is asynchronous on the context's stream except the
 * two that return a count (select, edge count), which read it back.  Exactness contract: DESIGN.md "Cost surface".
 * obia_cost_bands_f32_dev    : (H, W, 8) float32 WorldView-3 raster (C B G Y R RE N1 N2, 16-byte aligned) -> the C band
 *                              and 1 - ndvi(R, N1), float32, in one pass.
 * obia_cost_ndvi_f32_dev     : clip((nir - red) / (nir + red + 1e-9), -1, 1), float32.
 * obia_cost_sobel_f32_dev    : hypot(sobel(chm, axis=1), sobel(chm, axis=0)), mode "nearest", float32.
 * obia_cost_select_dev       : exact order statistics of the non-NaN values of a float32 (is_f64 = 0) or float64 plane
 *                              (16-byte aligned):
 *                              n_valid_out and bits4_out (HOST) = the float's bits of the values of rank floor(v), floor(v)+1
 *                              at v = (n_valid - 1) * q_lo, then at q_hi (both neighbours are the last value when v >= n_valid
 *                              - 1); np.nanpercentile's interpolation is left to the caller.  1 <= n < 2^32.
 * obia_cost_entropy_f32_dev  : u8 = (normalise(pan) * 255) with the given (lo, hi), then skimage's rank entropy over disk(3),
 *                              float64; table_30x32 (DEVICE) [pop][count] = (c/pop) * log(c/pop) / ln 2, column 0 = 0.
 * obia_cost_normalise_dev    : nan_to_num((clip(x, lo, hi) - lo) / (hi - lo)) of a float32 / float64 plane, float64 out.
 * obia_cost_edge_count_dev   : number of pixels whose label differs from the pixel below or to the right.
 * obia_cost_combine_dev      : clip(((w0 g + w1 p) + w2 t) + w3 e, 0, 1) -> float32 (NaN -> -9999), each layer stretched
 *                              by its (lo4[k], hi4[k]) (HOST arrays, as w4); labels may be NULL (edge term 0.0).       */
int obia_cost_bands_f32_dev(obia_ctx *ctx, const float *hwc8, int64_t n_pixels, float *pan_out, float *gap_out);
int obia_cost_ndvi_f32_dev(obia_ctx *ctx, const float *red, const float *nir, int64_t n, float *out);
int obia_cost_sobel_f32_dev(obia_ctx *ctx, const float *chm, int H, int W, float *grad_out);
int obia_cost_select_dev(obia_ctx *ctx, const void *plane, int is_f64, int64_t n, double q_lo, double q_hi, int64_t *n_valid_out,
                         uint64_t *bits4_out);
int obia_cost_entropy_f32_dev(obia_ctx *ctx, const float *pan, int H, int W, double lo, double hi, const double *table_30x32,
                              double *out);
int obia_cost_normalise_dev(obia_ctx *ctx, const void *plane, int is_f64, int64_t n, double lo, double hi, double *out);
int obia_cost_edge_count_dev(obia_ctx *ctx, const int32_t *labels_hw, int H, int W, int64_t *n_edge_out);
int obia_cost_combine_dev(obia_ctx *ctx, const float *grad, const float *gap, const double *tex, const int32_t *labels_hw, int H,
                          int W, const double *lo4, const double *hi4, const double *w4, float *out);

/* ---- next row f3: GLCM texture statistics per (label, band) ------------------------------------------------------
 * Restates calculate_textural_stats (segment_statistics.py:179-298) on the masked bounding-box crop of every segment,
 * for the band PLANE the code evidently means (the reference indexes a column, :214; see oracle/glcm.py): crop of the
 * band to the segment's bounding box, 0 outside the segment and at NaN pixels, uint8((v-min)/(max-min)*255) over that
 * crop, GLCM at distance 2 in four directions, 256 levels, symmetric, normed, scikit-image's greycoprops, mean over the
 * four angles.  out6 [6][n_labels][n_bands] float64 (device): contrast, dissimilarity, homogeneity, ASM, energy,
 * correlation; NaN for an empty label or a band without a valid pixel.                                              */
int obia_texture_stats_f32_dev(obia_ctx *ctx, const float *raw_hwc, const int32_t *labels_hw, int H, int W, int C,
                               const int32_t *bands, int n_bands, int n_labels, int start_label, double *out6);

/* ---- B1': quickshift (the alternate method of create_segments, segment_boundaries.py:48-49) ------------------
 * Replaces `segments = quickshift(img_to_segment, **kwargs)`: skimage _quickshift.py:59-74 + _quickshift_cy.pyx.
 * Arithmetic is float64, the dtype of the pinned scikit-image 0.18.3 kernel.  tie_noise_hw: the (H,W) float64
 * noise scikit-image adds to the densities, RandomState(random_seed).normal(scale=1e-5) -- generated by the host
 * (NumPy's legacy stream is stable); NULL = no noise.  labels_out: consecutive ids from 0 in ascending order of the
 * root pixel (np.unique(...)[1]).  Up to 16 bands, any kernel_size >= 1 (1 / 3 / 4 bands with kernel_size <= 5 -- the
 * reference's usual calls -- take the LDS-staged kernel, everything else the same arithmetic on global memory).
 * sigma (ABI 2): scikit-image's Gaussian pre-smoothing, `ndi.gaussian_filter(image, [sigma, sigma, 0])` on the float64 image after
 * the Lab conversion and before `* ratio`; 0 = none.                                                                        */
int obia_quickshift_f32(obia_ctx *ctx, const float *img_hwc, int H, int W, int C, double ratio, double kernel_size,
                        double max_dist, double sigma, int convert2lab, const double *tie_noise_hw, int normalize_bands,
                        int32_t *labels_out, int *n_labels_out);
int obia_quickshift_f32_dev(obia_ctx *ctx, const float *img_hwc, int H, int W, int C, double ratio, double kernel_size,
                            double max_dist, double sigma, int convert2lab, const double *tie_noise_hw, int normalize_bands,
                            int32_t *labels_out, int *n_labels_out);

/* Stage-level entry point (device pointers), used by the parity tests to compare each stage of quickshift with the
 * oracle (obia_oracle_quickshift_stages).  Arguments and results of obia_quickshift_f32_dev, plus these outputs, each
 * nullable, each one device-to-device copy at the point named (the production entries launch exactly what they did):
 *   staged_out      [C][H][W] float64: the image after Lab, smoothing and `* ratio` (what the window kernels read)
 *   noise_out       [H][W] float64: the noise added to the densities (zeros when tie_noise_hw is NULL)
 *   dens_out        [H][W] float64: densities after P1, noise included
 *   parent_out      [H][W] int32: nearest pixel of higher density after P2, BEFORE the max_dist cut (itself if none)
 *   dist_parent_out [H][W] float64: the distance to it after P2 (+inf if none)
 *   roots_out       [H][W] int32: the root of every pixel after the cut and pointer jumping                          */
int obia_quickshift_stages_f32_dev(obia_ctx *ctx, const float *img_hwc, int H, int W, int C, double ratio, double kernel_size,
                                   double max_dist, double sigma, int convert2lab, const double *tie_noise_hw, int normalize_bands,
                                   int32_t *labels_out, int *n_labels_out, double *staged_out, double *noise_out, double *dens_out,
                                   int32_t *parent_out, double *dist_parent_out, int32_t *roots_out);

/* ---- B3: tiled driver ------------------------------------------------------------------------------
 * Replaces the tile loops of create_tiled_segments (tiling.py:103-291) on label rasters: pass 1
 * "black" checkerboard tiles on exact windows, pass 2 "white" tiles on windows grown by `buffer`,
 * existing segments wholly inside a grown window (minus the two bottom corner squares) are erased
 * and re-segmented, straddling ones are kept and masked out (tiling.py:205-260); ids 1..N at the
 * end (tiling.py:289-290).  n_segments per tile: params->n_segments scaled by valid area if > 0,
 * else the reference's crown rule round(valid_px * pixel_area / (pi * crown_radius^2))
 * (tiling.py:126-135).
 *   row0/rows: this call processes tile rows whose first pixel row lies in [row0, row0+rows) of the
 *   full H-row raster (multi-GPU slabs); pass 0,H for the whole raster.                               */
typedef struct obia_tiling_params {
    double crown_radius;
    double pixel_width;    /* |geotransform[1]| */
    double pixel_height;   /* |geotransform[5]| */
    int32_t tile_size;
    int32_t buffer;
    int32_t white_order;   /* 0: white tiles in the reference's raster order (tile-row by tile-row);
                              1: two parity classes of tile rows (even rows, then odd rows) -- the order
                              the sharded driver needs so that neighbouring slabs never touch the same seam
                              at once; both orders give the same kind of result, they differ in who wins
                              the 2*buffer x 2*buffer corner overlaps of diagonal white neighbours          */
    int32_t reserved;
} obia_tiling_params;

int obia_tiled_slic_f32_dev(obia_ctx *ctx, const float *img_hwc, const uint8_t *mask, int H, int W, int C,
                            const obia_tiling_params *tiling, const obia_slic_params *params,
                            int32_t *labels_out, int64_t *n_segments_out);
int obia_tiled_slic_f32(obia_ctx *ctx, const float *img_hwc, const uint8_t *mask, int H, int W, int C,
                        const obia_tiling_params *tiling, const obia_slic_params *params,
                        int32_t *labels_out, int64_t *n_segments_out);

/* Seeding rule of the tiles.  OBIA_SEEDING_GRID (the default of the calls above and of a new session): the deterministic
 * masked-grid rule.  OBIA_SEEDING_SKIMAGE: every tile is seeded as scikit-image 0.18 seeds maskSLIC (`_get_mask_centroids`,
 * slic_superpixels.py:14-68 -- what every tile of the reference goes through, tiling.py:137-143), from the tile's own mask
 * window: for a white tile the input mask minus kept segments and corner squares.  The random picks stay the caller's (NumPy's
 * frozen legacy generator): the library asks `picks` for the two sorted rank lists of (n_valid, n_segments) of each tile and
 * runs the kernels of obia_mask_centroids_dev on the window (5 k-means iterations); K = min(n_segments, n_valid) centroids,
 * step = max(steps) as it comes out of the seeding -- not divided by `spacing`, like slic(seeding="skimage") of the
 * single-raster call.  A tile with n_segments < 2 or fewer than two valid pixels is skipped like an empty tile (scikit-image
 * divides by a zero step there; the reference's tile loop swallows the ValueError, tiling.py:149-150).
 *   obia_pick_fn: user, the tile's valid-pixel count and n_segments in; *idx / *n_idx = min(n_segments, n_valid) strictly
 *   ascending ranks among the valid pixels of the tile window in row-major order (the initial centroids), *dense / *n_dense =
 *   the ranks of the points k-means runs on, *dense = NULL: every valid pixel.  Returns 0, anything else fails the call with
 *   OBIA_E_INVALID.  The pointers stay valid until the next call of the function; it is called on the host thread of the
 *   library call, once per tile that is segmented.
 * Selecting OBIA_SEEDING_SKIMAGE without a function is OBIA_E_INVALID.                                                       */
#define OBIA_SEEDING_GRID 0
#define OBIA_SEEDING_SKIMAGE 1
typedef int (*obia_pick_fn)(void *user, int64_t n_valid, int32_t n_segments, const int64_t **idx, int32_t *n_idx,
                            const int64_t **dense, int64_t *n_dense);
int obia_tiled_slic_seeded_f32_dev(obia_ctx *ctx, const float *img_hwc, const uint8_t *mask, int H, int W, int C,
                                   const obia_tiling_params *tiling, const obia_slic_params *params, int seeding,
                                   obia_pick_fn picks, void *picks_user, int32_t *labels_out, int64_t *n_segments_out);
int obia_tiled_slic_seeded_f32(obia_ctx *ctx, const float *img_hwc, const uint8_t *mask, int H, int W, int C,
                               const obia_tiling_params *tiling, const obia_slic_params *params, int seeding,
                               obia_pick_fn picks, void *picks_user, int32_t *labels_out, int64_t *n_segments_out);

/* ---- B3, sharded: the same tile loops as a session, for slabs of a raster spread over several GPUs --------
 * The caller holds rows [row0, row0 + H_local) of a (H_global, W) raster on this GPU: its slab plus the halo
 * rows its white windows reach (`buffer` rows, +1 label row so that "segment continues beyond the halo" can be
 * seen).  labels_local (same rows) is the persistent label raster G of the session: provisional ids 1..next_id-1,
 * 0 = no segment.  Between passes the host exchanges halo rows of G with the neighbouring ranks (RCCL send/recv)
 * and registers the segments it imported with obia_tiler_set_segments (their pixel counts as seen locally;
 * 0xffffffff for a segment that continues beyond the halo and can therefore never be "within" a window).
 * tile rows are GLOBAL indices; row_parity -1 = all rows, 0/1 = rows of that parity (white_order 1).
 * A session HOLDS its context from obia_tiler_create to obia_tiler_destroy: its persistent state lives in the
 * context's workspace, which every other call would reset.  While it is open every entry point that takes that
 * context -- a second obia_tiler_create included, which returns null -- answers OBIA_E_INVALID with the text
 * "context is held by an open tiler session" and touches nothing; the session's own entry points are unaffected.
 * Work for other calls needs a context of its own.
 * Stream: obia_tiler_create queues its clears and returns without waiting for the context's stream; every other entry point of a
 * session that queues work (run, set_segments, get_alive, set_alive, import_seam, finalize, destroy) has waited for the stream when
 * it returns -- the caller reads labels_local and the outputs on a stream of its own.  obia_tiler_next_id and obia_tiler_set_seeding
 * touch host fields only.  A set_segments of no segments and an import of an empty seam return at once.                    */
typedef struct obia_tiler obia_tiler;
obia_tiler *obia_tiler_create(obia_ctx *ctx, const float *img_local, const uint8_t *mask_local, int H_local, int W, int C,
                              int H_global, int row0, const obia_tiling_params *tiling, const obia_slic_params *params,
                              int32_t *labels_local, int extra_ids);
void obia_tiler_destroy(obia_tiler *t);
int obia_tiler_run(obia_tiler *t, int white, int tile_row_lo, int tile_row_hi, int row_parity);
int obia_tiler_next_id(obia_tiler *t);
int obia_tiler_set_segments(obia_tiler *t, int first_id, int count, const uint32_t *sizes_dev);
/* alive flags of the provisional ids [0, count): 1 = the segment exists, 0 = dropped (it was `within` a white
 * window) or never created.  A rank that dropped a neighbour's segment tells the owner, which clears the flag. */
int obia_tiler_get_alive(obia_tiler *t, uint8_t *alive_out_dev, int count);
int obia_tiler_set_alive(obia_tiler *t, const uint8_t *alive_in_dev, int count);
int obia_tiler_finalize(obia_tiler *t, int64_t *n_segments_out);
/* Seeding rule of the session's later passes (OBIA_SEEDING_*, see obia_tiled_slic_seeded_f32_dev); `picks` and `picks_user`
 * must outlive the session.  Every rank draws its own tiles' picks: they depend on (n_valid, n_segments) only.            */
int obia_tiler_set_seeding(obia_tiler *t, int seeding, obia_pick_fn picks, void *picks_user);
/* Import of a seam (round 4): the boundary label rows a neighbouring rank sent, as wire codes, become local ids in ONE call --
 * the step between `ncclRecv` and the next pass (semantic anchor obia/utils/tiling.py:289-290: one id space).
 *   codes_dev [n]        int32: (owner_rank + 1) << 24 | the owner's local id; 0 = no segment
 *   fmap_dev [fmap_cap]  int32, persistent per (session, owner): the owner's local id -> my local id, 0 = not imported yet
 *   code_of_dev [cap]    int32, persistent per session: my local id -> wire code of an imported segment (0: one of my own);
 *                        the caller keeps cap above obia_tiler_next_id() + n
 *   ids_out_dev [n]      int32: my local ids (codes of `my_rank` map to their id field, codes of other owners to 0)
 * Codes of `owner_rank` that are not in fmap yet get consecutive new local ids in ascending order of the owner's ids, starting
 * at *first_new_out = obia_tiler_next_id(); the range is registered like obia_tiler_set_segments(first, n_new, 0xffffffff...)
 * (sizes follow from the caller's view of its halo).  *max_owner_id_out = the largest owner id on the seam: when it is
 * >= fmap_cap the ids beyond the map were left out (ids_out 0) and the caller calls again with a larger map (entries kept; what
 * the first call imported -- *n_new_out ids from *first_new_out -- stays imported).
 * OBIA_E_NOMEM when the new ids do not fit the session (obia_tiler_next_id() + n_new > its id capacity): nothing is imported,
 * fmap_dev, code_of_dev, the id counter and the alive flags are what they were before the call; ids_out_dev is unspecified.    */
int obia_tiler_import_seam(obia_tiler *t, const int32_t *codes_dev, int n, int my_rank, int owner_rank,
                           int32_t *fmap_dev, int fmap_cap, int32_t *code_of_dev, int32_t *ids_out_dev,
                           int *first_new_out, int *n_new_out, int *max_owner_id_out);

/* ---- seeds (obia/utils/seeds.py): CHM / density peaks and the cost-aware merge of seed points ------------------
 * Peaks of a float32 (H, W) plane: scipy.ndimage.gaussian_filter(plane, sigma) when sigma > 0 (mode "reflect", float32
 * intermediate), then plane == maximum_filter(plane, size = 2 * min_dist_px + 1) and plane >= threshold.  A NaN never wins
 * the maximum and a NaN pixel is never a peak.  min_dist_px <= 32.
 *   smooth_out  [H][W] float32: the smoothed plane (not written, may be NULL, when sigma == 0)
 *   flags_out   uint8, H * W rounded up to a multiple of 4096 bytes, 16-byte aligned: 1 = peak
 *   offsets_out int32 [ceil(H * W / 4096) + 1]: peaks before each 4096-pixel chunk; the last entry is the count
 *   n_peaks_out (host): the count -- the one read-back.
 * The gather writes the peaks in row-major order (np.where): row, col, smooth[row, col], plane[row, col]; `smooth` is
 * `plane` itself when sigma == 0.  Outputs hold n_peaks entries.
 * Stream: the peaks call, the link and the stats return a host value and have waited for the context's stream when they return; the
 * gather and the matrix are asynchronous on it, the caller waits (obia_synchronize) before it reads their outputs.         */
int obia_seeds_peaks_dev(obia_ctx *ctx, const float *plane, int H, int W, double sigma, int min_dist_px, float threshold,
                         float *smooth_out, uint8_t *flags_out, int32_t *offsets_out, int64_t *n_peaks_out);
int obia_seeds_peaks_gather_dev(obia_ctx *ctx, const float *plane, const float *smooth, const uint8_t *flags, const int32_t *offsets,
                                int H, int W, int64_t n_peaks, int32_t *rows_out, int32_t *cols_out, float *smooth_val_out,
                                float *raw_val_out);
/* Pairwise merge of n <= 2^20 seeds at (xs, ys) (float64, device): D(i, j) of _build_distance_matrix (seeds.py:148-163),
 * float32, evaluated on the fly and never stored.  cost [H][W] float32 (device); inv6 (host) = the inverse geotransform
 * a, b, c, d, e, f with col = a x + b y + c, row = d x + e y + f; ts_host [samples] = the interior float32 values of
 * np.linspace(0, 1, samples + 2) as doubles, samples <= 128.
 * link : cluster_out[i] (int32, device) = the connected component of i in the graph D <= float32(eps), numbered by smallest
 *        member -- the labels of DBSCAN(eps, min_samples = 1, metric = "precomputed").  nonneg != 0 promises cost >= 0
 *        everywhere: with weight >= 0 a pair whose float32(xy_dist) > float32(eps) then skips its gathers (same result).
 * stats: stats4_out (host) = min, lower middle, upper middle, max of the n (n - 1) / 2 values (np.median is the float32 mean of
 *        the two middle values); all NaN and *n_nan_out > 0 when any D is NaN.
 * matrix: the full symmetric n x n matrix for n <= 512 (test hook).                                                    */
int obia_seeds_pair_link_dev(obia_ctx *ctx, const double *xs, const double *ys, int n, const float *cost, int H, int W,
                             const double *inv6, double weight, double xy_thresh, int samples, const double *ts_host, double eps,
                             int nonneg, int32_t *cluster_out, int *n_clusters_out);
int obia_seeds_pair_stats_dev(obia_ctx *ctx, const double *xs, const double *ys, int n, const float *cost, int H, int W,
                              const double *inv6, double weight, double xy_thresh, int samples, const double *ts_host,
                              float *stats4_out, int64_t *n_nan_out);
int obia_seeds_pair_matrix_dev(obia_ctx *ctx, const double *xs, const double *ys, int n, const float *cost, int H, int W,
                               const double *inv6, double weight, double xy_thresh, int samples, const double *ts_host,
                               float *matrix_out);

/* ---- classification (obia/classification/classify.py): the prediction half, for the whole segment table at once -----
 * Training stays scikit-learn on the host; these two calls replace the StandardScaler of classify.py:126-129 and the per-row
 * loop of :135-158.  All pointers are DEVICE pointers unless marked HOST; both calls synchronise the stream before they return.
 * obia_table_scale_dev : table (n_rows, n_features) float64, row-major.  mean_out / scale_out [n_features] float64: per column
 *                        over its non-NaN values, n of them: mean = sum / n; var = (sum (x - mean)^2 - (sum (x - mean))^2 / n) / n
 *                        (scikit-learn's _incremental_mean_and_var); scale = sqrt(var), or 1 where
 *                        var <= n eps var + (n mean eps)^2 (StandardScaler's constant-feature rule); an all-NaN column gives NaN
 *                        for both.  scaled_out (n_rows, n_features) float32 = (float)((x - mean) / scale), in float64 until the
 *                        cast.  No floating-point atomics: partial sums are added in an order that (n_rows, n_features) fix.
 * obia_forest_predict_dev : x (n_rows, n_features) float32.  Per tree a walk from its root: v = x[row][feature]; NaN goes left
 *                        iff missing_go_to_left, anything else goes left iff (double)v <= threshold; a node with left < 0 is a
 *                        leaf.  proba[row] = (sum over trees 0 .. T-1, in that order, float64, of value[leaf]) / (double)T.
 *                        acceptable (n_rows, n_classes) uint8, nullable: 1 = the class is a candidate for that row (NULL: all).
 *                        Outputs, each nullable: proba_out (n_rows, n_classes) float64, never filtered; pred_out [n_rows] int32 =
 *                        the first maximum of proba over the candidates (-1 when there is none); margin_out [n_rows] float64 =
 *                        the largest minus the second largest candidate value (0 on a tie at the top); written for every row, its
 *                        value unspecified for a row with fewer than two candidates.
 *                        More than 64 classes, 4096 features, 65536 trees or 2^31 - 1 nodes: OBIA_E_UNSUPPORTED.  A node whose
 *                        feature or children point outside [0, n_features) / its own tree: OBIA_E_INVALID (no walk follows it).
 * obia_forest: the trees' nodes one after the other.  left / right are indices within the node's OWN tree (scikit-learn's
 * children_left / children_right); tree t owns nodes [tree_offset[t], tree_offset[t + 1]) (the last one up to n_nodes) and its
 * root is the first of them.  value (n_nodes, n_classes) float64: what a leaf adds.  missing_go_to_left is nullable (all 0).   */
typedef struct obia_forest {
    const double *threshold;
    const int32_t *feature;
    const int32_t *left;
    const int32_t *right;
    const uint8_t *missing_go_to_left;
    const int64_t *tree_offset;       /* [n_trees], device */
    const int64_t *tree_offset_host;  /* the same values, HOST */
    const double *value;
    int64_t n_nodes;
    int32_t n_trees;
    int32_t n_classes;
} obia_forest;
int obia_table_scale_dev(obia_ctx *ctx, const double *table, int64_t n_rows, int n_features, double *mean_out, double *scale_out,
                         float *scaled_out);
int obia_forest_predict_dev(obia_ctx *ctx, const float *x, int64_t n_rows, int n_features, const obia_forest *forest,
                            const uint8_t *acceptable, double *proba_out, int32_t *pred_out, double *margin_out);

/* ---- a fitted MLPClassifier on the whole segment table (scikit-learn's _forward_pass_fast, then class filter and margin) ----
 * obia_table_scale_f64_dev : obia_table_scale_dev without the cast: the same mean_out / scale_out bit for bit (the same partial
 *                        sums), scaled_out (n_rows, n_features) float64 = (x - mean) / scale.  What MLPClassifier is handed.
 * obia_mlp_predict_dev : x (n_rows, n_features) float64, n_features = layer_sizes[0].  All arithmetic in float64, every product
 *                        and every sum rounded on its own (no fma): per layer and unit j,
 *                        z_j = ((...((0.0 + a_0 W[0,j]) + a_1 W[1,j]) + ...) + a_{n-1} W[n-1,j]) + b_j, inputs in ascending order.
 *                        Hidden activation: 0 identity, 1 relu (z > 0 ? z : 0.0), 2 tanh(z), 3 logistic 1 / (1 + exp(-z)).
 *                        Output: 0 softmax -- m = max_k z_k, e_k = exp(z_k - m), s = the e_k added in ascending k, p_k = e_k / s;
 *                        1 binary logistic -- p = 1 / (1 + exp(-z_0)), proba = [1 - p, p] (n_out = 1, n_classes = 2).
 *                        acceptable / proba_out / pred_out / margin_out: as in obia_forest_predict_dev, the same selection rule.
 *                        logits_out (n_rows, n_out) float64, nullable: the last layer before the output activation.
 *                        A NaN or an infinity in x: OBIA_E_INVALID, "Input X contains NaN or infinity" (outputs unspecified).
 *                        More than 8 weight matrices, 4096 features, 64 classes or 512 units in a hidden layer: OBIA_E_UNSUPPORTED.
 * obia_mlp: weights = coefs_[0], coefs_[1], ... each row-major (n_in, n_out), one after the other; biases = intercepts_ likewise. */
typedef struct obia_mlp {
    const double *weights;        /* device */
    const double *biases;         /* device */
    const int32_t *layer_sizes;   /* HOST: n_layers + 1 values: n_features, hidden widths ..., n_out (K, or 1 for binary logistic) */
    int32_t n_layers;             /* number of weight matrices */
    int32_t hidden_activation;    /* 0 identity, 1 relu, 2 tanh, 3 logistic */
    int32_t out_activation;       /* 0 softmax, 1 logistic (binary) */
    int32_t n_classes;
} obia_mlp;
int obia_mlp_predict_dev(obia_ctx *ctx, const double *x, int64_t n_rows, int n_features, const obia_mlp *mlp, const uint8_t *acceptable,
                         double *proba_out, int32_t *pred_out, double *margin_out, double *logits_out);
int obia_table_scale_f64_dev(obia_ctx *ctx, const double *table, int64_t n_rows, int n_features, double *mean_out, double *scale_out,
                             double *scaled_out);

/* ---- SHAP values of a tree ensemble (what shap.TreeExplainer(forest).shap_values(x) computes without background data) -----
 * obia_forest_shap_dev : x (n_rows, n_features) float32 and forest as in obia_forest_predict_dev, the same walk rule.  cover
 *                        [n_nodes] float64, device: the weight of the training rows that reached the node (scikit-learn's
 *                        weighted_n_node_samples), finite and positive.  v_t(S) from the root of tree t: value[leaf] at a leaf;
 *                        at a node whose feature is in S the value of the child the row follows; otherwise
 *                        z_left v(left) + z_right v(right), z_child = cover[child] / cover[node].  phi_out (n_rows, n_features,
 *                        n_classes) float64 = the Shapley value of every feature under (1 / T) sum_t v_t; a feature no tree tests
 *                        gets exactly 0.  base_out [n_classes] float64 = v(empty set).  sum_f phi + base = proba of
 *                        obia_forest_predict_dev up to rounding.  Path-dependent TreeSHAP per root-to-leaf path with the splits
 *                        of one feature merged; all float64, no floating-point atomics, additions in an order the forest alone
 *                        fixes (trees ascending, leaves in ascending node index): two calls agree bit for bit and a row's result
 *                        does not depend on the other rows.  The stream is synchronised before the call returns.
 *                        More than 64 classes, 4096 features, 65536 trees or 2^31 - 1 nodes, or a path that tests more than 32
 *                        distinct features: OBIA_E_UNSUPPORTED.  A node whose feature or children point outside their range, a
 *                        node that is not reached from its tree's root exactly once, or a cover that is not finite and positive:
 *                        OBIA_E_INVALID; every walk is bounded by its tree's node count.                                        */
int obia_forest_shap_dev(obia_ctx *ctx, const float *x, int64_t n_rows, int n_features, const obia_forest *forest, const double *cover,
                         double *phi_out, double *base_out);

/* ---- exact Shapley values of a fitted MLP against a background table (shap.KernelExplainer with every coalition enumerated) ----
 * obia_mlp_coalition_dev : x (n_rows, n_features), background (n_background, n_features) float64, mlp as in obia_mlp_predict_dev.
 *                        masks (n_masks, n_features) bytes, non-zero = the feature comes from x; NULL = all 2^F coalitions in
 *                        binary order (coalition m holds feature f iff bit f of m is set; n_masks must be 2^F, F <= 16).
 *                        values_out (n_rows, n_masks, n_classes) float64:
 *                        values[n, m] = (...((0.0 + p(h_0)) + p(h_1)) + ... + p(h_{B-1})) / B, h_b[f] = x[n, f] where the coalition
 *                        holds f, else background[b, f]; p = proba of obia_mlp_predict_dev for that row, the same bits.  The
 *                        background rows are added in ascending order from 0.0 and the sum is divided once by B; the empty and
 *                        the full coalition follow the same rule.  No floating-point atomics.  A NaN or an infinity in x or in
 *                        background: OBIA_E_INVALID ("Input X ..." / "Input background contains NaN or infinity").  The limits
 *                        of obia_mlp_predict_dev, fewer than 2^31 background rows and (row, coalition) pairs: OBIA_E_UNSUPPORTED;
 *                        n_background < 1 or n_masks < 1: OBIA_E_INVALID.
 * obia_shapley_combine_dev : values (n_rows, 2^F, n_classes) float64 in binary coalition order, size_weights [F] float64 on the
 *                        HOST, w[s] = s! (F - 1 - s)! / F!.  phi_out (n_rows, F, n_classes) float64:
 *                        phi[n, f, k] = the sum over the coalitions m without bit f, in ascending m from 0.0, of
 *                        w[popcount(m)] * (values[n, m | 1 << f, k] - values[n, m, k]); every difference, product and sum is
 *                        rounded on its own.  F > 16 or more than 64 classes: OBIA_E_UNSUPPORTED.  The stream is synchronised
 *                        before the call returns.                                                                            */
int obia_mlp_coalition_dev(obia_ctx *ctx, const double *x, int64_t n_rows, int n_features, const obia_mlp *mlp, const double *background,
                           int64_t n_background, const uint8_t *masks, int64_t n_masks, double *values_out);
int obia_shapley_combine_dev(obia_ctx *ctx, const double *values, int64_t n_rows, int n_features, int n_classes, const double *size_weights,
                             double *phi_out);

/* ---- measurement hooks ------------------------------------------------------------------------------
 * Time of the most recent call's kernels by class, measured with HIP events on the context's
 * stream (bench.py's roofline leg).  `what`: 0 = SLIC colour sweeps (ms): time during which a colour sweep runs, batch by
 * batch -- the sum of the launches of a batch whose sweeps run one after the other, the UNION of the launches' intervals of a
 * batch whose colour pass ran as two window groups side by side (see 19), 1 = number of those sweeps (a sweep of a grouped batch
 * is two launches and counts once), 2 = feature preparation, 3 = connectivity, 4 = zonal statistics, 5 = whole call,
 * 6 = maskSLIC spatial-only pre-pass sweeps (ms), 7 = pixels actually processed by the launches of 0
 * (sum; tiles skipped by exit_on_fixed_point are not counted), 8 = the same for the pre-pass launches,
 * 9 = pixels of the launches of 0 that also stored their labels (only the last sweep of a batch does),
 * 10 / 11 = time during which at least one colour / pre-pass sweep was running, over the whole call (10 equals 0: batches run one
 * after the other and 0 is a union inside a grouped one; 11 is below 6 where a batch's spatial pre-pass ran as two window groups side by side, see 15).  The events of a sweep are bound to its dispatch (hipExtLaunchKernelGGL): 0, 6
 * and 20 are made of the kernels' own start-to-end times, as a rocprofv3 kernel trace reports them.
 * 12 = batches of the call whose sweeps ran a second time with every sweep storing its labels (a valid pixel that no window
 * reached keeps the label of the sweep before: DESIGN.md 3.2 item 5) -- counted whether profiling is on or not.
 * 13 = the part of 8 that no sweep evaluated: pre-pass pixel-sweeps of problems whose class representative ran them (DESIGN.md 3.2,
 * "One pre-pass per class of identical tiles"); 8 counts them as covered.
 * 14 = pixels whose feature planes were written by the last pre-pass sweep from the raster (the fused feature pass)
 * instead of the feature pass: all pixels of every batch that fused, 0 when none did -- counted whether profiling is on or not.
 * 15 = spatial pre-pass sweeps launched for one of two window groups of a batch ("Two window groups in flight"):
 * 2 per grouped sweep, 0 when no batch was grouped -- counted whether profiling is on or not.
 * 16 / 17 / 18 = small commands the call issued besides its kernels: fills (a memset, or one launch of the clear kernel that
 * stands for several), host -> device uploads, device -> host read-backs -- counted whether profiling is on or not.
 * 19 = colour sweeps launched for one of two window groups of a batch ("Two window groups in flight"): 2 x max_iter
 * per grouped batch, 0 when no batch was grouped -- counted whether profiling is on or not.
 * 20 = plain sum of the durations of all colour-sweep launches (ms), overlapping or not: equals 0 when no batch was grouped, above
 * it by the overlap otherwise.
 * `enabled`: 0 off, 1 every class, 2 only the colour sweeps (an event pair costs ~2.5 us of stream time: with all classes on,
 * a step of the headline workload records ~420 pairs = 1.1 ms; bench.py times its steps in mode 2).                       */
int obia_set_profiling(obia_ctx *ctx, int enabled);
double obia_last_timing(obia_ctx *ctx, int what);

#ifdef __cplusplus
}
#endif
#endif /* OBIA_HIP_H */
