// slic.hpp -- batched SLIC engine: host-side planning structures and entry points.
#pragma once
#include "common.hpp"

namespace obia {

// One independent SLIC problem (a whole image, or one tile window of the tiled driver).
// Device-visible, read through scalar loads (wave-uniform).
struct SlicProblem {
    int H, W;            // window size in pixels
    int K;               // number of centroids
    int sy, sx;          // window steps: regular_grid((1,H,W), K) (slic_superpixels.py -> _slic_cython)
    int ncy, ncx;        // bin grid: cells of sy x sx pixels
    float spatial_w;     // float(1 / step^2)
    int cent_off;        // first centroid of this problem in the batch-wide centroid arrays
    int cell_off;        // first bin of this problem in the batch-wide bin-head array
    int tile_off;        // first workgroup of this problem in the assign grid
    int tiles_x, tiles_y;
    long long pix_off;   // first pixel of this problem in the dense per-problem pixel arrays
    long long feat_off;  // first float4 of this problem in the feature planes (see feat_block_f4)
    int XB;              // 16-column blocks per row of the feature planes: ceil(W / 16)
    int n_valid;         // valid (unmasked) pixels
    long long fb_off;    // first record of this problem in the footprint colour boxes (SlicBatch::d_fbox)
    float sp_y, sp_x;    // slic()'s `spacing` of the row / column axis as float32 (1, 1 unless the caller says otherwise)
    int direct;          // 1: every tile takes the direct (unstaged) path -- set when the spacing is not (1, 1)
    int m4_off;          // first dword of this problem in the packed mask (SlicBatch::d_mask4): ceil(H / 4) * W dwords per problem
};

// Source window of a problem inside the caller's raster (feature preparation).
struct SrcWindow {
    int y0, x0, h, w;
    long long pix_off;   // pixel-major feature layout (quickshift): first pixel
    long long feat_off;  // quad-row plane layout (SLIC): first float4
    long long fb_off;    // first footprint colour box (see feat_boxes)
};


// Feature layout of the SLIC sweeps ("quad-row blocks").  Rows are grouped in fours, columns in sixteens; the unit is one
// float4 = ONE channel of the four pixels (4q .. 4q+3, x):
//   float4 index = feat_off + ((q * XB + x / 16) * CP + c) * 16 + x % 16            XB = ceil(W / 16)
// i.e. per (quad row, 16-column block): CP runs of 256 bytes, one per channel -- 4 KB for 8 bands, contiguous.
// A lane of the sweep owns a vertical 1x4 strip, so one 16-byte load brings a channel of its four pixels as two register
// pairs (packed-f32 arithmetic on two pixels per instruction), a quarter wave reads 256 contiguous bytes (whole 128-byte
// lines), the channels of a lane are 256 bytes apart (immediate offsets of one address) and a footprint's quad row is
// one contiguous block.  Rows past H inside the last quad and columns past W inside the last block hold zeros.
inline int feat_xb(int w) { return (w + 15) >> 4; }
inline long long feat_block_f4(int h, int w, int CP) { return (long long)((h + 3) / 4) * feat_xb(w) * CP * 16; }

// Footprint colour boxes (low compactness only, SlicBatch::col_lb): for every 16 x 16 footprint of the sweep -- quad rows
// 4f .. 4f+3 of one 16-column block -- the per-channel minimum and maximum of its features, 2 * CP floats {lo[CP], hi[CP]}.
// A candidate's colour distance to the box is a lower bound of its colour term for every pixel of the footprint: when the
// colour term decides (compactness below ~1) the spatial bound alone visits 13 candidates per footprint, the sum 7.
inline long long feat_boxes(int h, int w) { return (long long)(((h + 3) / 4 + 3) / 4) * feat_xb(w); }

// regular_grid((1,H,W), n) of scikit-image (util/_regular_grid.py:61-83): start/step per axis,
// step 0 == slice(None).
void regular_grid_hw(long long H, long long W, long long n, long long out[4]);

#ifndef OBIA_SWEEP_TW
#define OBIA_SWEEP_TW 64
#endif
#ifndef OBIA_SWEEP_MAXC
#define OBIA_SWEEP_MAXC 96
#endif
constexpr int SWEEP_TW = OBIA_SWEEP_TW, SWEEP_TH = 64;   // workgroup tile of the sweep kernel (pixels)
constexpr int SWEEP_MAXC = OBIA_SWEEP_MAXC;   // candidate slots of a sweep tile (LDS slots of the sweep kernel)
constexpr int CENT_REC = 8;      // header dwords of a centroid record: cy, cx, y0, y1, x0, x1, k, -
// Accumulator record of one centroid, 128-byte aligned so a tile's flush touches two 64-B lines:
//   q[0..CP)  colour sums, 64-bit fixed point     q[CP] = n | (sum_y << 32)     q[CP+1] = sum_x
inline int acc_record_qwords(int CP) { return CP <= 12 ? 16 : 32; }

struct SlicBatch {
    int nprob = 0;
    int C = 0, CP = 0;                 // bands, bands padded to a multiple of 4
    bool masked = false;
    int start_label = 1;
    int max_iter = 10;
    // settings: filled by slic_batch_settings from the caller's parameters, the same for every batch of one call
    bool direct = false;               // anisotropic `spacing`: every tile takes the direct sweep path (SlicProblem::direct)
    int normalize = 0, to_lab = 0;     // feature pass: per-band normalisation of each window, Lab conversion
    float feat_ratio = 1.0f;           // what the feature pass multiplies by: float(1 / compactness) * prescale
    // layout: filled by slic_batch_layout from `windows`
    long long total_pix = 0, total_boxes = 0, maxpix = 1;   // total_boxes: records of d_fbox; maxpix: pixels of the largest window
    int maxh = 1;                      // rows of the tallest window
    int total_cent = 0, total_cells = 0, total_tiles = 0;   // total_tiles: largest tile count of one problem (grid.x)
    long long total_tiles_all = 0;                          // sum over problems (per-tile state of exit_on_fixed_point)
    std::vector<SlicProblem> probs;    // host copy
    std::vector<SrcWindow> windows;
    // device arrays (arena)
    SlicProblem *d_probs = nullptr;
    SrcWindow *d_windows = nullptr;
    float *d_fbox = nullptr;           // footprint colour boxes (feat_boxes), or null
    bool col_lb = false;               // the sweeps add the colour-box bound to the spatial one (see slic_use_colour_bound)
    float *d_feat = nullptr;           // quad-row planes, 4 * total_feat_f4 floats (pixel-major [total_pix][CP] when !feat_planes)
    // fused feature pass (slic_fuse_features): the feature step ran the min / max pass only; the last sweep of the spatial pre-pass
    // reads the caller's raster, normalises with the keys and writes d_feat on its way (slic_sweep.hip: RAWIN)
    bool fuse_features = false;
    const float *raw_src = nullptr;    // the caller's raster (rows of raw_ws pixels, C bands) the windows lie in
    int raw_ws = 0;
    const unsigned *d_keys = nullptr;  // [nprob][C][2] min / max keys of the batch's windows (band_minmax_kernel)
    bool feat_planes = true;           // false: pixel-major features (quickshift reads them per pixel)
    double sigma[3] = {0.0, 0.0, 0.0};   // Gaussian pre-smoothing (z, y, x), 0 = none (obia_slic_params::sigma_zyx)
    double spacing[3] = {1.0, 1.0, 1.0}; // obia_slic_params::spacing_zyx
    long long total_feat_f4 = 0;       // float4 elements of d_feat (plane layout)
    uint8_t *d_mask = nullptr;         // [total_pix] or null
    unsigned *d_mask4 = nullptr;       // the same bytes packed for the sweeps: dword (q, x) = mask of the rows 4q .. 4q+3 at column x, a byte each
                                       // (a lane's 1x4 strip in ONE load and one register); written by slic_run_sweeps from d_mask
    long long total_m4 = 0;            // dwords of d_mask4
    int32_t *d_labels = nullptr;       // [total_pix] problem-local labels (start_label based)
    float *d_seed = nullptr;           // [total_cent][2]
    int *d_cent_prob = nullptr;        // [total_cent]
    int *d_tile_prob = nullptr;        // [total_tiles_all] problem of every sweep tile, tiles numbered problem by problem in raster order
    float *d_cent = nullptr;           // [total_cent][8 + CP] records
    int *d_head = nullptr;   // two buffers of total_cells (double-buffered per sweep); list links ride in the centroid records
    int *d_head_cur = nullptr;
    unsigned long long *d_acc = nullptr;   // [total_cent] accumulator records, see acc_record_qwords()
    // cached candidate lists of the sweep tiles (slic_sweep.hip, "candidate lists"): allocated by slic_run_sweeps
    int *d_tl_k = nullptr;             // [total_tiles_all][SWEEP_MAXC] centroid indices of a tile's list, ascending
    unsigned *d_tl_fp = nullptr;       // [total_tiles_all][256] per thread: its list slot in each of its wave's four footprints (a byte each)
    int *d_tl_meta = nullptr;          // [total_tiles_all][2] {entries (-1: no list yet, -2: the tile cannot be listed), sweep it was built in}
    int *d_tl_req = nullptr;           // [total_tiles_all] last sweep in which a centroid that left its margin asked the tile to rebuild (-1: none)
    float *d_ref = nullptr;            // [total_cent][2] position a centroid's margin is measured from
    double fscale = 1.0;
    float prescale = 1.0f;             // power of two already folded into the feature planes, the spatial weight and the centroid colours (slic_prescale); fscale is what is left
    bool exit_on_fixed_point = false;
    bool slic_zero = false;            // SLIC-zero: colour term scaled by the cluster's largest colour distance so far
    bool prepass_only = false;         // stage entry only (obia_slic_stages::prepass_only): a masked batch stops after its spatial pre-pass
    int prepass_iter = 0;              // stage entry only (obia_slic_stages::prepass_iters): sweeps of the pre-pass, 0 = max_iter
    std::vector<float> step;           // per problem: `step` of _slic_cython, max(steps) of the seeding grid (slic_plan_and_seed)
    std::vector<long long> grid_n;     // per problem: the n its seeds were laid out for by the grid rule (regular_grid((1,H,W), n)); 0: no
                                       // centroids or seeds from the caller (slic_plan_and_seed; read by slic_prepass_classes)
};

// Classes of problems whose spatial pre-pass is ONE computation (slic_sweep.hip, "shared pre-pass").  The pre-pass sweeps but the
// last read a problem's shape, its seeds and its mask and nothing else, so two problems of a masked batch with the same shape, the
// same grid seeds (same H, W and n: same K, steps, bins and weight) and a mask that hides nothing run the same sweeps bit for bit.
// rep[p] = the first problem of p's class, p itself for a representative and for every problem that shares with nobody.  Returns the
// number of problems that have another problem as representative.  A pure function of the problem table.
inline int slic_prepass_classes(const std::vector<SlicProblem> &probs, const std::vector<long long> &grid_n, std::vector<int> &rep) {
    const int np = (int)probs.size();
    rep.resize(np);
    std::vector<int> reps;   // representatives so far (a handful: interior, edge and corner shapes)
    int members = 0;
    for (int p = 0; p < np; ++p) {
        const SlicProblem &P = probs[p];
        rep[p] = p;
        if ((int)grid_n.size() != np || grid_n[p] <= 0 || P.K <= 0 || P.direct) continue;
        if ((long long)P.n_valid != (long long)P.H * (long long)P.W) continue;
        bool found = false;
        for (int r : reps) {
            const SlicProblem &R = probs[r];
            if (R.H == P.H && R.W == P.W && R.K == P.K && grid_n[r] == grid_n[p] && R.sy == P.sy && R.sx == P.sx && R.ncy == P.ncy &&
                R.ncx == P.ncx && R.tiles_x == P.tiles_x && R.tiles_y == P.tiles_y && R.spatial_w == P.spatial_w && R.sp_y == P.sp_y &&
                R.sp_x == P.sp_x) {
                rep[p] = r; ++members; found = true;
                break;
            }
        }
        if (!found) reps.push_back(p);
    }
    return members;
}

// Feature preparation for every problem of the batch: per-band min/max of its window, then
// normalise (optional) -> Lab (optional) -> * 1/compactness into d_feat.  `src` is the caller's
// (Hs,Ws,C) raster.  Returns OBIA_E_NONFINITE for constant / non-finite bands.
// `skip` (nullable): when given, a problem whose window holds a constant or non-finite band is flagged
// skip[p] = 1 (its features are zero) instead of failing the whole batch -- the reference's tiler
// swallows the per-tile ValueError (tiling.py:149-150).
// Gaussian pre-smoothing of slic(..., sigma=...) (slic_superpixels.py: ndi.gaussian_filter between the Lab conversion and the scaling):
// sigma per axis (z, y, x; the depth axis has ONE plane and is filtered too, as scipy does), two scratch arrays of total_pix * CP
// floats, the weights of the three passes on the device (smooth_upload_weights) and a scratch word per window.
struct SmoothSpec {
    double sigma[3] = {0.0, 0.0, 0.0};
    float *tmp_a = nullptr, *tmp_b = nullptr;
    double *d_w[3] = {nullptr, nullptr, nullptr};   // [radius + 1]: centre first
    int radius[3] = {0, 0, 0};
    unsigned *d_scratch = nullptr;                  // [np] (max |feature| of the unscaled pass: not used)
    bool on() const { return sigma[0] > 1e-15 || sigma[1] > 1e-15 || sigma[2] > 1e-15; }
};
int smooth_prepare(obia_ctx *ctx, SmoothSpec &sm, long long total_pix, int CP, int np);
int gaussian_weights_host(double sigma, bool sigma_is_f32, std::vector<double> &w);   // returns the radius; w[0] = centre weight
// (b.d_fbox, plane layout only: the footprints' colour boxes come out of the same pass)
// minmax_only: the fused form -- keys and flags only, no planes
int slic_features_launch(hipStream_t stream, const SlicBatch &b, const float *src, int Ws, unsigned *d_keys, const SmoothSpec *smooth = nullptr,
                         bool minmax_only = false);
// Does the batch (settings filled) take the fused feature pass on this raster?  Plane layout; normalised bands with the prescale in
// the ratio (no Lab, no SLIC-zero); no smoothing; masked with at least one sweep (the last pre-pass sweep folds colours: it is the
// first reader of the planes); not direct, exit_on_fixed_point or the colour-box bound; 4, 8 or 12 bands and a 16-byte aligned raster.
// The default where it applies; OBIA_FUSE_FEATURES=0 (developer switch, read per call) forces the separate pass, 1 asks for the fused one.
bool slic_fuse_features(const SlicBatch &b, const float *src, int Ws);
// The fixed-point scale of the colour sums from the largest |feature| (SlicBatch::fscale)
double slic_fscale(float maxabs);
int slic_features_finish(SlicBatch &b, const unsigned *keys, const unsigned *nonfinite, const unsigned *maxabs_bits, std::vector<int> *skip);
int slic_prepare_features(obia_ctx *ctx, SlicBatch &b, const float *src, int Ws, std::vector<int> *skip = nullptr);
// The part of the fixed-point scale of the colour sums that is known BEFORE the features are computed -- normalised bands times
// `ratio` reach exactly `ratio` -- as a power of two.  slic_batch_settings multiplies it into the ratio of the feature pass (exact: the
// planes hold the reference's features times 2^s) and stores it in SlicBatch::prescale; slic_plan_and_seed scales the spatial weight
// by its square, the centroid colours follow from the sums: every distance is the reference's times 2^(2s), every comparison and
// every tie the same, and the sweeps convert a feature to fixed point by truncation alone (SlicBatch::fscale, taken from the largest
// |feature| as before, comes out as 1).  1 when the range is not known beforehand (no normalisation, Lab) or SLIC-zero is on.
float slic_prescale(float ratio, int normalize, int to_lab, bool slic_zero);
// Does a batch with this image ratio (1 / compactness; to_lab: the features are Lab, ~100 units wide) use the colour-box bound?
bool slic_use_colour_bound(float ratio, bool to_lab = false);
// The two halves of a batch's description, each derived in one place.  Settings: everything that follows from the caller's
// parameters (spacing other than (1, 1) turns exit_on_fixed_point and the colour bound off: the direct sweep path has neither).
// Layout: the caller puts (y0, x0, h, w) of every window into b.windows; the offsets of the windows in the dense per-pixel arrays,
// the feature planes, the colour boxes and the packed mask, b.probs (H, W and the same offsets), nprob and the totals follow.
void slic_batch_settings(SlicBatch &b, const obia_slic_params &p, int C, int normalize_bands, bool masked);
int slic_batch_layout(SlicBatch &b);
// The component sizes connectivity merges below / cuts at: segment_size = mask.sum() / n_centroids  |  prod(shape) / n_centroids
// (slic_superpixels.py:321-326; 1 for a problem without centroids), max_size clamped to [1, INT_MAX].
inline std::pair<int, int> slic_cc_sizes(double min_size_factor, double max_size_factor, int n_valid, int K) {
    const double segment_size = K > 0 ? (double)n_valid / (double)K : 1.0;
    const double mxd = max_size_factor * segment_size;
    return {(int)(min_size_factor * segment_size), mxd >= 2147483647.0 ? 2147483647 : (mxd >= 1.0 ? (int)mxd : 1)};
}

// Seeds (grid or masked grid), fills K / steps / bins in b.probs, uploads descriptors.
// n_segments[p] = requested segments of problem p.
// nvalid (nullable): valid-pixel counts already known to the caller.
// ext (nullable): externally supplied initial centroids -- scikit-image's own _get_mask_centroids output
// (slic_superpixels.py:14-68) -- instead of the grid rule; step = max(steps).  One entry per problem of the batch (a single-raster
// call passes the address of one); n = 0 marks a problem without centroids, which is skipped like an empty one.  The positions
// come from the host (yx, float64, converted like segments.astype(float32)) or, when d_yx is set, from device memory as the
// float32 pairs themselves (the tiler's per-tile seeding leaves them there: mask_centroids_queue).
struct ExternalSeeds { const double *yx; int n; double step; const float *d_yx = nullptr; };
int slic_plan_and_seed(obia_ctx *ctx, SlicBatch &b, const std::vector<int> &n_segments,
                       const std::vector<int> *nvalid = nullptr, const ExternalSeeds *ext = nullptr);
// valid (unmasked) pixels per problem: mask.sum() (tiling.py:133, slic_superpixels.py:322)
// d_cnt_cleared: one zeroed int per problem that the caller cleared beside its own fills (null: allocated and cleared here)
// counted_parts > 0: the kernel that wrote the mask has counted it already (the tiler's mask kernel holds every byte it writes) and
// left counted_parts partial sums per problem, problem p's at d_cnt_cleared[p * counted_parts ...], every one written (nothing to
// clear): no counting kernel, the read-back fetches the parts and the host adds them up
int slic_count_valid(obia_ctx *ctx, SlicBatch &b, std::vector<int> &nvalid, int *d_cnt_cleared = nullptr, int counted_parts = 0);
// the tables that depend on the window shapes only (layout version of the problems, tile -> problem table) into the open planning
// blob; the caller flushes (slic_count_valid and slic_plan_and_seed do, for a caller that did not call it)
int slic_plan_layout(obia_ctx *ctx, SlicBatch &b);

// Runs the sweeps; labels (pre-connectivity) land in b.d_labels.  Three steps, the same for every caller:
// slic_run_sweeps queues the sweeps and the read-back of their orphan flag (a valid pixel no window reached) and pixel counters, and
// returns without a host synchronisation.  Once the caller has synchronised the stream for its own reasons (the tiler: the
// connectivity stage reads its counters back), slic_sweeps_settle looks at the flag.  When it reports `repeat`, the labels are not
// final: the caller rewinds the arena to a mark taken before slic_run_sweeps (b.d_mask4 as it was then: the sweeps pack the mask
// above the mark when it was null), calls slic_rerun_storing -- every sweep stores its labels; queued like the first run, its
// labels are final in stream order -- computes again whatever it had computed from the labels, and after its next synchronisation
// calls slic_sweeps_settle(ctx, nullptr) for the repeat's pixel counters: the repeat has no round trip of its own either.
int slic_run_sweeps(obia_ctx *ctx, SlicBatch &b);
int slic_sweeps_settle(obia_ctx *ctx, bool *repeat);
int slic_rerun_storing(obia_ctx *ctx, SlicBatch &b);

// What obia_slic_stages_f32_dev hands out of a finished single-raster batch (each pointer nullable, device memory): the features the
// sweeps read -- de-tiled from the quad-row planes by the layout formula above and divided by b.prescale (a power of two: exact) --
// as (H, W, C); the seeds (K, 2); the centroid records the last sweep assigned from as (K, 2 + C) rows {cy, cx, colours / prescale}.
int slic_stage_outputs(obia_ctx *ctx, const SlicBatch &b, float *features, float *seeds_yx, float *centroids);

// maskSLIC seeds as scikit-image computes them, from the random picks on (mask_seeds.hip; arguments: obia_mask_centroids_dev, which
// has checked them -- picks sorted and >= 0, K >= 1, n_dense >= 1 when dense is given).  mask: device; everything else: host.
int mask_centroids_dev(obia_ctx *ctx, const uint8_t *mask, int H, int W, const int64_t *picks, int K, const int64_t *dense, long long n_dense,
                       int iters, double *centroids_yx_out, double *steps_zyx_out);
// The same seeding for one tile of a batch, queued on the context's stream WITHOUT a host synchronisation: `mask` is the tile's
// dense (h, w) window inside the batch's mask (SlicBatch::d_mask + pix_off -- the tiler's mask kernel built it), the picks are ranks
// among its n_valid valid pixels in the window's row-major order (the caller has counted them and checked the picks against the count).  The
// centroids land in seeds_out_dev as K float32 (y, x) pairs -- what the sweeps start from -- and the row / column means of
// |centroid - nearest other centroid| in steps_out_dev[0..1]; the caller reads the steps of all its tiles back at once.  The
// workspace is taken from the arena and given back before returning: the next tile's kernels reuse it in stream order.
int mask_centroids_queue(obia_ctx *ctx, const uint8_t *mask, int h, int w, long long n_valid, const int64_t *picks, int K, const int64_t *dense,
                         long long n_dense, int iters, float *seeds_out_dev, double *steps_out_dev);

// Connectivity enforcement on a batch of dense label maps laid out back to back (pix_off); labels come
// out consecutive over the whole batch, in problem order then raster order of each component's first pixel.
struct CcProblem { int H, W; long long pix_off; int min_size; int max_size; };   // component sizes: merge below min, cut at max
// The last step of the enforcement -- every pixel takes the final label of its component -- as data: a caller that moves the labels
// somewhere else anyway (the tiler scatters them into the raster's id space) asks for this instead of the dense label map and
// resolves each pixel where it consumes it (cc_resolve_label): one pass over the batch and 8 bytes per pixel less (round 4).
// The arrays live in the context's arena: valid until the caller rewinds it.
struct CcResolve { const int *parent; const int *newlab; const int *small_final; int start_label; int mask_label; };
#if defined(__HIPCC__)
// The label as a function of the pixel's parent alone: pixels with equal parents have equal labels, so a consumer that walks a
// column resolves where the parent changes and reuses the label above everywhere else (tiling.hip: tile_scatter_kernel).
__device__ __forceinline__ int cc_resolve_parent(const CcResolve &R, int p) {
    // (a pixel's parent is its tile-local root, whose parent is the root of the component: cc.hip, cc_roots_kernel)
    if (p < 0) return R.mask_label;
    const int r = R.parent[p];
    int nl = R.newlab[r];
    // a small component took the label at the end of its adjacency chain: followed once per COMPONENT (cc_small_final_kernel), not
    // per pixel -- a pixel of a small component costs one more gather, not four per hop (round 4)
    if (nl < 0) nl = R.small_final[-nl - 2];
    return (nl >= 0) ? nl + R.start_label : 0;   // `adjacent = 0` when no labelled neighbour exists
}
__device__ __forceinline__ int cc_resolve_label(const CcResolve &R, long long i) { return cc_resolve_parent(R, R.parent[i]); }
#endif
// labels_out: the dense label map.  deferred (nullable): when given, the final relabel pass is NOT run -- labels_out is not
// written -- and *deferred describes how to resolve a pixel.  (The component walks mark their pixels in a map of the context's
// that is all zero between calls, obia_ctx::cc_visited.)  d_probs (nullable): `probs` on the device already, as part of an upload
// the caller has queued (a tiler batch sends the table with its sweeps' descriptors); null: uploaded here.
int enforce_connectivity_batch(obia_ctx *ctx, const std::vector<CcProblem> &probs, const int32_t *labels_in,
                               long long total_pix, int start_label, int32_t *labels_out, int *h_n_labels_out,
                               CcResolve *deferred = nullptr, const CcProblem *d_probs = nullptr);

// Connectivity enforcement on one dense (H,W) label map (device pointers).
int enforce_connectivity_dev(obia_ctx *ctx, const int32_t *labels_in, int H, int W, int min_size,
                             int max_size, int start_label, int32_t *labels_out, int *d_n_labels_out);

// Zonal statistics (device pointers, outputs device).
int zonal_stats_dev(obia_ctx *ctx, const float *raw, const int32_t *labels, int H, int W, int C,
                    const int32_t *bands_host, int n_bands, int n_labels, int start_label,
                    int64_t *count, double *mean, double *var, float *mn, float *mx);
int zonal_moments_dev(obia_ctx *ctx, const float *raw, const int32_t *labels, int H, int W, int C,
                      const int32_t *bands_host, int n_bands, int n_labels, int start_label, const double *mean,
                      double *skew, double *kurt, double *var /* nullable: m2 written here */);

}  // namespace obia
