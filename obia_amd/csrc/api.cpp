// api.cpp -- the C ABI of libobia_hip.so (include/obia_hip.h): argument checking and orchestration of
// the kernels for the single-raster operators B1 (SLIC) and B2 (zonal statistics).
#include "slic.hpp"
#include "../../include/obia_testing.h"

#include <cmath>

using namespace obia;

namespace {

int check_slic_args(const float *img, int H, int W, int C, const obia_slic_params *p) {
    if (!img || !p) { set_error("null image or params"); return OBIA_E_INVALID; }
    if (H <= 0 || W <= 0 || C <= 0) { set_error("bad image shape (%d,%d,%d)", H, W, C); return OBIA_E_INVALID; }
    if ((long long)H * W > 0x7fffffffLL) { set_error("rasters above 2^31 pixels must go through the tiled driver"); return OBIA_E_INVALID; }
    if (C > 16) { set_error("more than 16 bands not supported (got %d)", C); return OBIA_E_UNSUPPORTED; }
    if (p->start_label != 0 && p->start_label != 1) { set_error("start_label should be 0 or 1."); return OBIA_E_INVALID; }
    if (p->convert2lab == 1 && C != 3) { set_error("Lab colorspace conversion requires a RGB image."); return OBIA_E_INVALID; }
    if (!(p->compactness > 0.0)) { set_error("compactness must be positive"); return OBIA_E_INVALID; }
    if (p->n_segments <= 0) { set_error("n_segments must be positive"); return OBIA_E_INVALID; }
    if (p->max_num_iter < 0) { set_error("max_num_iter must be >= 0"); return OBIA_E_INVALID; }
    for (int i = 0; i < 3; ++i) {
        if (!(p->sigma_zyx[i] >= 0.0)) { set_error("sigma must be >= 0"); return OBIA_E_INVALID; }
        if (!(p->spacing_zyx[i] > 0.0) || !(p->spacing_zyx[i] < 1.0e30)) { set_error("spacing must be positive and finite"); return OBIA_E_INVALID; }
    }
    return OBIA_OK;
}

// Whole-raster SLIC up to the pre-connectivity labels (device pointers).  On return b holds the plan.
int slic_single(obia_ctx *ctx, const float *img, int H, int W, int C, const uint8_t *mask,
                const obia_slic_params *p, SlicBatch &b, const ExternalSeeds *ext = nullptr, bool prepass_only = false,
                int prepass_iters = 0) {
    Arena &A = ctx->arena;
    slic_batch_settings(b, *p, C, p->normalize_bands, mask != nullptr);
    b.prepass_only = prepass_only && b.masked;
    b.prepass_iter = b.masked ? prepass_iters : 0;
    b.windows.assign(1, SrcWindow{0, 0, H, W, 0, 0, 0});
    OBIA_TRY(slic_batch_layout(b));
    b.d_windows = A.get<SrcWindow>(1);
    b.d_feat = A.get<float>(4 * (size_t)b.total_feat_f4);
    b.d_labels = A.get<int32_t>((size_t)b.total_pix);
    if (!b.d_windows || !b.d_feat || !b.d_labels) return OBIA_E_NOMEM;
    OBIA_HIP_TRY(hipMemcpyAsync(b.d_windows, b.windows.data(), sizeof(SrcWindow), hipMemcpyHostToDevice, ctx->stream));
    b.d_mask = const_cast<uint8_t *>(mask);
    if (b.col_lb) {
        b.d_fbox = A.get<float>((size_t)b.total_boxes * 2 * b.CP);
        if (!b.d_fbox) return OBIA_E_NOMEM;
    }
    OBIA_TRY(slic_prepare_features(ctx, b, img, W));
    std::vector<int> nseg(1, p->n_segments);
    OBIA_TRY(slic_plan_and_seed(ctx, b, nseg, nullptr, ext));
    if (b.probs[0].K <= 0) {
        set_error("mask is empty: nothing to segment");
        return OBIA_E_EMPTY;
    }
    const Arena::Mark sweeps_mk = A.mark();   // a repeat of the sweeps reuses their workspace
    OBIA_TRY(slic_run_sweeps(ctx, b));
    OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
    bool repeat = false;
    OBIA_TRY(slic_sweeps_settle(ctx, &repeat));
    if (repeat) {
        A.rewind(sweeps_mk);
        b.d_mask4 = nullptr;   // (the sweeps packed it above the mark)
        OBIA_TRY(slic_rerun_storing(ctx, b));
        OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
        OBIA_TRY(slic_sweeps_settle(ctx, nullptr));
    }
    return OBIA_OK;
}

}  // namespace

extern "C" {

static int check_seeds(const obia_slic_seeds *seeds, int H, int W, ExternalSeeds &ext) {
    if (!seeds) { set_error("null seeds"); return OBIA_E_INVALID; }
    if (!seeds->yx || seeds->n < 1) { set_error("seeds: need at least one (y, x) pair"); return OBIA_E_INVALID; }
    for (int i = 0; i < seeds->n; ++i) {
        const double y = seeds->yx[2 * (size_t)i], x = seeds->yx[2 * (size_t)i + 1];
        if (!(y >= 0.0 && y <= (double)(H - 1) && x >= 0.0 && x <= (double)(W - 1))) {
            set_error("seed %d = (%g, %g) lies outside the (%d, %d) raster", i, y, x, H, W);
            return OBIA_E_INVALID;
        }
    }
    double st = seeds->steps_zyx[0];
    if (seeds->steps_zyx[1] > st) st = seeds->steps_zyx[1];
    if (seeds->steps_zyx[2] > st) st = seeds->steps_zyx[2];
    if (!(st > 0.0) || !(st < 1e9)) { set_error("seeds: steps must be positive and finite"); return OBIA_E_INVALID; }
    ext.yx = seeds->yx; ext.n = seeds->n; ext.step = st;   // step = max(steps), slic_superpixels.py:288
    return OBIA_OK;
}

// The sweeps of one raster and whatever of their stages the caller asked for: the body of obia_slic_assign_only_f32_dev (labels_pre
// alone) and of obia_slic_stages_f32_dev.
static int slic_stages_impl(obia_ctx *ctx, const float *img, int H, int W, int C, const uint8_t *mask,
                            const obia_slic_params *params, const ExternalSeeds *ext, obia_slic_stages *st) {
    OBIA_TRY(check_slic_args(img, H, W, C, params));
    if (!st) { set_error("null output"); return OBIA_E_INVALID; }
    if (st->prepass_iters < 0) { set_error("prepass_iters must be >= 0"); return OBIA_E_INVALID; }
    if (st->centroids && params->max_num_iter < 1) { set_error("centroids: no sweep ran (max_num_iter = 0)"); return OBIA_E_INVALID; }
    SlicBatch b;
    OBIA_TRY(call_frame(ctx, FRAME_TOTAL, [&] {
        int rc = slic_single(ctx, img, H, W, C, mask, params, b, ext, st->prepass_only != 0, st->prepass_iters);
        if (rc == OBIA_OK && (st->seeds_yx || st->centroids) && b.probs[0].K > st->centroid_capacity) {
            set_error("%d centroids, room for %d", b.probs[0].K, st->centroid_capacity);
            rc = OBIA_E_INVALID;
        }
        if (rc == OBIA_OK && st->labels_pre) {
            hipError_t e = hipMemcpyAsync(st->labels_pre, b.d_labels, sizeof(int32_t) * (size_t)H * W, hipMemcpyDeviceToDevice, ctx->stream);
            if (e != hipSuccess) { set_error("copy failed: %s", hipGetErrorString(e)); rc = OBIA_E_HIP; }
        }
        if (rc == OBIA_OK && (st->features || st->seeds_yx || st->centroids))
            rc = slic_stage_outputs(ctx, b, st->features, st->seeds_yx, st->centroids);
        return rc;
    }));
    st->K = b.probs[0].K;
    st->step = (double)b.step[0];
    st->prescale = (double)b.prescale;
    st->fscale = b.fscale * (double)b.prescale;   // in units of the handed-out features
    return OBIA_OK;
}

static int slic_assign_only_impl(obia_ctx *ctx, const float *img, int H, int W, int C, const uint8_t *mask,
                                 const obia_slic_params *params, const ExternalSeeds *ext, int32_t *labels_pre_out,
                                 int *n_centroids_out) {
    if (!labels_pre_out) { set_error("null output"); return OBIA_E_INVALID; }
    obia_slic_stages st{};
    st.labels_pre = labels_pre_out;
    OBIA_TRY(slic_stages_impl(ctx, img, H, W, C, mask, params, ext, &st));
    if (n_centroids_out) *n_centroids_out = st.K;
    return OBIA_OK;
}

static int slic_full_impl(obia_ctx *ctx, const float *img, int H, int W, int C, const uint8_t *mask,
                          const obia_slic_params *params, const ExternalSeeds *ext, int32_t *labels_out, int *n_labels_out) {
    OBIA_TRY(check_slic_args(img, H, W, C, params));
    if (!labels_out) { set_error("null output"); return OBIA_E_INVALID; }
    SlicBatch b;
    int n_labels = 0;
    OBIA_TRY(call_frame(ctx, FRAME_TOTAL, [&]() -> int {
        OBIA_TRY(slic_single(ctx, img, H, W, C, mask, params, b, ext));
        if (params->enforce_connectivity) {
            const auto [min_size, max_size] = slic_cc_sizes(params->min_size_factor, params->max_size_factor, b.probs[0].n_valid, b.probs[0].K);
            return enforce_connectivity_dev(ctx, b.d_labels, H, W, min_size, max_size, params->start_label, labels_out, &n_labels);
        }
        hipError_t e = hipMemcpyAsync(labels_out, b.d_labels, sizeof(int32_t) * (size_t)H * W, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) { set_error("copy failed: %s", hipGetErrorString(e)); return OBIA_E_HIP; }
        n_labels = b.probs[0].K;
        return OBIA_OK;
    }));
    if (n_labels_out) *n_labels_out = n_labels;
    return OBIA_OK;
}

int obia_slic_assign_only_f32_dev(obia_ctx *ctx, const float *img, int H, int W, int C, const uint8_t *mask,
                                  const obia_slic_params *params, int32_t *labels_pre_out, int *n_centroids_out) {
    OBIA_TRY(enter(ctx));
    return slic_assign_only_impl(ctx, img, H, W, C, mask, params, nullptr, labels_pre_out, n_centroids_out);
}

int obia_slic_f32_dev(obia_ctx *ctx, const float *img, int H, int W, int C, const uint8_t *mask,
                      const obia_slic_params *params, int32_t *labels_out, int *n_labels_out) {
    OBIA_TRY(enter(ctx));
    return slic_full_impl(ctx, img, H, W, C, mask, params, nullptr, labels_out, n_labels_out);
}

int obia_slic_seeded_f32_dev(obia_ctx *ctx, const float *img, int H, int W, int C, const uint8_t *mask,
                             const obia_slic_params *params, const obia_slic_seeds *seeds, int stage,
                             int32_t *labels_out, int *n_out) {
    OBIA_TRY(enter(ctx));
    if (H <= 0 || W <= 0) { set_error("bad image shape"); return OBIA_E_INVALID; }
    ExternalSeeds ext{};
    OBIA_TRY(check_seeds(seeds, H, W, ext));
    if (stage == 1) return slic_assign_only_impl(ctx, img, H, W, C, mask, params, &ext, labels_out, n_out);
    if (stage != 0) { set_error("stage must be 0 (full) or 1 (labels before connectivity)"); return OBIA_E_INVALID; }
    return slic_full_impl(ctx, img, H, W, C, mask, params, &ext, labels_out, n_out);
}

int obia_slic_stages_f32_dev(obia_ctx *ctx, const float *img, int H, int W, int C, const uint8_t *mask,
                             const obia_slic_params *params, const obia_slic_seeds *seeds, obia_slic_stages *stages) {
    OBIA_TRY(enter(ctx));
    if (!seeds) return slic_stages_impl(ctx, img, H, W, C, mask, params, nullptr, stages);
    if (H <= 0 || W <= 0) { set_error("bad image shape"); return OBIA_E_INVALID; }
    ExternalSeeds ext{};
    OBIA_TRY(check_seeds(seeds, H, W, ext));
    return slic_stages_impl(ctx, img, H, W, C, mask, params, &ext, stages);
}

static int check_picks(const char *what, const int64_t *v, long long n) {
    if (v[0] < 0) { set_error("mask centroids: %s %lld is negative", what, (long long)v[0]); return OBIA_E_INVALID; }
    for (long long i = 1; i < n; ++i)
        if (v[i] <= v[i - 1]) {
            set_error("mask centroids: %ss must be strictly ascending (%lld follows %lld at %lld)", what, (long long)v[i], (long long)v[i - 1], i);
            return OBIA_E_INVALID;
        }
    return OBIA_OK;
}

int obia_mask_centroids_dev(obia_ctx *ctx, const uint8_t *mask, int H, int W, const int64_t *picks, int32_t n_picks,
                            const int64_t *dense_picks, int64_t n_dense, int iters, double *centroids_yx_out, double *steps_zyx_out) {
    OBIA_TRY(enter(ctx));
    if (!mask || !picks || !centroids_yx_out || !steps_zyx_out) { set_error("mask centroids: null pointer argument"); return OBIA_E_INVALID; }
    if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL) { set_error("mask centroids: bad mask shape (%d, %d)", H, W); return OBIA_E_INVALID; }
    if (n_picks < 1) { set_error("mask centroids: need at least one pick (got %d)", n_picks); return OBIA_E_INVALID; }
    if (dense_picks && (n_dense < 1 || n_dense > 0x7fffffffLL)) { set_error("mask centroids: bad dense pick count %lld", (long long)n_dense); return OBIA_E_INVALID; }
    if (iters < 0) { set_error("mask centroids: iters must be >= 0"); return OBIA_E_INVALID; }
    OBIA_TRY(check_picks("pick", picks, n_picks));
    if (dense_picks) OBIA_TRY(check_picks("dense pick", dense_picks, n_dense));
    return mask_centroids_dev(ctx, mask, H, W, picks, n_picks, dense_picks, dense_picks ? (long long)n_dense : 0, iters, centroids_yx_out,
                              steps_zyx_out);
}

int obia_slic_f32(obia_ctx *ctx, const float *img, int H, int W, int C, const uint8_t *mask,
                  const obia_slic_params *params, int32_t *labels_out, int *n_labels_out) {
    OBIA_TRY(enter(ctx));
    OBIA_TRY(check_slic_args(img, H, W, C, params));
    if (!labels_out) { set_error("null output"); return OBIA_E_INVALID; }
    const size_t npix = (size_t)H * W;
    Staging s(ctx);
    const float *d_img = s.in(img, npix * C);
    const uint8_t *d_mask = s.in(mask, npix);
    int32_t *d_lab = s.out<int32_t>(npix);
    s.run([&] { return obia_slic_f32_dev(ctx, d_img, H, W, C, d_mask, params, d_lab, n_labels_out); });
    s.fetch(labels_out, d_lab, npix);
    return s.finish();
}

int obia_enforce_connectivity_i32_dev(obia_ctx *ctx, const int32_t *labels_in, int H, int W, int min_size, int max_size,
                                      int start_label, int32_t *labels_out, int *n_labels_out) {
    OBIA_TRY(enter(ctx));
    if (!labels_in || !labels_out || H <= 0 || W <= 0) { set_error("bad arguments"); return OBIA_E_INVALID; }
    if (start_label != 0 && start_label != 1) { set_error("start_label should be 0 or 1."); return OBIA_E_INVALID; }
    int n = 0;
    OBIA_TRY(call_frame(ctx, FRAME_TIMING, [&] { return enforce_connectivity_dev(ctx, labels_in, H, W, min_size, max_size, start_label, labels_out, &n); }));
    if (n_labels_out) *n_labels_out = n;
    return OBIA_OK;
}

// ---- include/obia_testing.h: the connectivity stage on a batch, and the record of its last call
int obia_test_enforce_connectivity_batch_dev(obia_ctx *ctx, const int32_t *labels_in, const int64_t *problems, int n_problems,
                                             int start_label, int32_t *labels_out, int *n_labels_out) {
    OBIA_TRY(enter(ctx));
    if (!labels_in || !labels_out || !problems || n_problems < 1) { set_error("bad arguments"); return OBIA_E_INVALID; }
    if (n_problems > 65535) { set_error("a batch holds 65535 problems at the most (got %d)", n_problems); return OBIA_E_INVALID; }
    if (start_label != 0 && start_label != 1) { set_error("start_label should be 0 or 1."); return OBIA_E_INVALID; }
    std::vector<CcProblem> probs((size_t)n_problems);
    long long total = 0;
    for (int p = 0; p < n_problems; ++p) {
        const int64_t *r = problems + 4 * (size_t)p;
        if (r[0] <= 0 || r[1] <= 0 || r[0] > 0x7fffffffLL || r[1] > 0x7fffffffLL) { set_error("problem %d: bad shape (%lld, %lld)", p, (long long)r[0], (long long)r[1]); return OBIA_E_INVALID; }
        if (r[2] < INT32_MIN || r[2] > INT32_MAX || r[3] < INT32_MIN || r[3] > INT32_MAX) { set_error("problem %d: min_size / max_size out of range", p); return OBIA_E_INVALID; }
        probs[(size_t)p] = CcProblem{(int)r[0], (int)r[1], total, (int)r[2], r[3] > 0 ? (int)r[3] : 1};
        if (r[0] * r[1] > 0x7fffffffLL - total) { set_error("batches of 2^31 pixels or more are not supported"); return OBIA_E_INVALID; }
        total += r[0] * r[1];
    }
    int n = 0;
    OBIA_TRY(call_frame(ctx, FRAME_TIMING, [&] { return enforce_connectivity_batch(ctx, probs, labels_in, total, start_label, labels_out, &n, nullptr); }));
    if (n_labels_out) *n_labels_out = n;
    return OBIA_OK;
}

int obia_test_cc_report(obia_ctx *ctx, int64_t *out, int n) {
    if (!ctx) { set_error("null context"); return OBIA_E_INVALID; }
    if (!out || n < obia_ctx::CC_REPORT_FIELDS) { set_error("cc report: room for %d fields is needed", (int)obia_ctx::CC_REPORT_FIELDS); return OBIA_E_INVALID; }
    std::copy(ctx->cc_report, ctx->cc_report + obia_ctx::CC_REPORT_FIELDS, out);
    return OBIA_OK;
}

int obia_zonal_stats_f32_dev(obia_ctx *ctx, const float *raw, const int32_t *labels, int H, int W, int C,
                             const int32_t *bands, int n_bands, int n_labels, int start_label, int64_t *count_out,
                             double *mean_out, double *var_out, float *min_out, float *max_out) {
    OBIA_TRY(enter(ctx));
    if (!raw || !labels || !count_out || !mean_out || !var_out || !min_out || !max_out) { set_error("null pointer argument"); return OBIA_E_INVALID; }
    return call_frame(ctx, FRAME_TIMING, [&] {
        return zonal_stats_dev(ctx, raw, labels, H, W, C, bands, n_bands, n_labels, start_label, count_out, mean_out, var_out, min_out, max_out);
    });
}

int obia_zonal_stats_f32(obia_ctx *ctx, const float *raw, const int32_t *labels, int H, int W, int C,
                         const int32_t *bands, int n_bands, int n_labels, int start_label, int64_t *count_out,
                         double *mean_out, double *var_out, float *min_out, float *max_out) {
    OBIA_TRY(enter(ctx));
    if (!raw || !labels || H <= 0 || W <= 0 || C <= 0 || n_labels < 0) { set_error("bad arguments"); return OBIA_E_INVALID; }
    const size_t npix = (size_t)H * W;
    const int nb = bands ? n_bands : C;
    if (nb < 1 || nb > 16) { set_error("n_bands %d out of range (1..16)", nb); return OBIA_E_UNSUPPORTED; }
    const size_t nl = (size_t)(n_labels > 0 ? n_labels : 1), nlb = nl * nb;
    Staging s(ctx);
    const float *d_raw = s.in(raw, npix * C);
    const int32_t *d_lab = s.in(labels, npix);
    int64_t *d_cnt = s.out<int64_t>(nl);
    double *d_mean = s.out<double>(nlb), *d_var = s.out<double>(nlb);
    float *d_mn = s.out<float>(nlb), *d_mx = s.out<float>(nlb);
    s.run([&] { return obia_zonal_stats_f32_dev(ctx, d_raw, d_lab, H, W, C, bands, n_bands, n_labels, start_label, d_cnt, d_mean, d_var, d_mn, d_mx); });
    if (n_labels > 0) {
        s.fetch(count_out, d_cnt, nl);
        s.fetch(mean_out, d_mean, nlb);
        s.fetch(var_out, d_var, nlb);
        s.fetch(min_out, d_mn, nlb);
        s.fetch(max_out, d_mx, nlb);
    }
    return s.finish();
}

int obia_zonal_moments_f32_dev(obia_ctx *ctx, const float *raw, const int32_t *labels, int H, int W, int C,
                               const int32_t *bands, int n_bands, int n_labels, int start_label, const double *mean_dev,
                               double *skew_out, double *kurt_out, double *var_out) {
    OBIA_TRY(enter(ctx));
    if (!raw || !labels || !mean_dev || !skew_out || !kurt_out) { set_error("null pointer argument"); return OBIA_E_INVALID; }
    return call_frame(ctx, FRAME_TIMING, [&] {
        return zonal_moments_dev(ctx, raw, labels, H, W, C, bands, n_bands, n_labels, start_label, mean_dev, skew_out, kurt_out, var_out);
    });
}

int obia_zonal_moments_f32(obia_ctx *ctx, const float *raw, const int32_t *labels, int H, int W, int C,
                           const int32_t *bands, int n_bands, int n_labels, int start_label, double *skew_out,
                           double *kurt_out, double *var_out) {
    OBIA_TRY(enter(ctx));
    if (!raw || !labels || !skew_out || !kurt_out || H <= 0 || W <= 0 || C <= 0 || n_labels < 0) { set_error("bad arguments"); return OBIA_E_INVALID; }
    const size_t npix = (size_t)H * W;
    const int nb = bands ? n_bands : C;
    if (nb < 1 || nb > 16) { set_error("n_bands %d out of range (1..16)", nb); return OBIA_E_UNSUPPORTED; }
    const size_t nl = (size_t)(n_labels > 0 ? n_labels : 1), nlb = nl * nb;
    Staging s(ctx);
    const float *d_raw = s.in(raw, npix * C);
    const int32_t *d_lab = s.in(labels, npix);
    int64_t *d_cnt = s.out<int64_t>(nl);
    double *d_mean = s.out<double>(nlb), *d_var = s.out<double>(nlb), *d_skew = s.out<double>(nlb), *d_kurt = s.out<double>(nlb);
    float *d_mn = s.out<float>(nlb), *d_mx = s.out<float>(nlb);
    s.run([&] { return obia_zonal_stats_f32_dev(ctx, d_raw, d_lab, H, W, C, bands, n_bands, n_labels, start_label, d_cnt, d_mean, d_var, d_mn, d_mx); });
    s.run([&] { return obia_zonal_moments_f32_dev(ctx, d_raw, d_lab, H, W, C, bands, n_bands, n_labels, start_label, d_mean, d_skew, d_kurt, d_var); });
    if (n_labels > 0) {
        s.fetch(skew_out, d_skew, nlb);
        s.fetch(kurt_out, d_kurt, nlb);
        if (var_out) s.fetch(var_out, d_var, nlb);
    }
    return s.finish();
}

}  // extern "C"
