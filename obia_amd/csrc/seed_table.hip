// seed_table.hip -- the table options of the canonical seeds (include/obia_seed_table.h): heights from a raster, stage 1, the
// per-cluster passes and the suppression inside a cluster.  DESIGN.md 3.5q.
//
// A ball is searched without a tree.  The caller hands the table over sorted by the key of a uniform grid whose cell side is not
// smaller than the largest radius, so a ball lies within the 3 x 3 cells around its centre; the three cells of one grid row are one
// run of the sorted keys, found by binary search.  One lane owns one seed and walks the three runs.  Everything a lane makes of a ball
// is a count, a minimum, a maximum or an "exists", so the order in which it meets the members does not matter, there is no atomic on a
// floating-point value, and two runs agree bit for bit.  Nothing is exchanged between workgroups inside a launch: a round of stage 1
// reads the states the round before it wrote and writes its own into a second buffer.
#include "common.hpp"
#include "grid_cells.hpp"
#include "../../include/obia_seed_table.h"

#include <climits>
#include <cmath>

namespace obia {
namespace {

enum : unsigned char { ST_UNDECIDED = 0, ST_FIRED = 1, ST_NOT = 2 };

// j in the ball of radius r around i: float64, this order, nothing contracted (-ffp-contract=off)
__device__ __forceinline__ bool in_ball(double xi, double yi, double xj, double yj, double r) {
    const double dx = xi - xj, dy = yi - yj;
    return dx * dx + dy * dy <= r * r;
}

__global__ __launch_bounds__(256) void seedtab_cells_kernel(const double *__restrict__ xs, const double *__restrict__ ys, int n, double side,
                                                            int *__restrict__ cx, int *__restrict__ cy) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const double lim = 1073741824.0;
    cx[k] = (int)fmin(fmax(floor(xs[k] / side), -lim), lim);
    cy[k] = (int)fmin(fmax(floor(ys[k] / side), -lim), lim);
}

struct Inv6 { double a, b, c, d, e, f; };

__global__ __launch_bounds__(256) void seedtab_sample_kernel(const double *__restrict__ xs, const double *__restrict__ ys, int n,
                                                             const float *__restrict__ chm, int H, int W, Inv6 t, float *__restrict__ h_out,
                                                             uint8_t *__restrict__ valid_out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const double x = xs[k], y = ys[k];
    const double fc = floor((t.a * x + t.b * y) + t.c), fr = floor((t.d * x + t.e * y) + t.f);
    float v = __uint_as_float(0x7FC00000u);
    if (fc >= 0.0 && fc < (double)W && fr >= 0.0 && fr < (double)H) v = chm[(long long)fr * W + (long long)fc];
    const bool ok = v == v;
    h_out[k] = ok ? v : __uint_as_float(0x7FC00000u);
    valid_out[k] = ok ? 1 : 0;
}

// eps and eligible(i) of every seed; an ineligible seed is decided at once
__global__ __launch_bounds__(256) void seedtab_eligible_kernel(const double *__restrict__ xs, const double *__restrict__ ys,
                                                               const float *__restrict__ hs, const long long *__restrict__ skey, int n,
                                                               long long ncx, float eps_scale, float min_eps, float max_eps, int use_z,
                                                               float z_thresh, int min_samples, double *__restrict__ eps_out,
                                                               uint8_t *__restrict__ state_out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const float h = hs[k];
    const double eps = (double)fminf(fmaxf(eps_scale * h, min_eps), max_eps);
    const double x = xs[k], y = ys[k];
    int count = 0;
    float mn = h, mx = h;
    for_cells(skey, n, skey[k], ncx, [&](int q) {
        if (in_ball(x, y, xs[q], ys[q], eps)) {
            const float g = hs[q];
            count += 1;
            mn = fminf(mn, g);
            mx = fmaxf(mx, g);
        }
    });
    const bool eligible = count >= min_samples && !(use_z && (mx - mn) > z_thresh);
    eps_out[k] = eps;
    state_out[k] = eligible ? ST_UNDECIDED : ST_NOT;
}

// One round: an undecided seed with a fired earlier coverer is not fired; one whose eligible earlier coverers are all decided, none
// of them fired, is fired; the others wait and are counted.
__global__ __launch_bounds__(256) void seedtab_round_kernel(const double *__restrict__ xs, const double *__restrict__ ys,
                                                            const double *__restrict__ eps, const int *__restrict__ orig,
                                                            const long long *__restrict__ skey, int n, long long ncx,
                                                            const uint8_t *__restrict__ state_in, uint8_t *__restrict__ state_out,
                                                            int *remaining) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    bool waits = false;
    if (k < n) {
        unsigned char s = state_in[k];
        if (s == ST_UNDECIDED) {
            const double x = xs[k], y = ys[k];
            const int me = orig[k];
            bool covered = false, pending = false;
            for_cells(skey, n, skey[k], ncx, [&](int q) {
                const unsigned char sq = state_in[q];
                if (sq != ST_NOT && orig[q] < me && in_ball(xs[q], ys[q], x, y, eps[q])) {
                    covered |= sq == ST_FIRED;
                    pending |= sq == ST_UNDECIDED;
                }
            });
            s = covered ? ST_NOT : pending ? ST_UNDECIDED : ST_FIRED;
            waits = s == ST_UNDECIDED;
        }
        state_out[k] = s;
    }
    const unsigned long long b = __ballot(waits);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(remaining, __popcll(b));
}

__global__ __launch_bounds__(256) void seedtab_owner_kernel(const double *__restrict__ xs, const double *__restrict__ ys,
                                                            const double *__restrict__ eps, const int *__restrict__ orig,
                                                            const long long *__restrict__ skey, int n, long long ncx,
                                                            const uint8_t *__restrict__ state, uint8_t *__restrict__ fired_out,
                                                            int *__restrict__ owner_out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const double x = xs[k], y = ys[k];
    int owner = -1;
    for_cells(skey, n, skey[k], ncx, [&](int q) {
        if (state[q] == ST_FIRED && in_ball(xs[q], ys[q], x, y, eps[q])) owner = max(owner, orig[q]);
    });
    fired_out[k] = state[k] == ST_FIRED ? 1 : 0;
    owner_out[k] = owner;
}

// rank and size of the run of equal cluster ids a row lies in, and the side of the run's median it is on
__global__ __launch_bounds__(256) void seedtab_segments_kernel(const int *__restrict__ cl, const float *__restrict__ hs, int n, int use_dz,
                                                               float dz, int *__restrict__ rank_out, int *__restrict__ size_out,
                                                               uint8_t *__restrict__ part_out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int c = cl[k];
    int lo = 0, hi = k;                                  // first row of the run: the first with cl >= c, it is <= k
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cl[mid] < c) lo = mid + 1; else hi = mid;
    }
    const int start = lo;
    lo = k; hi = n;                                      // one past its last row: the first with cl > c, it is > k
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cl[mid] <= c) lo = mid + 1; else hi = mid;
    }
    const int end = lo, m = end - start;
    unsigned char part = 0;
    if (use_dz && (hs[start] - hs[end - 1]) > dz) {      // descending: the first is the maximum, the last the minimum
        // ascending rank t is row end - 1 - t
        const float med = (m & 1) ? hs[end - 1 - m / 2]
                                  : (hs[end - 1 - m / 2] + hs[end - m / 2]) / 2.0f;   // in float32, as pandas takes the mean
        part = hs[k] > med ? 1 : 0;
    }
    rank_out[k] = k - start;
    size_out[k] = m;
    part_out[k] = part;
}

__global__ __launch_bounds__(256) void seedtab_nms_kernel(const double *__restrict__ xs, const double *__restrict__ ys,
                                                          const float *__restrict__ hs, const int *__restrict__ cl,
                                                          const int *__restrict__ pos, const long long *__restrict__ skey, int n,
                                                          long long ncx, double base, double scale, uint8_t *__restrict__ keep_out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const double x = xs[k], y = ys[k];
    const int c = cl[k], p = pos[k];
    bool cleared = false;
    for_cells(skey, n, skey[k], ncx, [&](int q) {
        if (cl[q] == c && pos[q] > p) {
            const double v = scale * (double)hs[q];
            cleared |= in_ball(xs[q], ys[q], x, y, v > base ? v : base);
        }
    });
    keep_out[k] = cleared ? 0 : 1;
}

thread_local int64_t last_work[2] = {0, 0};

int check_grid(const Refusal &refuse, int64_t n, int64_t ncx) {
    OBIA_TRY(refuse.n(n));
    if (ncx < 3) { set_error("seed table: %s: ncx must be at least 3, got %lld", refuse.what, (long long)ncx); return OBIA_E_INVALID; }
    return OBIA_OK;
}

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_seedtab_cells_dev(obia_ctx *ctx, const double *xs, const double *ys, int64_t n, double side, int32_t *cx_out, int32_t *cy_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"seed table", "cells"};
    if (Buffers().out(cx_out).out(cy_out).lone(xs).lone(ys).bad()) return refuse.buffers();
    OBIA_TRY(refuse.n(n));
    if (!(side > 0.0)) { set_error("seed table: cells: the cell side must be positive, got %g", side); return OBIA_E_INVALID; }
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(seedtab_cells_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, xs, ys, (int)n, side, cx_out, cy_out);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_seedtab_sample_dev(obia_ctx *ctx, const double *xs, const double *ys, int64_t n, const float *chm, int H, int W,
                            const double *inv6, float *height_out, uint8_t *valid_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"seed table", "sample"};
    if (!inv6 || Buffers().out(height_out).in(chm).lone(xs).lone(ys).lone(valid_out).bad()) return refuse.buffers();
    OBIA_TRY(refuse.n(n));
    if (H <= 0 || W <= 0) { set_error("seed table: sample: H and W must be positive, got %d x %d", H, W); return OBIA_E_INVALID; }
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(inv6[i])) { set_error("seed table: sample: the inverse geotransform is not finite"); return OBIA_E_INVALID; }
    const Inv6 t{inv6[0], inv6[1], inv6[2], inv6[3], inv6[4], inv6[5]};
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(seedtab_sample_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, xs, ys, (int)n, chm, H, W, t, height_out,
                           valid_out);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_seedtab_stage1_dev(obia_ctx *ctx, const double *xs, const double *ys, const float *hs, const int32_t *orig, const int64_t *key,
                            int64_t n, int64_t ncx, float eps_scale, float min_eps, float max_eps, float z_thresh, int min_samples,
                            uint8_t *fired_out, int32_t *owner_out, int32_t *rounds_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"seed table", "stage 1"};
    if (Buffers().out(owner_out).in(orig).lone(xs).lone(ys).lone(hs).lone(key).lone(fired_out).bad()) return refuse.buffers();
    OBIA_TRY(check_grid(refuse, n, ncx));
    if (!(min_eps >= 0.0f) || !(max_eps >= min_eps) || !std::isfinite(eps_scale) || std::isnan(z_thresh)) {
        set_error("seed table: stage 1: needs 0 <= min_eps <= max_eps, a finite eps_scale and a z_thresh that is not NaN, got (%g, %g, %g, %g)",
                  (double)min_eps, (double)max_eps, (double)eps_scale, (double)z_thresh);
        return OBIA_E_INVALID;
    }
    if (min_samples < 1) { set_error("seed table: stage 1: min_samples must be at least 1, got %d", min_samples); return OBIA_E_INVALID; }
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        const int N = (int)n;
        double *eps = ctx->arena.get<double>(n);
        int *remaining = ctx->arena.get<int>(4);
        uint8_t *state[2] = {ctx->arena.get<uint8_t>(n), ctx->arena.get<uint8_t>(n)};
        if (!eps || !remaining || !state[0] || !state[1]) return OBIA_E_NOMEM;
        const dim3 grid(cdiv(n, 256)), block(256);
        const long long *skey = reinterpret_cast<const long long *>(key);
        hipLaunchKernelGGL(seedtab_eligible_kernel, grid, block, 0, ctx->stream, xs, ys, hs, skey, N, (long long)ncx, eps_scale, min_eps,
                           max_eps, z_thresh >= 0.0f ? 1 : 0, z_thresh, min_samples, eps, state[0]);
        OBIA_HIP_TRY(hipGetLastError());
        int64_t rounds = 0;
        int cur = 0;
        for (;;) {
            if (rounds >= n) {
                set_error("seed table: stage 1 did not settle within n = %lld rounds", (long long)n);
                return OBIA_E_INTERNAL;
            }
            OBIA_TRY(fill_async(ctx, remaining, 0, 4 * sizeof(int)));
            hipLaunchKernelGGL(seedtab_round_kernel, grid, block, 0, ctx->stream, xs, ys, (const double *)eps, orig, skey, N, (long long)ncx,
                               (const uint8_t *)state[cur], state[cur ^ 1], remaining);
            OBIA_HIP_TRY(hipGetLastError());
            int left = 0;
            OBIA_TRY(read_back(ctx, &left, remaining, sizeof(int)));
            cur ^= 1;
            rounds += 1;
            if (!left) break;
        }
        hipLaunchKernelGGL(seedtab_owner_kernel, grid, block, 0, ctx->stream, xs, ys, (const double *)eps, orig, skey, N, (long long)ncx,
                           (const uint8_t *)state[cur], fired_out, owner_out);
        OBIA_HIP_TRY(hipGetLastError());
        if (rounds_out) *rounds_out = (int32_t)rounds;
        last_work[0] = rounds;
        last_work[1] = n;
        return OBIA_OK;
    });
}

int obia_seedtab_last_work(obia_ctx *ctx, int64_t *work_out) {
    OBIA_TRY(enter(ctx));
    if (!work_out) { set_error("seed table: work_out is null"); return OBIA_E_INVALID; }
    work_out[0] = last_work[0];
    work_out[1] = last_work[1];
    return OBIA_OK;
}

int obia_seedtab_segments_dev(obia_ctx *ctx, const int32_t *cluster, const float *heights, int64_t n, float dz_merge, int32_t *rank_out,
                              int32_t *size_out, uint8_t *part_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"seed table", "segments"};
    if (Buffers().out(rank_out).out(size_out).in(cluster).lone(heights).lone(part_out).bad()) return refuse.buffers();
    OBIA_TRY(refuse.n(n));
    if (std::isnan(dz_merge)) { set_error("seed table: segments: dz_merge is NaN"); return OBIA_E_INVALID; }
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(seedtab_segments_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, cluster, heights, (int)n,
                           dz_merge > 0.0f ? 1 : 0, dz_merge, rank_out, size_out, part_out);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_seedtab_nms_dev(obia_ctx *ctx, const double *xs, const double *ys, const float *hs, const int32_t *cluster, const int32_t *pos,
                         const int64_t *key, int64_t n, int64_t ncx, double base, double scale, uint8_t *keep_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"seed table", "nms"};
    if (Buffers().lone(xs).lone(ys).lone(hs).lone(cluster).lone(pos).lone(key).lone(keep_out).bad()) return refuse.buffers();
    OBIA_TRY(check_grid(refuse, n, ncx));
    if (std::isnan(base) || std::isnan(scale)) { set_error("seed table: nms: nms_base or nms_scale is NaN"); return OBIA_E_INVALID; }
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(seedtab_nms_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, xs, ys, hs, cluster, pos,
                           reinterpret_cast<const long long *>(key), (int)n, (long long)ncx, base, scale, keep_out);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

}  // extern "C"
