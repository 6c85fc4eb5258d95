// crowns.hip -- cost allocation (include/obia_crowns.h): the multi-source shortest-path distance over the pixel grid as a tiled
// Bellman-Ford, then the labels as an int32 minimum over the tight edges.  DESIGN.md 3.5p.
//
// One workgroup owns a tile of 32 x 32 pixels.  It stages the tile's distances and costs with a halo of one pixel in LDS, relaxes there
// until nothing in the tile changes, stores the pixels that decreased and counts itself in a device counter when any did.  The host
// repeats such rounds until a round leaves the counter at zero.  The rounds work IN PLACE: a halo pixel may or may not hold what its
// owner wrote in the same round.  Either value is an upper bound of the fixpoint and the values only ever decrease, so the result is
// the fixpoint whatever the schedule; a round in which nothing was stored has read nothing but final values and proves it.  Values
// that other workgroups write during a round are read and written as relaxed 64-bit (32-bit) atomic loads and stores, which do not
// tear.  There is no floating-point atomic; the integer ones (a minimum per seed, the counters) commute.
#include "common.hpp"
#include "../../include/obia_crowns.h"

#include <climits>
#include <cmath>

namespace obia {
namespace {

constexpr int CT = OBIA_CROWNS_TILE;                   // side of a tile
constexpr int CS = CT + 2;                             // ... and of what is staged: a halo of one pixel
constexpr int CPX = CT * CT / 256;                     // pixels of one lane: rows ty, ty + 8, ty + 16, ty + 24 of column tx
constexpr int NO_LABEL = INT_MAX;
static_assert(CT == 32 && CPX == 4, "256 lanes, lane -> (tid >> 5, tid & 31)");

struct Counters { int negative, bad_id, seeded, changed; };

// the eight neighbours: 0 .. 3 share an edge (the 4-connected ones), 4 .. 7 a corner
// (dy, dx) = (0, -1) (0, 1) (-1, 0) (1, 0) (-1, -1) (-1, 1) (1, -1) (1, 1); the loops over j are unrolled, so these fold
__device__ __forceinline__ constexpr int nb_dy(int j) { return (j == 2 || j == 4 || j == 5) ? -1 : (j == 3 || j >= 6) ? 1 : 0; }
__device__ __forceinline__ constexpr int nb_dx(int j) { return (j == 0 || j == 4 || j == 6) ? -1 : (j == 1 || j == 5 || j == 7) ? 1 : 0; }
__device__ __forceinline__ constexpr int nb_len(int j) { return j < 2 ? 0 : j < 4 ? 1 : 2; }   // horizontal, vertical, diagonal

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ double inf_d() { return __longlong_as_double(0x7FF0000000000000LL); }

__device__ __forceinline__ double load_d(const double *p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void store_d(double *p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool passable(const float *cost, const uint8_t *mask, long long i) {
    return finite_f(cost[i]) && (!mask || mask[i] != 0);
}

// the weight of the step between two pixels of costs cu and cv: this order, nothing contracted
__device__ __forceinline__ double edge_weight(double len, double weight, float cu, float cv) {
    return len * (1.0 + weight * (0.5 * ((double)cu + (double)cv)));
}

// D = +inf and no label everywhere; counts the negative costs at pixels the mask lets through
__global__ __launch_bounds__(256) void crowns_init_kernel(const float *__restrict__ cost, const uint8_t *__restrict__ mask, long long n,
                                                          double *__restrict__ dist, int *__restrict__ labels, Counters *cnt) {
    int neg = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        dist[i] = inf_d();
        labels[i] = NO_LABEL;
        neg += (cost[i] < 0.0f && passable(cost, mask, i)) ? 1 : 0;
    }
    if (neg) atomicAdd(&cnt->negative, neg);
}

__global__ __launch_bounds__(256) void crowns_seed_kernel(const float *__restrict__ cost, const uint8_t *__restrict__ mask, int H, int W,
                                                          const int *__restrict__ seed_rc, const int *__restrict__ seed_id, int n,
                                                          double *dist, int *labels, Counters *cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = seed_rc[2 * (long long)i], c = seed_rc[2 * (long long)i + 1], id = seed_id[i];
    if (id < 1 || id == NO_LABEL) { atomicAdd(&cnt->bad_id, 1); return; }
    if (r < 0 || r >= H || c < 0 || c >= W) return;
    const long long p = (long long)r * W + c;
    if (!passable(cost, mask, p)) return;
    dist[p] = 0.0;                                                           // (every seed of the pixel stores the same bits)
    atomicMin(&labels[p], id);
    atomicAdd(&cnt->seeded, 1);
}

// Stages cost and D of the tile and its halo.  A pixel outside the raster and a barrier get D = +inf, which is what keeps every step
// from them out of the minimum; a barrier's own D is never read from memory (it holds +inf there too).
template <bool FIXED>
__device__ __forceinline__ void stage_tile(const float *__restrict__ cost, const uint8_t *__restrict__ mask, const double *dist, int H,
                                           int W, int y0, int x0, double (*s_d)[CS], float (*s_c)[CS]) {
    for (int i = threadIdx.x; i < CS * CS; i += 256) {
        const int ly = i / CS, lx = i - ly * CS;
        const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
        double d = inf_d();
        float c = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const long long g = (long long)gy * W + gx;
            if (passable(cost, mask, g)) {
                c = cost[g];
                d = FIXED ? dist[g] : load_d(dist + g);
            }
        }
        s_d[ly][lx] = d;
        s_c[ly][lx] = c;
    }
}

template <int CONN>
__global__ __launch_bounds__(256) void crowns_relax_kernel(const float *__restrict__ cost, const uint8_t *__restrict__ mask, int H, int W,
                                                           int ntx, double weight, double len_h, double len_v, double len_d,
                                                           double limit, double *dist, Counters *cnt) {
    __shared__ double s_d[CS][CS];
    __shared__ float s_c[CS][CS];
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int by = blockIdx.x / ntx, bx = blockIdx.x - by * ntx;
    const int y0 = by * CT, x0 = bx * CT;
    stage_tile<false>(cost, mask, dist, H, W, y0, x0, s_d, s_c);
    __syncthreads();
    double first[CPX], now[CPX];
    bool open[CPX];
#pragma unroll
    for (int k = 0; k < CPX; ++k) {
        const int ly = ty + 8 * k + 1, lx = tx + 1;
        const int gy = y0 + ly - 1, gx = x0 + lx - 1;
        first[k] = now[k] = s_d[ly][lx];
        // a barrier of the interior was staged with +inf and stays there: it is never relaxed
        open[k] = gy < H && gx < W && passable(cost, mask, (long long)gy * W + gx);
    }
    const double len[3] = {len_h, len_v, len_d};
    bool tile_changed = false;
    for (;;) {
        int changed = 0;
        double next[CPX];
#pragma unroll
        for (int k = 0; k < CPX; ++k) {
            const int ly = ty + 8 * k + 1, lx = tx + 1;
            double best = now[k];
            if (open[k]) {
                const float cv = s_c[ly][lx];
#pragma unroll
                for (int j = 0; j < CONN; ++j) {
                    const double du = s_d[ly + nb_dy(j)][lx + nb_dx(j)];
                    if (du < inf_d()) {
                        const double cand = du + edge_weight(len[nb_len(j)], weight, s_c[ly + nb_dy(j)][lx + nb_dx(j)], cv);
                        if (cand < best && cand <= limit) best = cand;
                    }
                }
            }
            next[k] = best;
            changed |= best < now[k] ? 1 : 0;
        }
        if (!__syncthreads_or(changed)) break;                               // (a barrier: every lane has read what it needs)
        tile_changed = true;
#pragma unroll
        for (int k = 0; k < CPX; ++k)
            if (next[k] < now[k]) s_d[ty + 8 * k + 1][tx + 1] = now[k] = next[k];
        __syncthreads();
    }
    if (!tile_changed) return;
#pragma unroll
    for (int k = 0; k < CPX; ++k)
        if (now[k] < first[k]) store_d(dist + (long long)(y0 + ty + 8 * k) * W + (x0 + tx), now[k]);   // open[k]: inside the raster
    if (tid == 0) atomicAdd(&cnt->changed, 1);
}

// The label pass: D is final.  Which neighbours are tight is worked out once, as a bit per direction; the rounds move int32 labels only.
template <int CONN>
__global__ __launch_bounds__(256) void crowns_label_kernel(const float *__restrict__ cost, const uint8_t *__restrict__ mask,
                                                           const double *__restrict__ dist, int H, int W, int ntx, double weight,
                                                           double len_h, double len_v, double len_d, int *labels, Counters *cnt) {
    __shared__ double s_d[CS][CS];
    __shared__ float s_c[CS][CS];
    __shared__ int s_l[CS][CS];
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int by = blockIdx.x / ntx, bx = blockIdx.x - by * ntx;
    const int y0 = by * CT, x0 = bx * CT;
    stage_tile<true>(cost, mask, dist, H, W, y0, x0, s_d, s_c);
    for (int i = tid; i < CS * CS; i += 256) {
        const int ly = i / CS, lx = i - ly * CS;
        const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
        int l = NO_LABEL;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) l = __hip_atomic_load(labels + (long long)gy * W + gx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_l[ly][lx] = l;
    }
    __syncthreads();
    const double len[3] = {len_h, len_v, len_d};
    int first[CPX], now[CPX];
    unsigned tight[CPX];
#pragma unroll
    for (int k = 0; k < CPX; ++k) {
        const int ly = ty + 8 * k + 1, lx = tx + 1;
        first[k] = now[k] = s_l[ly][lx];
        tight[k] = 0;
        const double dv = s_d[ly][lx];                                       // +inf outside the raster, at barriers, where no seed reaches
        if (dv < inf_d()) {
            const float cv = s_c[ly][lx];
#pragma unroll
            for (int j = 0; j < CONN; ++j) {
                const double du = s_d[ly + nb_dy(j)][lx + nb_dx(j)];
                if (du < inf_d() &&
                    du + edge_weight(len[nb_len(j)], weight, s_c[ly + nb_dy(j)][lx + nb_dx(j)], cv) == dv)
                    tight[k] |= 1u << j;
            }
        }
    }
    bool tile_changed = false;
    for (;;) {
        int changed = 0;
        int next[CPX];
#pragma unroll
        for (int k = 0; k < CPX; ++k) {
            const int ly = ty + 8 * k + 1, lx = tx + 1;
            int best = now[k];
#pragma unroll
            for (int j = 0; j < CONN; ++j)
                if (tight[k] & (1u << j)) best = min(best, s_l[ly + nb_dy(j)][lx + nb_dx(j)]);
            next[k] = best;
            changed |= best < now[k] ? 1 : 0;
        }
        if (!__syncthreads_or(changed)) break;
        tile_changed = true;
#pragma unroll
        for (int k = 0; k < CPX; ++k)
            if (next[k] < now[k]) s_l[ty + 8 * k + 1][tx + 1] = now[k] = next[k];
        __syncthreads();
    }
    if (!tile_changed) return;
#pragma unroll
    for (int k = 0; k < CPX; ++k)
        if (now[k] < first[k])                                               // tight[k] != 0: a finite D, inside the raster
            __hip_atomic_store(labels + (long long)(y0 + ty + 8 * k) * W + (x0 + tx), now[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) atomicAdd(&cnt->changed, 1);
}

// no label -> 0
__global__ __launch_bounds__(256) void crowns_finish_kernel(int *__restrict__ labels, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        if (labels[i] == NO_LABEL) labels[i] = 0;
}

thread_local int64_t last_work[4] = {0, 0, 0, 0};

// Rounds of one pass until one leaves the counter of changed tiles at zero; rounds and the sum of the counters into out[0], out[1].
template <typename Launch> int run_rounds(obia_ctx *ctx, const char *what, long long npx, Counters *cnt, Launch &&launch, int64_t *out) {
    out[0] = out[1] = 0;
    for (;;) {
        if (out[0] > npx) {
            set_error("crowns: the %s pass did not settle within H * W + 1 = %lld rounds", what, npx + 1);
            return OBIA_E_INTERNAL;
        }
        OBIA_TRY(fill_async(ctx, &cnt->changed, 0, sizeof(int)));
        launch();
        OBIA_HIP_TRY(hipGetLastError());
        int changed = 0;
        OBIA_TRY(read_back(ctx, &changed, &cnt->changed, sizeof(int)));
        out[0] += 1;
        out[1] += changed;
        if (!changed) return OBIA_OK;
    }
}

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_crowns_allocate_dev(obia_ctx *ctx, const float *cost, const uint8_t *mask, int H, int W, const int32_t *seed_rc,
                             const int32_t *seed_id, int n, double weight, double len_h, double len_v, double len_d, int connectivity,
                             double max_dist, double *dist_out, int32_t *labels_out, int32_t *rounds_out) {
    OBIA_TRY(enter(ctx));
    // each output against the cost raster: the two outputs have never been compared with each other
    if (Buffers().out(dist_out).in(cost).lone(seed_rc).lone(seed_id).bad() || Buffers().out(labels_out).in(cost).bad()) {
        set_error("crowns: bad arguments (null, misaligned or overlapping buffers)");
        return OBIA_E_INVALID;
    }
    if (H <= 0 || W <= 0) { set_error("crowns: H and W must be positive, got %d x %d", H, W); return OBIA_E_INVALID; }
    if (n <= 0) { set_error("crowns: at least one seed is needed, got %d", n); return OBIA_E_INVALID; }
    if (connectivity != 4 && connectivity != 8) { set_error("crowns: connectivity must be 4 or 8, got %d", connectivity); return OBIA_E_INVALID; }
    if (!(weight >= 0.0) || !std::isfinite(weight)) { set_error("crowns: weight must be finite and not negative, got %g", weight); return OBIA_E_INVALID; }
    if (!(len_h > 0.0) || !(len_v > 0.0) || !(len_d > 0.0) || !std::isfinite(len_h) || !std::isfinite(len_v) || !std::isfinite(len_d)) {
        set_error("crowns: the step lengths must be finite and positive, got (%g, %g, %g)", len_h, len_v, len_d);
        return OBIA_E_INVALID;
    }
    if (std::isnan(max_dist)) { set_error("crowns: max_dist is NaN"); return OBIA_E_INVALID; }
    const long long npx = (long long)H * W;
    if (npx > 0x7fffffffLL) { set_error("crowns: %d x %d is 2^31 pixels or more", H, W); return OBIA_E_UNSUPPORTED; }
    const double limit = max_dist < 0.0 ? INFINITY : max_dist;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        Counters *cnt = ctx->arena.get<Counters>(1);
        if (!cnt) return OBIA_E_NOMEM;
        OBIA_TRY(fill_async(ctx, cnt, 0, sizeof(Counters)));
        hipLaunchKernelGGL(crowns_init_kernel, dim3(flat_grid(npx)), dim3(256), 0, ctx->stream, cost, mask, npx, dist_out, labels_out, cnt);
        hipLaunchKernelGGL(crowns_seed_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, cost, mask, H, W, seed_rc, seed_id, n, dist_out,
                           labels_out, cnt);
        OBIA_HIP_TRY(hipGetLastError());
        Counters h;
        OBIA_TRY(read_back(ctx, &h, cnt, sizeof(Counters)));
        if (h.negative) { set_error("crowns: negative cost at %d passable pixels", h.negative); return OBIA_E_INVALID; }
        if (h.bad_id) { set_error("crowns: %d seed ids outside 1 .. 2^31 - 2", h.bad_id); return OBIA_E_INVALID; }
        if (!h.seeded) { set_error("crowns: no seed lies on a passable pixel of the raster"); return OBIA_E_EMPTY; }
        const int ntx = cdiv(W, CT);
        const dim3 grid((unsigned)((long long)ntx * cdiv(H, CT)));           // at most 2^31 / 1024 tiles
        int64_t work[4];
        OBIA_TRY(run_rounds(ctx, "distance", npx, cnt, [&] {
            if (connectivity == 8)
                hipLaunchKernelGGL(crowns_relax_kernel<8>, grid, dim3(256), 0, ctx->stream, cost, mask, H, W, ntx, weight, len_h, len_v, len_d,
                                   limit, dist_out, cnt);
            else
                hipLaunchKernelGGL(crowns_relax_kernel<4>, grid, dim3(256), 0, ctx->stream, cost, mask, H, W, ntx, weight, len_h, len_v, len_d,
                                   limit, dist_out, cnt);
        }, work));
        OBIA_TRY(run_rounds(ctx, "label", npx, cnt, [&] {
            if (connectivity == 8)
                hipLaunchKernelGGL(crowns_label_kernel<8>, grid, dim3(256), 0, ctx->stream, cost, mask, (const double *)dist_out, H, W, ntx,
                                   weight, len_h, len_v, len_d, labels_out, cnt);
            else
                hipLaunchKernelGGL(crowns_label_kernel<4>, grid, dim3(256), 0, ctx->stream, cost, mask, (const double *)dist_out, H, W, ntx,
                                   weight, len_h, len_v, len_d, labels_out, cnt);
        }, work + 2));
        hipLaunchKernelGGL(crowns_finish_kernel, dim3(flat_grid(npx)), dim3(256), 0, ctx->stream, labels_out, npx);
        OBIA_HIP_TRY(hipGetLastError());
        if (rounds_out) { rounds_out[0] = (int32_t)work[0]; rounds_out[1] = (int32_t)work[2]; }
        last_work[0] = work[0]; last_work[1] = work[2]; last_work[2] = work[1]; last_work[3] = work[3];
        return OBIA_OK;
    });
}

int obia_crowns_last_work(obia_ctx *ctx, int64_t *work_out) {
    OBIA_TRY(enter(ctx));
    if (!work_out) { set_error("crowns: work_out is null"); return OBIA_E_INVALID; }
    for (int i = 0; i < 4; ++i) work_out[i] = last_work[i];
    return OBIA_OK;
}

}  // extern "C"
