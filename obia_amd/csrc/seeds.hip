// seeds.hip -- the seed points of obia/utils/seeds.py on gfx950.
//   peaks : scipy.ndimage.gaussian_filter (float32 plane, mode "reflect"), a (2d+1)^2 maximum filter, the threshold, and
//           the surviving pixels as a row-major list (np.where order) with their smoothed and raw values
//   pairs : D(i, j) of _build_distance_matrix (seeds.py:148-163), never stored: one kernel links every pair with
//           D <= eps in a lock-free union-find (DBSCAN(min_samples=1, metric="precomputed") = connected components numbered
//           by smallest member), another selects min / median / max of the upper triangle by radix passes over the keys
// Every stage restates the reference's arithmetic operation for operation (the library is built with -ffp-contract=off).
// Deviation: a NaN never wins the maximum filter and a NaN pixel is never a peak (scipy's answer near a NaN depends on the side
// the NaN is on); DESIGN.md 5.
#include "slic.hpp"
#include "wave_ops.hpp"

#include <algorithm>
#include <cmath>

namespace obia {
namespace {

// scipy's "reflect" (d c b a | a b c d | d c b a), any distance outside
__device__ __forceinline__ int reflect_idx(int i, int n) {
    const int per = 2 * n;
    i %= per;
    if (i < 0) i += per;
    return i >= n ? per - 1 - i : i;
}

// ---------------------------------------------------------------------------------------------------------------- gauss
// One axis pass of scipy.ndimage.correlate1d with symmetric weights on one float32 plane (gauss_axis_kernel of slic.hip for a
// single plane): the line is read as double, tmp = line[i] * w[0]; for j = r .. 1: tmp += (line[i - j] + line[i + j]) * w[j];
// stored as float32.  AXIS 0 runs along the rows (y), AXIS 1 along the columns (x).
template <int AXIS>
__global__ __launch_bounds__(256) void seeds_gauss_kernel(const float *__restrict__ in, float *__restrict__ out, int H, int W,
                                                          const double *__restrict__ w, int r) {
    const long long n_el = (long long)H * W;
    const int n = AXIS == 0 ? H : W;
    const long long stride = AXIS == 0 ? (long long)W : 1LL;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_el; i += (long long)gridDim.x * 256) {
        const int y = (int)(i / W), x = (int)(i - (long long)y * W);
        const int pos = AXIS == 0 ? y : x;
        const float *line = in + (i - (long long)pos * stride);
        double tmp = (double)in[i] * w[0];
        for (int j = r; j >= 1; --j) {
            const int lo = reflect_idx(pos - j, n), hi = reflect_idx(pos + j, n);
            tmp += ((double)line[(long long)lo * stride] + (double)line[(long long)hi * stride]) * w[j];
        }
        out[i] = (float)tmp;
    }
}

// ------------------------------------------------------------------------------------------------------- maximum filter
// A 64 x 16 tile and its d-pixel halo (reflect) in LDS, NaN staged as -inf; row maxima over 2d + 1 taps, then column maxima;
// flag = g is not NaN && g == max && g >= threshold.
constexpr int MX_TW = grids::SEEDS_FLAG_TW, MX_TH = grids::SEEDS_FLAG_TH, MX_MAXD = 32;
constexpr int CHUNK = 4096;                   // pixels of one compaction block: 256 lanes x 16 flag bytes

__global__ __launch_bounds__(256) void seeds_flag_kernel(const float *__restrict__ g, int H, int W, int d, float thr,
                                                         uint8_t *__restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int LW = MX_TW + 2 * d, LH = MX_TH + 2 * d;
    float *tile = sm;                         // [LH][LW]
    float *rmax = sm + LH * LW;               // [LH][MX_TW]
    const int x0 = blockIdx.x * MX_TW;
    const int tx = threadIdx.x & 63;
    for (int by = blockIdx.y; by * MX_TH < H; by += gridDim.y) {
        const int y0 = by * MX_TH;
        __syncthreads();
        for (int i = threadIdx.x; i < LH * LW; i += 256) {
            const int ly = i / LW, lx = i - ly * LW;
            const int gy = reflect_idx(y0 - d + ly, H), gx = reflect_idx(x0 - d + lx, W);
            const float v = g[(long long)gy * W + gx];
            tile[i] = (v != v) ? -INFINITY : v;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < LH * MX_TW; i += 256) {
            const float *p = tile + (i >> 6) * LW + (i & 63);
            float m = p[0];
            for (int k = 1; k <= 2 * d; ++k) m = fmaxf(m, p[k]);
            rmax[i] = m;
        }
        __syncthreads();
        const int x = x0 + tx;
        for (int r = threadIdx.x >> 6; r < MX_TH; r += 4) {
            const int y = y0 + r;
            if (y >= H || x >= W) continue;
            float m = rmax[r * MX_TW + tx];
            for (int k = 1; k <= 2 * d; ++k) m = fmaxf(m, rmax[(r + k) * MX_TW + tx]);
            const float v = g[(long long)y * W + x];
            flags[(long long)y * W + x] = (v == v && v == m && v >= thr) ? 1 : 0;
        }
    }
}

// ----------------------------------------------------------------------------------------------------------- compaction
// flags hold 0 / 1 bytes, zero past the last pixel up to a multiple of CHUNK; a lane owns 16 consecutive pixels
__device__ __forceinline__ int flags16(const uint8_t *flags, long long chunk, uint4 &q) {
    q = *reinterpret_cast<const uint4 *>(flags + chunk * CHUNK + threadIdx.x * 16);
    return __popc(q.x) + __popc(q.y) + __popc(q.z) + __popc(q.w);
}

__global__ __launch_bounds__(256) void seeds_count_kernel(const uint8_t *__restrict__ flags, int *__restrict__ counts) {
    uint4 q;
    const int total = block_sum<256>(flags16(flags, blockIdx.x, q));
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// exclusive scan of m ints by one workgroup: out[0 .. m), out[m] = the sum
__global__ __launch_bounds__(1024) void seeds_scan_kernel(const int *__restrict__ in, int *__restrict__ out, int m) {
    workgroup_exclusive_scan<1024>(in, out, m, out + m);
}

__global__ __launch_bounds__(256) void seeds_scatter_kernel(const uint8_t *__restrict__ flags, const int *__restrict__ offsets,
                                                            const float *__restrict__ smooth, const float *__restrict__ raw, int W,
                                                            int32_t *__restrict__ rows, int32_t *__restrict__ cols,
                                                            float *__restrict__ gval, float *__restrict__ rval) {
    uint4 q;
    int total;
    const int c = flags16(flags, blockIdx.x, q);
    int o = offsets[blockIdx.x] + block_exclusive_scan<256>(c, total);
    if (c == 0) return;
    const uint32_t wds[4] = {q.x, q.y, q.z, q.w};
    const long long base = (long long)blockIdx.x * CHUNK + threadIdx.x * 16;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if ((wds[k >> 2] >> (8 * (k & 3))) & 0xFFu) {
            const long long i = base + k;
            const int y = (int)(i / W);
            rows[o] = y;
            cols[o] = (int)(i - (long long)y * W);
            gval[o] = smooth[i];
            rval[o] = raw[i];
            ++o;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- pairs
constexpr int PT = grids::SEEDS_PAIR_TILE;    // a pair tile is PT x PT seeds
constexpr int PAIR_MAX_SAMPLES = 128;         // NumPy's pairwise sum is restated up to its 128-element block

struct PairArgs {
    const double *xs, *ys;
    const float *cost;
    const double *ts;                         // interior float32 values of np.linspace(0, 1, samples + 2), as doubles
    int n, H, W, samples;
    double inv[6];                            // col = inv[0] * x + inv[1] * y + inv[2];  row = inv[3] * x + inv[4] * y + inv[5]
    double xy_thresh;
    float weight, eps;
    int weight_zero;                          // the caller's weight == 0 (tested on the double)
    int prune;                                // weight >= 0 and min(cost) >= 0: D >= xy_dist, so float32(xy_dist) > eps cannot link
};

// rows.round().astype(int) clipped to [0, n - 1]: round half to even; NaN and values past int64 become INT64_MIN on the
// reference's platform, i.e. 0 after the clip
__device__ __forceinline__ int round_clip(double v, int n) {
    const double r = __builtin_rint(v);
    if (!(__builtin_fabs(r) < 9.2e18) || r < 0.0) return 0;
    return r > (double)(n - 1) ? n - 1 : (int)r;
}

__device__ __forceinline__ float cost_tap(const PairArgs &P, double xi, double yi, double dx, double dy, int k) {
    const double t = P.ts[k];
    const double x = xi + t * dx, y = yi + t * dy;
    const double col = (x * P.inv[0] + y * P.inv[1]) + P.inv[2];
    const double row = (x * P.inv[3] + y * P.inv[4]) + P.inv[5];
    return P.cost[(long long)round_clip(row, P.H) * P.W + round_clip(col, P.W)];
}

__device__ __forceinline__ double pair_xy(double xi, double yi, double xj, double yj) {
    const double dx = xj - xi, dy = yj - yi;
    return __builtin_sqrt(dx * dx + dy * dy);
}

// D(i, j), i < j, as the reference writes it into its float32 matrix
__device__ __forceinline__ float pair_dist(const PairArgs &P, double xi, double yi, double xj, double yj) {
    const double dx = xj - xi, dy = yj - yi;
    const double xy = __builtin_sqrt(dx * dx + dy * dy);
    if (xy == 0.0) return 0.0f;
    if (xy <= P.xy_thresh || P.weight_zero) return (float)xy;
    const int S = P.samples;
    float res;
    if (S < 8) {                              // float32 np.mean: NumPy's pairwise sum
        res = 0.0f;
        for (int k = 0; k < S; ++k) res += cost_tap(P, xi, yi, dx, dy, k);
    } else {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = cost_tap(P, xi, yi, dx, dy, j);
        int k = 8;
        for (; k < S - (S % 8); k += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += cost_tap(P, xi, yi, dx, dy, k + j);
        }
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; k < S; ++k) res += cost_tap(P, xi, yi, dx, dy, k);
    }
    const float mean = res / (float)S;
    return (float)xy * (1.0f + P.weight * mean);
}

// tile pair t of the upper triangle of nt x nt tiles, rows first: row bi holds the tiles (bi, bi) .. (bi, nt - 1)
__device__ __forceinline__ long long tile_row_off(long long k, long long nt) { return k * nt - k * (k - 1) / 2; }
__device__ __forceinline__ void tile_of(long long t, int nt, int &bi, int &bj) {
    const double b = 2.0 * (double)nt + 1.0;
    long long i = (long long)((b - __builtin_sqrt(b * b - 8.0 * (double)t)) * 0.5);
    i = i < 0 ? 0 : (i > nt - 1 ? nt - 1 : i);
    while (i > 0 && tile_row_off(i, nt) > t) --i;
    while (i + 1 < nt && tile_row_off(i + 1, nt) <= t) ++i;
    bi = (int)i;
    bj = (int)(i + (t - tile_row_off(i, nt)));
}

// Walks the upper triangle: a workgroup takes tile pairs in a grid stride, stages the 2 x PT seed positions in LDS and hands
// every pair i < j of the tile to `f(i, j, xi, yi, xj, yj)`.  `skip_far`: leave out tile pairs whose bounding boxes are further apart
// than eps along one axis (every pair of such a tile has float32(xy_dist) > eps).
template <typename F> __device__ __forceinline__ void walk_pairs(const PairArgs &P, bool skip_far, F f) {
    __shared__ double s_x[2][PT], s_y[2][PT];
    __shared__ double s_box[2][4];            // min x, max x, min y, max y of each side
    const int nt = (P.n + PT - 1) / PT;
    const long long ntp = (long long)nt * (nt + 1) / 2;
    for (long long t = blockIdx.x; t < ntp; t += gridDim.x) {
        int bi, bj;
        tile_of(t, nt, bi, bj);
        __syncthreads();
        if (threadIdx.x < 2 * PT) {
            const int side = threadIdx.x >> 6, l = threadIdx.x & 63;
            const int idx = (side ? bj : bi) * PT + l;
            const bool in = idx < P.n;
            const double x = in ? P.xs[idx] : 0.0, y = in ? P.ys[idx] : 0.0;
            s_x[side][l] = x;
            s_y[side][l] = y;
            double mnx = in ? x : INFINITY, mxx = in ? x : -INFINITY, mny = in ? y : INFINITY, mxy = in ? y : -INFINITY;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                mnx = fmin(mnx, __shfl_xor(mnx, off));
                mxx = fmax(mxx, __shfl_xor(mxx, off));
                mny = fmin(mny, __shfl_xor(mny, off));
                mxy = fmax(mxy, __shfl_xor(mxy, off));
            }
            if (l == 0) { s_box[side][0] = mnx; s_box[side][1] = mxx; s_box[side][2] = mny; s_box[side][3] = mxy; }
        }
        __syncthreads();
        if (skip_far) {
            const double gx = fmax(s_box[1][0] - s_box[0][1], s_box[0][0] - s_box[1][1]);
            const double gy = fmax(s_box[1][2] - s_box[0][3], s_box[0][2] - s_box[1][3]);
            if ((float)gx > P.eps || (float)gy > P.eps) continue;
        }
        const int lj = threadIdx.x & 63;
        const int j = bj * PT + lj;
        if (j >= P.n) continue;               // (no barrier below: the next iteration starts with one every thread reaches)
        const double xj = s_x[1][lj], yj = s_y[1][lj];
        for (int li = threadIdx.x >> 6; li < PT; li += 4) {
            const int i = bi * PT + li;
            if (i >= P.n || i >= j) continue;
            f(i, j, s_x[0][li], s_y[0][li], xj, yj);
        }
    }
}

// the `continue`s above leave threads of a workgroup at different barriers of the SAME loop header only: every thread of the
// block runs the same number of iterations (t is uniform), and both barriers sit before any divergent exit of an iteration.

// ---- union-find: parent[v] <= v always, roots are the smallest members; reads go to the coherent level (another workgroup's
// compare-and-swap is not seen through this CU's L1 otherwise)
__device__ __forceinline__ int uf_find(int *parent, int v) {
    int p = __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != v) {
        v = p;
        p = __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return v;
}
__device__ __forceinline__ void uf_unite(int *parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        if (atomicCAS(parent + a, a, b) == a) return;     // a was still a root: it now hangs under the smaller root
    }
}

__global__ __launch_bounds__(256) void seeds_iota_kernel(int *parent, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = i;
}

__global__ __launch_bounds__(256) void seeds_link_kernel(PairArgs P, int *parent) {
    walk_pairs(P, P.prune != 0, [&](int i, int j, double xi, double yi, double xj, double yj) {
        if (P.prune && (float)pair_xy(xi, yi, xj, yj) > P.eps) return;
        if (pair_dist(P, xi, yi, xj, yj) <= P.eps) uf_unite(parent, i, j);
    });
}

__global__ __launch_bounds__(256) void seeds_flatten_kernel(const int *__restrict__ parent, int n, int *__restrict__ root,
                                                            int *__restrict__ is_root) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int v = i;
    while (parent[v] != v) v = parent[v];
    root[i] = v;
    is_root[i] = v == i;
}

__global__ __launch_bounds__(256) void seeds_rank_kernel(const int *__restrict__ root, const int *__restrict__ rank, int n,
                                                         int32_t *__restrict__ cluster) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) cluster[i] = rank[root[i]];
}

// full symmetric matrix for small n (test hook)
__global__ __launch_bounds__(256) void seeds_matrix_kernel(PairArgs P, float *__restrict__ D) {
    const long long nn = (long long)P.n * P.n;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < nn; k += (long long)gridDim.x * 256) {
        const int a = (int)(k / P.n), b = (int)(k - (long long)a * P.n);
        const int i = a < b ? a : b, j = a < b ? b : a;
        D[k] = (i == j) ? 0.0f : pair_dist(P, P.xs[i], P.ys[i], P.xs[j], P.ys[j]);
    }
}

// ---- statistics: keys that sort like the floats (negative values included); three digit passes of 11 / 11 / 10 bits over the
// recomputed D, two targets (the middle ranks) per pass; pass 0 also takes the extremes and counts NaN
constexpr int ST_NB = 2048;
struct PairStats {
    unsigned long long n_nan;
    unsigned int min_key, max_key;
    unsigned long long hist[2][ST_NB];
};

__device__ __forceinline__ uint32_t dist_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int L> __global__ __launch_bounds__(256) void seeds_hist_kernel(PairArgs P, uint32_t prefix_a, uint32_t prefix_b,
                                                                          PairStats *__restrict__ st) {
    constexpr int WID = L < 2 ? 11 : 10;
    constexpr int CONS = L * 11;
    constexpr int SHIFT = 32 - CONS - WID;
    __shared__ unsigned h[2][ST_NB];
    __shared__ unsigned s_min, s_max, s_nan;
    for (int i = threadIdx.x; i < 2 * ST_NB; i += 256) (&h[0][0])[i] = 0;
    if (threadIdx.x == 0) { s_min = 0xFFFFFFFFu; s_max = 0; s_nan = 0; }
    __syncthreads();
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0;
    unsigned nan = 0;
    walk_pairs(P, false, [&](int, int, double xi, double yi, double xj, double yj) {
        const float d = pair_dist(P, xi, yi, xj, yj);
        if (d != d) { ++nan; return; }
        const uint32_t k = dist_key(d);
        const uint32_t bin = (k >> SHIFT) & (uint32_t)((1 << WID) - 1);
        if (L == 0) {
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
            atomicAdd(&h[0][bin], 1u);
        } else {
            const uint32_t top = k >> (32 - CONS);
            if (top == prefix_a) atomicAdd(&h[0][bin], 1u);
            if (top == prefix_b) atomicAdd(&h[1][bin], 1u);
        }
    });
    if (L == 0) {
        atomicMin(&s_min, kmin);
        atomicMax(&s_max, kmax);
        if (nan) atomicAdd(&s_nan, nan);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * ST_NB; i += 256) {
        const unsigned v = (&h[0][0])[i];
        if (v) atomicAdd(&st->hist[0][0] + i, (unsigned long long)v);
    }
    if (L == 0 && threadIdx.x == 0) {
        atomicMin(&st->min_key, s_min);
        atomicMax(&st->max_key, s_max);
        if (s_nan) atomicAdd(&st->n_nan, (unsigned long long)s_nan);
    }
}

float key_value(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    float f;
    memcpy(&f, &u, sizeof(f));
    return f;
}

// checks the arguments shared by the pair entry points, uploads the sample table and fills P
int pair_setup(obia_ctx *ctx, const double *xs, const double *ys, int n, const float *cost, int H, int W, const double *inv6,
               double weight, double xy_thresh, int samples, const double *ts_host, double eps, int nonneg, PairArgs &P) {
    if (!xs || !ys || !cost || !inv6 || !ts_host || n <= 0 || H <= 0 || W <= 0) {
        set_error("seed pairs: bad arguments");
        return OBIA_E_INVALID;
    }
    if (samples < 1 || samples > PAIR_MAX_SAMPLES) {
        set_error("seed pairs: samples must be in 1..%d (got %d)", PAIR_MAX_SAMPLES, samples);
        return OBIA_E_UNSUPPORTED;
    }
    if (n > (1 << 20)) { set_error("seed pairs: more than 2^20 seeds not supported (got %d)", n); return OBIA_E_UNSUPPORTED; }
    if ((long long)H * W > 0x7fffffffLL) { set_error("seed pairs: cost raster above 2^31 pixels"); return OBIA_E_UNSUPPORTED; }
    double *d_ts = ctx->arena.get<double>((size_t)samples);
    if (!d_ts) return OBIA_E_NOMEM;
    OBIA_TRY(upload_async(ctx, d_ts, ts_host, sizeof(double) * (size_t)samples));
    P.xs = xs; P.ys = ys; P.cost = cost; P.ts = d_ts;
    P.n = n; P.H = H; P.W = W; P.samples = samples;
    for (int k = 0; k < 6; ++k) P.inv[k] = inv6[k];
    P.xy_thresh = xy_thresh;
    P.weight = (float)weight;
    P.eps = (float)eps;
    P.weight_zero = weight == 0.0;
    P.prune = nonneg != 0 && weight >= 0.0;
    return OBIA_OK;
}

int pair_grid(int n) { return (int)grids::seeds_pairs(n).x.n; }

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_seeds_peaks_dev(obia_ctx *ctx, const float *plane, int H, int W, double sigma, int min_dist_px, float threshold,
                         float *smooth_out, uint8_t *flags_out, int32_t *offsets_out, int64_t *n_peaks_out) {
    OBIA_TRY(enter(ctx));
    if (!plane || !flags_out || !offsets_out || !n_peaks_out || H <= 0 || W <= 0 || ((uintptr_t)flags_out & 15)) {
        set_error("seed peaks: bad arguments (the flag plane must be 16-byte aligned)");
        return OBIA_E_INVALID;
    }
    if ((long long)H * W > 0x7fffffffLL - CHUNK) { set_error("seed peaks: rasters above 2^31 pixels not supported"); return OBIA_E_UNSUPPORTED; }
    if (min_dist_px < 0 || min_dist_px > MX_MAXD) {
        set_error("seed peaks: min_dist_px must be in 0..%d (got %d)", MX_MAXD, min_dist_px);
        return OBIA_E_UNSUPPORTED;
    }
    if (!(sigma >= 0.0) || !(sigma <= 1000.0)) { set_error("seed peaks: sigma must be in 0..1000"); return OBIA_E_INVALID; }
    if (sigma > 0.0 && !smooth_out) { set_error("seed peaks: sigma > 0 needs smooth_out"); return OBIA_E_INVALID; }
    const long long n = (long long)H * W;
    const int nchunks = cdiv(n, CHUNK);
    ctx->arena.reset();
    const float *g = plane;
    if (sigma > 0.0) {
        std::vector<double> w;
        const int r = gaussian_weights_host(sigma, false, w);
        double *d_w = ctx->arena.get<double>(w.size());
        float *tmp = ctx->arena.get<float>((size_t)n);
        if (!d_w || !tmp) return OBIA_E_NOMEM;
        OBIA_TRY(upload_async(ctx, d_w, w.data(), sizeof(double) * w.size()));
        const dim3 grid = to_dim3(grids::seeds_gauss(n));
        hipLaunchKernelGGL(seeds_gauss_kernel<0>, grid, dim3(256), 0, ctx->stream, plane, tmp, H, W, d_w, r);
        hipLaunchKernelGGL(seeds_gauss_kernel<1>, grid, dim3(256), 0, ctx->stream, tmp, smooth_out, H, W, d_w, r);
        g = smooth_out;
    }
    int *counts = ctx->arena.get<int>((size_t)nchunks);
    if (!counts) return OBIA_E_NOMEM;
    // the flag bytes past the last pixel, up to the end of the last chunk
    if ((long long)nchunks * CHUNK > n) OBIA_HIP_TRY(hipMemsetAsync(flags_out + n, 0, (size_t)((long long)nchunks * CHUNK - n), ctx->stream));
    const int d = min_dist_px;
    const size_t lds = sizeof(float) * (size_t)(MX_TH + 2 * d) * (size_t)(2 * MX_TW + 2 * d);
    hipLaunchKernelGGL(seeds_flag_kernel, to_dim3(grids::seeds_flag(H, W)), dim3(256), lds, ctx->stream, g, H, W, d,
                       threshold, flags_out);
    hipLaunchKernelGGL(seeds_count_kernel, dim3(nchunks), dim3(256), 0, ctx->stream, flags_out, counts);
    hipLaunchKernelGGL(seeds_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, counts, offsets_out, nchunks);
    OBIA_HIP_TRY(hipGetLastError());
    int total = 0;
    OBIA_TRY(read_back(ctx, &total, offsets_out + nchunks, sizeof(int)));
    *n_peaks_out = total;
    return OBIA_OK;
}

int obia_seeds_peaks_gather_dev(obia_ctx *ctx, const float *plane, const float *smooth, const uint8_t *flags, const int32_t *offsets,
                                int H, int W, int64_t n_peaks, int32_t *rows_out, int32_t *cols_out, float *smooth_val_out,
                                float *raw_val_out) {
    OBIA_TRY(enter(ctx));
    if (!plane || !smooth || !flags || !offsets || H <= 0 || W <= 0 || n_peaks < 0 || ((uintptr_t)flags & 15)) {
        set_error("seed peaks gather: bad arguments");
        return OBIA_E_INVALID;
    }
    if (n_peaks == 0) return OBIA_OK;
    if (!rows_out || !cols_out || !smooth_val_out || !raw_val_out) { set_error("seed peaks gather: null output"); return OBIA_E_INVALID; }
    const int nchunks = cdiv((long long)H * W, CHUNK);
    hipLaunchKernelGGL(seeds_scatter_kernel, dim3(nchunks), dim3(256), 0, ctx->stream, flags, offsets, smooth, plane, W, rows_out, cols_out,
                       smooth_val_out, raw_val_out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_seeds_pair_link_dev(obia_ctx *ctx, const double *xs, const double *ys, int n, const float *cost, int H, int W,
                             const double *inv6, double weight, double xy_thresh, int samples, const double *ts_host, double eps,
                             int nonneg, int32_t *cluster_out, int *n_clusters_out) {
    OBIA_TRY(enter(ctx));
    if (!cluster_out || !n_clusters_out) { set_error("seed pairs: null output"); return OBIA_E_INVALID; }
    ctx->arena.reset();
    PairArgs P;
    OBIA_TRY(pair_setup(ctx, xs, ys, n, cost, H, W, inv6, weight, xy_thresh, samples, ts_host, eps, nonneg, P));
    int *parent = ctx->arena.get<int>((size_t)n);
    int *root = ctx->arena.get<int>((size_t)n);
    int *is_root = ctx->arena.get<int>((size_t)n);
    int *rank = ctx->arena.get<int>((size_t)n + 1);
    if (!parent || !root || !is_root || !rank) return OBIA_E_NOMEM;
    const dim3 gn(cdiv(n, 256));
    hipLaunchKernelGGL(seeds_iota_kernel, gn, dim3(256), 0, ctx->stream, parent, n);
    hipLaunchKernelGGL(seeds_link_kernel, dim3(pair_grid(n)), dim3(256), 0, ctx->stream, P, parent);
    hipLaunchKernelGGL(seeds_flatten_kernel, gn, dim3(256), 0, ctx->stream, parent, n, root, is_root);
    hipLaunchKernelGGL(seeds_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, is_root, rank, n);
    hipLaunchKernelGGL(seeds_rank_kernel, gn, dim3(256), 0, ctx->stream, root, rank, n, cluster_out);
    OBIA_HIP_TRY(hipGetLastError());
    int total = 0;
    OBIA_TRY(read_back(ctx, &total, rank + n, sizeof(int)));
    *n_clusters_out = total;
    return OBIA_OK;
}

int obia_seeds_pair_stats_dev(obia_ctx *ctx, const double *xs, const double *ys, int n, const float *cost, int H, int W,
                              const double *inv6, double weight, double xy_thresh, int samples, const double *ts_host,
                              float *stats4_out, int64_t *n_nan_out) {
    OBIA_TRY(enter(ctx));
    if (!stats4_out || !n_nan_out) { set_error("seed pair stats: null output"); return OBIA_E_INVALID; }
    if (n < 2) { set_error("seed pair stats: fewer than two seeds have no pair"); return OBIA_E_EMPTY; }
    ctx->arena.reset();
    PairArgs P;
    OBIA_TRY(pair_setup(ctx, xs, ys, n, cost, H, W, inv6, weight, xy_thresh, samples, ts_host, 0.0, 0, P));
    PairStats *st = ctx->arena.get<PairStats>(1);
    if (!st) return OBIA_E_NOMEM;
    std::vector<unsigned long long> h(sizeof(PairStats) / 8);
    const PairStats *hs = reinterpret_cast<const PairStats *>(h.data());
    const unsigned long long init[2] = {0ull, 0x00000000FFFFFFFFull};   // n_nan = 0 | min_key = all ones, max_key = 0
    const dim3 grid(pair_grid(n));
    const long long N = (long long)n * (n - 1) / 2;
    uint32_t prefix[2] = {0, 0};
    long long rank[2] = {(N - 1) / 2, N / 2};             // the middle values: the same one when N is odd
    const float nanv = std::nanf("");
    for (int L = 0; L < 3; ++L) {
        OBIA_HIP_TRY(hipMemsetAsync(st, 0, sizeof(PairStats), ctx->stream));
        if (L == 0) {
            OBIA_TRY(upload_async(ctx, st, init, sizeof(init)));
            hipLaunchKernelGGL(seeds_hist_kernel<0>, grid, dim3(256), 0, ctx->stream, P, 0u, 0u, st);
        } else if (L == 1) {
            hipLaunchKernelGGL(seeds_hist_kernel<1>, grid, dim3(256), 0, ctx->stream, P, prefix[0], prefix[1], st);
        } else {
            hipLaunchKernelGGL(seeds_hist_kernel<2>, grid, dim3(256), 0, ctx->stream, P, prefix[0], prefix[1], st);
        }
        OBIA_HIP_TRY(hipGetLastError());
        OBIA_TRY(read_back(ctx, h.data(), st, sizeof(PairStats)));
        if (L == 0) {
            *n_nan_out = (int64_t)hs->n_nan;
            if (hs->n_nan) {                              // np.min / np.median / np.max of an array that holds a NaN
                for (int k = 0; k < 4; ++k) stats4_out[k] = nanv;
                return OBIA_OK;
            }
            stats4_out[0] = key_value(hs->min_key);
            stats4_out[3] = key_value(hs->max_key);
        }
        const int wid = L < 2 ? 11 : 10;
        for (int t = 0; t < 2; ++t) {
            const unsigned long long *hg = hs->hist[L == 0 ? 0 : t];
            long long below = 0;
            int bin = 0;
            for (; bin < (1 << wid) - 1; ++bin) {
                if (rank[t] < below + (long long)hg[bin]) break;
                below += (long long)hg[bin];
            }
            prefix[t] = (prefix[t] << wid) | (uint32_t)bin;
            rank[t] -= below;
        }
    }
    stats4_out[1] = key_value(prefix[0]);
    stats4_out[2] = key_value(prefix[1]);
    return OBIA_OK;
}

int obia_seeds_pair_matrix_dev(obia_ctx *ctx, const double *xs, const double *ys, int n, const float *cost, int H, int W,
                               const double *inv6, double weight, double xy_thresh, int samples, const double *ts_host,
                               float *matrix_out) {
    OBIA_TRY(enter(ctx));
    if (!matrix_out) { set_error("seed pair matrix: null output"); return OBIA_E_INVALID; }
    if (n > 512) { set_error("seed pair matrix: a test hook for n <= 512 (got %d)", n); return OBIA_E_UNSUPPORTED; }
    ctx->arena.reset();
    PairArgs P;
    OBIA_TRY(pair_setup(ctx, xs, ys, n, cost, H, W, inv6, weight, xy_thresh, samples, ts_host, 0.0, 0, P));
    hipLaunchKernelGGL(seeds_matrix_kernel, dim3(cdiv((long long)n * n, 256)), dim3(256), 0, ctx->stream, P, matrix_out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

}  // extern "C"
