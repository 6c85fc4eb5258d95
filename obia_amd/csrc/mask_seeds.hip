// mask_seeds.hip -- maskSLIC seeding as scikit-image 0.18 does it (`_get_mask_centroids`, slic_superpixels.py:14-68), bit for bit:
// k-means (scipy.cluster.vq.kmeans2, 5 iterations) on a random subset of the valid pixels, started from a sparser random subset,
// then per centroid the nearest other centroid (pdist + argmin) for `steps`.  The random picks are the caller's (NumPy's frozen
// legacy generator stays in NumPy); everything from the picks on is here.
//
// Why a parallel version can be bit-exact:
//   * a point's label is a per-point argmin with a fixed tie rule -- ascending centroid index, strict `<` -- and every lane scans the
//     code book in exactly that order;
//   * the distance is ((0 + dz*dz) + dy*dy) + dx*dx in float64 with separate multiply and add; dz is exactly 0, so the first two
//     terms are dy*dy exactly.  The Makefile's -ffp-contract=off keeps multiply and add apart;
//   * a cluster's sum is a sum of integer pixel coordinates: 64-bit integer atomics, exact and order-free, so two runs agree bit for
//     bit; the mean is one IEEE division per coordinate;
//   * pdist compares ROOTS: two different squares can round to one root, and then the lower index wins.  sqrt is monotonic, so a
//     root needs computing only when the square is below the best square so far -- same index in every case, no K x K roots.
// No K x K matrix and no (n_valid, 3) coordinate table are stored.
#include "slic.hpp"
#include "wave_ops.hpp"

#include <algorithm>
#include <cmath>

namespace obia {
namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_CHUNK = OBIA_MASK_SEEDS_CHUNK;   // centroids staged in LDS at a time: 1024 x (y, x) float64 = 16 KiB

// ---- rank -> coordinate ---------------------------------------------------------------------------------------------------------
// valid pixels of each mask row
__global__ __launch_bounds__(MS_THREADS) void ms_row_count_kernel(const uint8_t *__restrict__ mask, int W, int *__restrict__ rowcnt) {
    const uint8_t *row = mask + (size_t)blockIdx.x * W;
    int c = 0;
    for (int x = threadIdx.x; x < W; x += MS_THREADS) c += row[x] != 0;
    c = block_sum<MS_THREADS>(c);
    if (threadIdx.x == 0) rowcnt[blockIdx.x] = c;
}

// exclusive prefix over the rows (one workgroup): rowoff[r] = rank of row r's first valid pixel, rowoff[H] = n_valid
__global__ __launch_bounds__(1024) void ms_row_scan_kernel(const int *__restrict__ rowcnt, int H, long long *__restrict__ rowoff) {
    workgroup_exclusive_scan<1024>(rowcnt, rowoff, H, rowoff + H);
}

// One workgroup per mask row: the rank of every valid pixel (row offset + prefix inside the row); a pixel whose rank is picks[j]
// writes (y, x) to out[j].  picks == nullptr: every valid pixel, out[rank].  j < n_picks by the search, rank < n_valid = rowoff[H].
__global__ __launch_bounds__(MS_THREADS) void ms_gather_kernel(const uint8_t *__restrict__ mask, int W, const long long *__restrict__ rowoff,
                                                               const long long *__restrict__ picks, long long n_picks,
                                                               int2 *__restrict__ out) {
    const int y = blockIdx.x;
    const long long first = rowoff[y];
    if (rowoff[y + 1] == first) return;   // (uniform over the workgroup) no valid pixel in this row
    const uint8_t *row = mask + (size_t)y * W;
    long long base = first;
    for (int x0 = 0; x0 < W; x0 += MS_THREADS) {
        const int x = x0 + (int)threadIdx.x;
        const bool v = x < W && row[x] != 0;
        int total;
        const int before = block_flag_rank<MS_THREADS>(v, total);
        if (v) {
            const long long rank = base + before;
            if (!picks) {
                out[rank] = make_int2(y, x);
            } else {
                long long lo = 0, hi = n_picks;
                while (lo < hi) {
                    const long long mid = (lo + hi) >> 1;
                    if (picks[mid] < rank) lo = mid + 1; else hi = mid;
                }
                if (lo < n_picks && picks[lo] == rank) out[lo] = make_int2(y, x);
            }
        }
        base += total;
    }
}

__global__ __launch_bounds__(MS_THREADS) void ms_init_book_kernel(const int2 *__restrict__ seeds, int K, double2 *__restrict__ book) {
    const int k = blockIdx.x * MS_THREADS + threadIdx.x;
    if (k < K) book[k] = make_double2((double)seeds[k].x, (double)seeds[k].y);
}

// ---- k-means --------------------------------------------------------------------------------------------------------------------
// One lane per point; the code book passes through LDS in index order, MS_CHUNK centroids at a time (every lane reads the same
// address: a broadcast).  The label goes straight into the cluster's integer sums: acc[3k] = sum y, [3k + 1] = sum x, [3k + 2] = count.
__global__ __launch_bounds__(MS_THREADS) void ms_assign_kernel(const int2 *__restrict__ pts, long long n, const double2 *__restrict__ book, int K,
                                                               unsigned long long *__restrict__ acc) {
    __shared__ double2 sb[MS_CHUNK];
    const long long i = (long long)blockIdx.x * MS_THREADS + threadIdx.x;
    const bool live = i < n;
    const int2 p = live ? pts[i] : make_int2(0, 0);
    const double py = (double)p.x, px = (double)p.y;
    double best = INFINITY;
    int lab = 0;
    for (int c0 = 0; c0 < K; c0 += MS_CHUNK) {
        const int m = min(MS_CHUNK, K - c0);
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += MS_THREADS) sb[t] = book[c0 + t];
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            const double2 c = sb[j];
            const double dy = py - c.x, dx = px - c.y;
            const double d = dy * dy + dx * dx;   // (0 + 0 * 0) + dy * dy is dy * dy exactly
            if (d < best) { best = d; lab = c0 + j; }
        }
    }
    if (live) {
        atomicAdd(&acc[3 * (size_t)lab], (unsigned long long)p.x);
        atomicAdd(&acc[3 * (size_t)lab + 1], (unsigned long long)p.y);
        atomicAdd(&acc[3 * (size_t)lab + 2], 1ull);
    }
}

// new centroid = sum / count, one division per coordinate (the sums are below 2^53: exact as float64); a cluster without points
// keeps its centroid.  Clears the sums for the next iteration.
__global__ __launch_bounds__(MS_THREADS) void ms_finalise_kernel(unsigned long long *__restrict__ acc, int K, double2 *__restrict__ book) {
    const int k = blockIdx.x * MS_THREADS + threadIdx.x;
    if (k >= K) return;
    const unsigned long long sy = acc[3 * (size_t)k], sx = acc[3 * (size_t)k + 1], cnt = acc[3 * (size_t)k + 2];
    if (cnt) {
        const double c = (double)cnt;
        book[k] = make_double2((double)sy / c, (double)sx / c);
    }
    acc[3 * (size_t)k] = 0; acc[3 * (size_t)k + 1] = 0; acc[3 * (size_t)k + 2] = 0;
}

// ---- nearest other centroid -----------------------------------------------------------------------------------------------------
// One lane per centroid i, the same LDS-chunked ascending scan over j != i.  closest[i] = the first j that minimises
// sqrt(dy*dy + dx*dx); with K = 1 there is no other centroid and closest[0] = 0 (argmin of an all-infinite row).
__global__ __launch_bounds__(MS_THREADS) void ms_nearest_kernel(const double2 *__restrict__ book, int K, int *__restrict__ closest) {
    __shared__ double2 sb[MS_CHUNK];
    const int i = blockIdx.x * MS_THREADS + threadIdx.x;
    const bool live = i < K;
    const double2 ci = live ? book[i] : make_double2(0.0, 0.0);
    double best_sq = INFINITY, best_rt = INFINITY;
    int bj = 0;
    for (int c0 = 0; c0 < K; c0 += MS_CHUNK) {
        const int m = min(MS_CHUNK, K - c0);
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += MS_THREADS) sb[t] = book[c0 + t];
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            const double2 c = sb[j];
            const double dy = ci.x - c.x, dx = ci.y - c.y;
            const double s = dy * dy + dx * dx;
            if (s < best_sq && c0 + j != i) {
                // a square at or above best_sq has a root at or above best_rt; below it the root may still be EQUAL: roots decide
                const double r = sqrt(s);
                if (r < best_rt) { best_rt = r; bj = c0 + j; }
                best_sq = s;
            }
        }
    }
    if (live) closest[i] = bj;
}

// ---- a tile of a batch: seeds and steps stay on the device -----------------------------------------------------------------------
// One workgroup.  seeds_out[k] = the centroid as the float32 pair the sweeps start from (segments.astype(float32)); steps_out[0..1] =
// abs(centroids - centroids[closest]).mean(0) of the row and column axes.  NumPy reduces axis 0 of the C-ordered (K, 3) array row by
// row, one running sum per column, then divides by K: the terms are computed by all lanes, MS_CHUNK at a time into LDS, and ONE lane
// adds them up in index order -- the order of the host loop in mask_centroids_dev, bit for bit.
__global__ __launch_bounds__(MS_THREADS) void ms_emit_kernel(const double2 *__restrict__ book, const int *__restrict__ closest, int K,
                                                             float2 *__restrict__ seeds_out, double *__restrict__ steps_out) {
    __shared__ double2 sd[MS_CHUNK];
    double sy = 0.0, sx = 0.0;
    for (int c0 = 0; c0 < K; c0 += MS_CHUNK) {
        const int m = min(MS_CHUNK, K - c0);
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += MS_THREADS) {
            const double2 a = book[c0 + t];
            const int j = closest[c0 + t];                                      // (0 <= j < K: ms_nearest_kernel)
            const double2 o = book[j];
            sd[t] = make_double2(fabs(a.x - o.x), fabs(a.y - o.y));
            seeds_out[c0 + t] = make_float2((float)a.x, (float)a.y);
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int t = 0; t < m; ++t) { sy += sd[t].x; sx += sd[t].y; }
    }
    if (threadIdx.x == 0) { steps_out[0] = sy / (double)K; steps_out[1] = sx / (double)K; }
}

}  // namespace

// rank of every row's first valid pixel: rowoff[0 .. H], rowoff[H] = n_valid
static int ms_rank_rows(obia_ctx *ctx, const uint8_t *mask, int H, int W, long long **rowoff_out) {
    Arena &A = ctx->arena;
    int *rowcnt = A.get<int>((size_t)H);
    long long *rowoff = A.get<long long>((size_t)H + 1);
    if (!rowcnt || !rowoff) return OBIA_E_NOMEM;
    hipLaunchKernelGGL(ms_row_count_kernel, dim3(H), dim3(MS_THREADS), 0, ctx->stream, mask, W, rowcnt);
    hipLaunchKernelGGL(ms_row_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, rowcnt, H, rowoff);
    OBIA_HIP_TRY(hipGetLastError());
    *rowoff_out = rowoff;
    return OBIA_OK;
}

// picks -> k-means -> nearest other centroid, queued on the context's stream; book / closest: K entries each, in the arena
static int ms_kmeans(obia_ctx *ctx, const uint8_t *mask, int H, int W, const long long *rowoff, const int64_t *picks, int K, const int64_t *dense,
                     long long n_dense, long long n_pts, int iters, double2 **book_out, int **closest_out) {
    Arena &A = ctx->arena;
    long long *d_picks = A.get<long long>((size_t)K);
    long long *d_dense = dense ? A.get<long long>((size_t)n_dense) : nullptr;
    int2 *seeds = A.get<int2>((size_t)K);
    int2 *pts = A.get<int2>((size_t)n_pts);
    double2 *book = A.get<double2>((size_t)K);
    unsigned long long *acc = A.get<unsigned long long>(3 * (size_t)K);
    int *closest = A.get<int>((size_t)K);
    if (!d_picks || (dense && !d_dense) || !seeds || !pts || !book || !acc || !closest) return OBIA_E_NOMEM;
    OBIA_TRY(upload_async(ctx, d_picks, picks, sizeof(long long) * (size_t)K));
    if (dense) OBIA_TRY(upload_async(ctx, d_dense, dense, sizeof(long long) * (size_t)n_dense));
    OBIA_HIP_TRY(hipMemsetAsync(acc, 0, sizeof(unsigned long long) * 3 * (size_t)K, ctx->stream));
    hipLaunchKernelGGL(ms_gather_kernel, dim3(H), dim3(MS_THREADS), 0, ctx->stream, mask, W, rowoff, d_picks, (long long)K, seeds);
    hipLaunchKernelGGL(ms_gather_kernel, dim3(H), dim3(MS_THREADS), 0, ctx->stream, mask, W, rowoff, d_dense, n_dense, pts);
    const dim3 kgrid(cdiv(K, MS_THREADS));
    hipLaunchKernelGGL(ms_init_book_kernel, kgrid, dim3(MS_THREADS), 0, ctx->stream, seeds, K, book);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(ms_assign_kernel, dim3(cdiv(n_pts, MS_THREADS)), dim3(MS_THREADS), 0, ctx->stream, pts, n_pts, book, K, acc);
        hipLaunchKernelGGL(ms_finalise_kernel, kgrid, dim3(MS_THREADS), 0, ctx->stream, acc, K, book);
    }
    hipLaunchKernelGGL(ms_nearest_kernel, kgrid, dim3(MS_THREADS), 0, ctx->stream, book, K, closest);
    OBIA_HIP_TRY(hipGetLastError());
    *book_out = book;
    *closest_out = closest;
    return OBIA_OK;
}

int mask_centroids_dev(obia_ctx *ctx, const uint8_t *mask, int H, int W, const int64_t *picks, int K, const int64_t *dense, long long n_dense,
                       int iters, double *centroids_yx_out, double *steps_zyx_out) {
    Arena &A = ctx->arena;
    A.reset();
    long long *rowoff = nullptr;
    OBIA_TRY(ms_rank_rows(ctx, mask, H, W, &rowoff));
    long long n_valid = 0;
    OBIA_TRY(read_back(ctx, &n_valid, rowoff + H, sizeof(long long)));
    // the picks are sorted (checked by the caller): the last one bounds them all
    if (picks[K - 1] >= n_valid) {
        set_error("mask centroids: pick %lld out of range, the mask has %lld valid pixels", (long long)picks[K - 1], n_valid);
        return OBIA_E_INVALID;
    }
    if (dense && dense[n_dense - 1] >= n_valid) {
        set_error("mask centroids: dense pick %lld out of range, the mask has %lld valid pixels", (long long)dense[n_dense - 1], n_valid);
        return OBIA_E_INVALID;
    }
    const long long n_pts = dense ? n_dense : n_valid;
    if ((double)n_pts * (double)std::max(H, W) >= 9007199254740992.0) {   // coordinate sums must stay exact as float64
        set_error("mask centroids: %lld points on a (%d, %d) raster overflow the exact sums", n_pts, H, W);
        return OBIA_E_UNSUPPORTED;
    }
    double2 *book = nullptr;
    int *closest = nullptr;
    OBIA_TRY(ms_kmeans(ctx, mask, H, W, rowoff, picks, K, dense, n_dense, n_pts, iters, &book, &closest));
    std::vector<int> h_closest((size_t)K);
    OBIA_HIP_TRY(hipMemcpyAsync(centroids_yx_out, book, sizeof(double2) * (size_t)K, hipMemcpyDeviceToHost, ctx->stream));
    OBIA_TRY(read_back(ctx, h_closest.data(), closest, sizeof(int) * (size_t)K));
    // steps = abs(centroids - centroids[closest]).mean(0): NumPy reduces axis 0 of the C-ordered (K, 3) array row by row, one running
    // sum per column, then divides by K.  K values: on the host.  The depth column is all zeros.
    double sy = 0.0, sx = 0.0;
    for (int i = 0; i < K; ++i) {
        const double *a = centroids_yx_out + 2 * (size_t)i, *b = centroids_yx_out + 2 * (size_t)h_closest[(size_t)i];
        sy += std::fabs(a[0] - b[0]);
        sx += std::fabs(a[1] - b[1]);
    }
    steps_zyx_out[0] = 0.0;
    steps_zyx_out[1] = sy / (double)K;
    steps_zyx_out[2] = sx / (double)K;
    return OBIA_OK;
}

int mask_centroids_queue(obia_ctx *ctx, const uint8_t *mask, int h, int w, long long n_valid, const int64_t *picks, int K, const int64_t *dense,
                         long long n_dense, int iters, float *seeds_out_dev, double *steps_out_dev) {
    if (!mask || !picks || K < 1 || h <= 0 || w <= 0 || n_valid < K || n_valid > (long long)h * w || (dense && (n_dense < 1 || n_dense > n_valid)) ||
        !seeds_out_dev || !steps_out_dev) {
        set_error("mask centroids (tile): bad arguments");
        return OBIA_E_INVALID;
    }
    Arena &A = ctx->arena;
    const Arena::Mark mk = A.mark();
    long long *rowoff = nullptr;
    OBIA_TRY(ms_rank_rows(ctx, mask, h, w, &rowoff));
    const long long n_pts = dense ? n_dense : n_valid;   // without the dense draw every valid pixel is a point
    double2 *book = nullptr;
    int *closest = nullptr;
    OBIA_TRY(ms_kmeans(ctx, mask, h, w, rowoff, picks, K, dense, n_dense, n_pts, iters, &book, &closest));
    hipLaunchKernelGGL(ms_emit_kernel, dim3(1), dim3(MS_THREADS), 0, ctx->stream, book, closest, K, reinterpret_cast<float2 *>(seeds_out_dev), steps_out_dev);
    OBIA_HIP_TRY(hipGetLastError());
    A.rewind(mk);   // (reused in stream order by whatever the caller queues next)
    return OBIA_OK;
}

}  // namespace obia
