// ground.hip -- height above ground from raw elevations (include/obia_ground.h): every point against its k nearest ground points on a
// uniform grid, or against a terrain raster.  DESIGN.md 3.5t.
//
// The search is one lane per query.  The ground arrays lie in cell order, so a grid row of a ring's top or bottom edge is ONE run of
// positions (cell_start of its first cell to cell_start past its last), and only the left and right edges are walked cell by cell.  The
// candidate list -- at most eight triples (d2, i, gz), ordered by (d2, i) -- lives in registers: the kernel is a template of the
// count, every index into the list is a constant after unrolling, and the build shows no scratch.  The order of the visits does not
// matter, because a candidate is placed by the pair (d2, i) alone; every d2 is two subtractions, two multiplies and one add in float64
// with nothing contracted (-ffp-contract=off), so the result is the same bits for every order of the queries and every cut.
#include "common.hpp"
#include "../../include/obia_ground.h"

#include <climits>
#include <cmath>

namespace obia {
namespace {

constexpr int NONE = INT_MAX;                                    // the index of an empty slot: above every ground index (ng < 2^31)

struct GroundArgs {
    const double *gx, *gy, *gz;
    const int *gidx, *cell_start;
    long long ncx, ncy, cx0, cy0;
    int ng;
    double side, md2;                                            // md2 = max_distance^2, judged only when limited
    int limited;
    const double *x, *y, *z;
    long long n;
    double *zg;
    float *hag;
    unsigned char *m;
};

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ float quiet_nanf() { return __uint_as_float(0x7fc00000u); }

// what both kernels write for a point: zg, and hag = (float)(z - zg) in one rounding; every NaN is the quiet NaN
__device__ __forceinline__ void write_point(long long i, double zg, const double *z, double *zg_out, float *hag_out) {
    if (zg != zg) zg = quiet_nan();
    if (zg_out) zg_out[i] = zg;
    if (hag_out) {
        float h = (float)(z[i] - zg);
        if (h != h) h = quiet_nanf();
        hag_out[i] = h;
    }
}

template <int K> struct Best {
    double d[K], z[K];
    int id[K];
};

template <int K> __device__ __forceinline__ bool before(double d, int i, const Best<K> &B, int k) {
    return d < B.d[k] || (d == B.d[k] && i < B.id[k]);
}

// the positions lo .. hi - 1 of the ground arrays as candidates of the query (X, Y)
template <int K> __device__ __forceinline__ void offer_run(const GroundArgs &A, double X, double Y, int lo, int hi, Best<K> &B) {
    lo = lo < 0 ? 0 : lo;
    hi = hi > A.ng ? A.ng : hi;
    for (int p = lo; p < hi; ++p) {
        const double dx = X - A.gx[p], dy = Y - A.gy[p];
        double d = dx * dx + dy * dy;
        if (A.limited && !(d <= A.md2)) continue;
        int i = A.gidx[p];
        if (!before<K>(d, i, B, K - 1)) continue;
        double z = A.gz[p];
        // one pass of compare and swap: the candidate settles at its place and what it displaced moves on; the last one falls out
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool lt = before<K>(d, i, B, k);
            const double td = B.d[k], tz = B.z[k];
            const int ti = B.id[k];
            B.d[k] = lt ? d : td;
            B.z[k] = lt ? z : tz;
            B.id[k] = lt ? i : ti;
            d = lt ? td : d;
            z = lt ? tz : z;
            i = lt ? ti : i;
        }
    }
}

template <int K> __global__ __launch_bounds__(256) void ground_query_kernel(GroundArgs A) {
    const double lim = 1073741824.0;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < A.n; q += (long long)gridDim.x * 256) {
        const double X = A.x[q], Y = A.y[q];
        if (!(isfinite(X) && isfinite(Y))) {
            write_point(q, quiet_nan(), A.z, A.zg, A.hag);
            if (A.m) A.m[q] = 0;
            continue;
        }
        Best<K> B;
#pragma unroll
        for (int k = 0; k < K; ++k) { B.d[k] = __longlong_as_double(0x7ff0000000000000ll); B.z[k] = 0.0; B.id[k] = NONE; }
        // the query's cell, clamped into the grid
        long long cx = (long long)fmin(fmax(floor(X / A.side), -lim), lim) - A.cx0;
        long long cy = (long long)fmin(fmax(floor(Y / A.side), -lim), lim) - A.cy0;
        cx = cx < 0 ? 0 : (cx > A.ncx - 1 ? A.ncx - 1 : cx);
        cy = cy < 0 ? 0 : (cy > A.ncy - 1 ? A.ncy - 1 : cy);
        const long long far_x = cx > A.ncx - 1 - cx ? cx : A.ncx - 1 - cx, far_y = cy > A.ncy - 1 - cy ? cy : A.ncy - 1 - cy;
        const long long r_all = far_x > far_y ? far_x : far_y;                  // the ring that covers the whole grid
        for (long long r = 0;; ++r) {
            // the pieces of ring r, one run each: 0 the top row, 1 the bottom row (ring 0 has the one), then the cells of the left and
            // of the right edge between them.  An edge whose column lies outside the grid has no pieces, so a ring costs two steps
            // and its cells inside the grid, and all rings together O(ncx + ncy + cells) = O(ng) whatever the shape of the grid.
            const long long xl = cx - r < 0 ? 0 : cx - r, xr = cx + r > A.ncx - 1 ? A.ncx - 1 : cx + r;
            const long long yl = cy - r + 1 < 0 ? 0 : cy - r + 1, yh = cy + r - 1 > A.ncy - 1 ? A.ncy - 1 : cy + r - 1;
            const long long ny = yh >= yl ? yh - yl + 1 : 0;
            const long long n_left = cx - r >= 0 ? ny : 0, n_right = cx + r <= A.ncx - 1 ? ny : 0;
            for (long long t = 0; t < 2 + n_left + n_right; ++t) {
                long long c0, c1;
                bool inside = true;
                if (t < 2) {
                    const long long yy = t == 0 ? cy - r : cy + r;
                    inside = yy >= 0 && yy <= A.ncy - 1 && (t == 0 || r > 0);
                    c0 = yy * A.ncx + xl;
                    c1 = yy * A.ncx + xr;
                } else {
                    const bool left = t - 2 < n_left;
                    c0 = c1 = (yl + (left ? t - 2 : t - 2 - n_left)) * A.ncx + (left ? cx - r : cx + r);
                }
                if (inside) offer_run<K>(A, X, Y, A.cell_start[c0], A.cell_start[c1 + 1], B);
            }
            if (r >= r_all) break;
            if (r >= 1) {
                // no ground point outside ring r is nearer than this: a full list below it is final
                const double rs = (double)r * A.side;
                const double bound = rs * rs * (1.0 - 9.5367431640625e-07);      // 1 - 2^-20
                if (B.id[K - 1] != NONE && B.d[K - 1] < bound) break;
                if (A.limited && bound > A.md2) break;
            }
        }
        int m = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) m += B.id[k] != NONE ? 1 : 0;
        double zg;
        if (m == 0) {
            zg = quiet_nan();
        } else if (m == 1 || B.d[0] == 0.0) {
            zg = B.z[0];
        } else {
            double num = 0.0, den = 0.0;
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (k < m) {
                    num = num + B.z[k] / B.d[k];
                    den = den + 1.0 / B.d[k];
                }
            zg = num / den;
        }
        write_point(q, zg, A.z, A.zg, A.hag);
        if (A.m) A.m[q] = (unsigned char)m;
    }
}

struct DtmArgs {
    const double *x, *y, *z;
    long long n;
    double a, b, d, e, xoff, yoff;
    const float *dtm;
    int H, W;
    double *zg;
    float *hag;
};

__global__ __launch_bounds__(256) void ground_dtm_kernel(DtmArgs A) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < A.n; i += (long long)gridDim.x * 256) {
        const double X = A.x[i], Y = A.y[i];
        const double col = floor(A.a * X + A.b * Y + A.xoff), row = floor(A.d * X + A.e * Y + A.yoff);      // THE PIXEL RULE
        double zg = quiet_nan();
        if (col >= 0.0 && col < (double)A.W && row >= 0.0 && row < (double)A.H) {
            const float v = A.dtm[(long long)row * A.W + (long long)col];
            if (isfinite(v)) zg = (double)v;
        }
        write_point(i, zg, A.z, A.zg, A.hag);
    }
}

template <int K> void launch_query(obia_ctx *ctx, const GroundArgs &A) {
    hipLaunchKernelGGL(ground_query_kernel<K>, to_dim3(grids::ground_query(A.n)), dim3(256), 0, ctx->stream, A);
}

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_ground_query_dev(obia_ctx *ctx, const double *gx, const double *gy, const double *gz, const int32_t *gidx, int64_t ng,
                          const int32_t *cell_start, int64_t ncx, int64_t ncy, int64_t cx0, int64_t cy0, double side, const double *x,
                          const double *y, const double *z, int64_t n, int32_t count, double max_distance, double *zg, float *hag,
                          uint8_t *m) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"ground", "query"};
    OBIA_TRY(refuse.n_or_none(n));
    if (ng < 1) { set_error("ground: query: the ground set must hold a point, got ng = %lld", (long long)ng); return OBIA_E_INVALID; }
    if (ng > (int64_t)INT_MAX) { set_error("ground: query: ng must be below 2^31, got %lld", (long long)ng); return OBIA_E_UNSUPPORTED; }
    Buffers b;
    b.in(gx).in(gy).in(gz).in(gidx).in(cell_start).in(x, n > 0).in(y, n > 0).in(z, OPTIONAL);
    if ((z == nullptr) != (hag == nullptr) || b.out(zg).out(hag, OPTIONAL).out(m, OPTIONAL).bad()) return refuse.buffers();
    if (count < 1 || count > OBIA_GROUND_MAX_COUNT) {
        set_error("ground: query: count must be in 1 .. %d, got %d", OBIA_GROUND_MAX_COUNT, count);
        return OBIA_E_INVALID;
    }
    if (!(max_distance >= 0.0)) { set_error("ground: query: max_distance must not be negative, got %g", max_distance); return OBIA_E_INVALID; }
    if (!(std::isfinite(side) && side > 0.0)) { set_error("ground: query: side must be finite and positive, got %g", side); return OBIA_E_INVALID; }
    const long long lim = 1ll << 30, cells = 4 * (long long)ng + 16;
    if (ncx < 1 || ncy < 1 || ncx > cells || ncy > cells / ncx || cx0 < -lim || cx0 > lim || cy0 < -lim || cy0 > lim) {
        set_error("ground: query: the grid must have 1 <= ncx * ncy <= 4 ng + 16 cells and an origin within +-2^30, got %lld x %lld at (%lld, %lld)",
                  (long long)ncx, (long long)ncy, (long long)cx0, (long long)cy0);
        return OBIA_E_INVALID;
    }
    if (n == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        GroundArgs A{};
        A.gx = gx; A.gy = gy; A.gz = gz; A.gidx = gidx; A.cell_start = cell_start;
        A.ncx = ncx; A.ncy = ncy; A.cx0 = cx0; A.cy0 = cy0; A.ng = (int)ng;
        A.side = side; A.md2 = max_distance * max_distance; A.limited = max_distance > 0.0 ? 1 : 0;
        A.x = x; A.y = y; A.z = z; A.n = n; A.zg = zg; A.hag = hag; A.m = m;
        switch (count) {
            case 1: launch_query<1>(ctx, A); break;
            case 2: launch_query<2>(ctx, A); break;
            case 3: launch_query<3>(ctx, A); break;
            case 4: launch_query<4>(ctx, A); break;
            case 5: launch_query<5>(ctx, A); break;
            case 6: launch_query<6>(ctx, A); break;
            case 7: launch_query<7>(ctx, A); break;
            default: launch_query<8>(ctx, A); break;
        }
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_ground_dtm_dev(obia_ctx *ctx, const double *x, const double *y, const double *z, int64_t n, const double *inv6, const float *dtm,
                        int H, int W, double *zg, float *hag) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"ground", "dtm"};
    OBIA_TRY(refuse.n_or_none(n));
    if (!inv6 || Buffers().in(x, n > 0).in(y, n > 0).in(z, n > 0).in(dtm).out(zg, OPTIONAL).out(hag).bad()) return refuse.buffers();
    if (H <= 0 || W <= 0) { set_error("ground: dtm: H and W must be positive, got %d x %d", H, W); return OBIA_E_INVALID; }
    if (n == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        const DtmArgs A{x, y, z, (long long)n, inv6[0], inv6[1], inv6[2], inv6[3], inv6[4], inv6[5], dtm, H, W, zg, hag};
        hipLaunchKernelGGL(ground_dtm_kernel, dim3(flat_grid(n)), dim3(256), 0, ctx->stream, A);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

}  // extern "C"
