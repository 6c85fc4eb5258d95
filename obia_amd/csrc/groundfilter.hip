// groundfilter.hip -- ground points of an unclassified cloud (include/obia_groundfilter.h): the cell minimum of a cloud, grey erosion /
// dilation of a plane with a square window, the threshold raster of a progressive morphological filter and the test of every point
// against it.  DESIGN.md 3.5u.
//
// A filter is two LINE PASSES, along the rows and then along the columns, and a line pass is a running maximum of unsigned keys: a
// value is loaded as the order key of v + 0.0f (common.hpp: zkey), complemented for a minimum, and an EMPTY cell (NaN) as 0, which
// lies below every key.  So one integer maximum serves erosion and dilation, +-inf stay data, and the NaN <-> empty conversion is
// part of the loads and stores.  The running maximum over 2r + 1 cells is two overlapping windows of 2^p cells, p = floor(log2(2r +
// 1)), built by doubling in LDS: m_j+1[i] = max(m_j[i], m_j[i + 2^j]) over the run and its 2r halo cells, then out[i] = max(m_p[i -
// r], m_p[i + r + 1 - 2^p]).  O(log r) per cell, no divergence, no dependence on the data.
//
//   rows     a workgroup of 256 owns OBIA_MORPH_ROW_TILE cells of one row; the doubling ping-pongs between two LDS lines.
//   columns  a workgroup of 1024 owns OBIA_MORPH_COL_LANES columns side by side (lanes are columns: every load and store of a wave is
//            two rows of 128 contiguous bytes) and OBIA_MORPH_COL_TILE rows; the doubling runs in place in one LDS tile (at most 382
//            rows of 32 keys, 48 KiB at radius 127, sized by the radius): every lane first reads its partners, at most 12, then all write.
//
// Nothing here takes memory from the context's workspace: every plane is the caller's.  Every atomic is an integer atomic.
#include "common.hpp"
#include "../../include/obia_groundfilter.h"

#include <climits>
#include <cmath>

namespace obia {
namespace {

constexpr int RT = OBIA_MORPH_ROW_TILE, CT = OBIA_MORPH_COL_TILE, CL = OBIA_MORPH_COL_LANES, RMAX = OBIA_MORPH_MAX_RADIUS;
constexpr int CTHREADS = 1024, CG = CTHREADS / CL;              // row groups of a column workgroup
constexpr int CQ = (CT + 2 * RMAX + CG - 1) / CG;               // rows of the tile one lane owns at the most
static_assert((CL & (CL - 1)) == 0 && CTHREADS % CL == 0 && RT % 256 == 0, "tile shapes");
static_assert((size_t)(CT + 2 * RMAX) * CL * 4 <= 64 * 1024 && (size_t)2 * (RT + 2 * RMAX) * 4 <= 64 * 1024, "a tile fits the LDS of a workgroup");

enum { OP_MIN = 0, OP_MAX = 1 };

__device__ __forceinline__ float quiet_nanf() { return __uint_as_float(0x7fc00000u); }

// the key of a cell: 0 when EMPTY, else the order key of v + 0.0f (no -0), complemented for a minimum: a larger key wins either way
template <int OP> __device__ __forceinline__ unsigned enc(float v) {
    v = v + 0.0f;
    if (v != v) return 0u;
    const unsigned k = zkey(v);
    return OP == OP_MIN ? ~k : k;
}
template <int OP> __device__ __forceinline__ float dec(unsigned k) {
    if (k == 0u) return quiet_nanf();
    return zunkey(OP == OP_MIN ? ~k : k);
}
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

template <int OP> __global__ __launch_bounds__(256) void morph_rows_kernel(const float *__restrict__ src, float *__restrict__ dst, int H, int W,
                                                                           int r, int p) {
    __shared__ unsigned line[2][RT + 2 * RMAX];
    const int x0 = (int)blockIdx.x * RT;
    const int len = W - x0 < RT ? W - x0 : RT;                   // cells of this run; with the halo: n
    const int n = len + 2 * r, off = 2 * r + 1 - (1 << p);
    for (int row = blockIdx.y; row < H; row += gridDim.y) {
        const float *s = src + (long long)row * W;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int gx = x0 - r + i;
            line[0][i] = (gx >= 0 && gx < W) ? enc<OP>(s[gx]) : 0u;
        }
        __syncthreads();
        int cur = 0;
        for (int j = 0; j < p; ++j) {
            const int step = 1 << j;
            for (int i = threadIdx.x; i < n; i += 256) line[cur ^ 1][i] = umax(line[cur][i], i + step < n ? line[cur][i + step] : 0u);
            __syncthreads();
            cur ^= 1;
        }
        float *d = dst + (long long)row * W + x0;
        for (int c = threadIdx.x; c < len; c += 256) d[c] = dec<OP>(umax(line[cur][c], line[cur][c + off]));
        __syncthreads();
    }
}

// FOLD (the last pass of a step of the threshold raster, a dilation): dst is the surface S, and thresh = min(thresh, S + dh) with
// EMPTY terms ignored; the first step has no earlier thresh to read
template <int OP, bool FOLD> __global__ __launch_bounds__(CTHREADS) void morph_cols_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                                                           int H, int W, int r, int p, float dh, int first,
                                                                                           float *__restrict__ thresh) {
    extern __shared__ unsigned tile[];                           // (CT + 2 r) rows of CL keys
    const int lx = threadIdx.x & (CL - 1), ly = threadIdx.x / CL;
    const long long gx = (long long)blockIdx.x * CL + lx;
    const bool col_in = gx < W;
    const int n_tiles = (H + CT - 1) / CT, off = 2 * r + 1 - (1 << p);
    for (int t = blockIdx.y; t < n_tiles; t += gridDim.y) {
        const int y0 = t * CT;
        const int len = H - y0 < CT ? H - y0 : CT;
        const int n = len + 2 * r;
        for (int i = ly; i < n; i += CG) {
            const int gy = y0 - r + i;
            tile[i * CL + lx] = (col_in && gy >= 0 && gy < H) ? enc<OP>(src[(long long)gy * W + gx]) : 0u;
        }
        __syncthreads();
        for (int j = 0; j < p; ++j) {
            const int step = 1 << j;
            unsigned partner[CQ];
#pragma unroll
            for (int q = 0; q < CQ; ++q) {
                const int i = ly + CG * q + step;
                partner[q] = i < n ? tile[i * CL + lx] : 0u;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < CQ; ++q) {
                const int i = ly + CG * q;
                if (i < n) tile[i * CL + lx] = umax(tile[i * CL + lx], partner[q]);
            }
            __syncthreads();
        }
        if (col_in)
            for (int c = ly; c < len; c += CG) {
                const float S = dec<OP>(umax(tile[c * CL + lx], tile[(c + off) * CL + lx]));
                const long long at = (long long)(y0 + c) * W + gx;
                dst[at] = S;
                if (FOLD) {
                    const float add = S + dh, old = first ? quiet_nanf() : thresh[at];
                    float T = (S != S) ? old : ((old != old) ? add : (old <= add ? old : add));
                    if (T != T) T = quiet_nanf();
                    thresh[at] = T;
                }
            }
        __syncthreads();
    }
}

struct Cloud {
    const double *x, *y, *z;
    long long n;
    double a, b, d, e, xoff, yoff;
    int H, W;
};

// flat pixel index of point i, -1 outside: THE PIXEL RULE, the arithmetic of pixel_of (points.hip); a NaN fails every comparison
__device__ __forceinline__ long long pixel_of(const Cloud &C, long long i) {
    const double X = C.x[i], Y = C.y[i];
    const double col = floor(C.a * X + C.b * Y + C.xoff), row = floor(C.d * X + C.e * Y + C.yoff);
    if (col >= 0.0 && col < (double)C.W && row >= 0.0 && row < (double)C.H) return (long long)row * C.W + (long long)col;
    return -1;
}

// the running minimum as a maximum of complemented keys, as raise_max of points.hip: the plain load may be stale, but a stale key is
// an earlier and so a smaller one, and then the atomic runs; most points of a populated cell cost a load instead of an atomic
__global__ __launch_bounds__(256) void gf_cell_min_kernel(Cloud C, unsigned *__restrict__ keys) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < C.n; i += (long long)gridDim.x * 256) {
        const long long px = pixel_of(C, i);
        if (px < 0) continue;
        const double z = C.z[i];
        if (!isfinite(z)) continue;
        const unsigned k = enc<OP_MIN>((float)z);
        if (keys[px] < k) atomicMax(&keys[px], k);
    }
}

__global__ __launch_bounds__(256) void gf_cell_min_finish_kernel(const unsigned *__restrict__ keys, long long npx, float *__restrict__ zmin) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npx; i += (long long)gridDim.x * 256) zmin[i] = dec<OP_MIN>(keys[i]);
}

__global__ __launch_bounds__(256) void gf_classify_kernel(Cloud C, const float *__restrict__ thresh, unsigned char *__restrict__ flags,
                                                          unsigned long long *__restrict__ counters) {
    __shared__ unsigned long long s_counters[4];
    if (threadIdx.x < 4) s_counters[threadIdx.x] = 0;
    __syncthreads();
    unsigned mine[4] = {0, 0, 0, 0};                            // of this lane: below 2^31 / 256
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < C.n; i += (long long)gridDim.x * 256) {
        const long long px = pixel_of(C, i);
        int what;
        if (px < 0) {
            what = 0;
        } else {
            const double z = C.z[i];
            if (!isfinite(z)) what = 1;
            else what = z <= (double)thresh[px] ? 3 : 2;         // a NaN threshold fails
        }
        flags[i] = what == 3 ? 1 : 0;
        mine[0] += what == 0; mine[1] += what == 1; mine[2] += what == 2; mine[3] += what == 3;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (mine[k]) atomicAdd(&s_counters[k], (unsigned long long)mine[k]);
    __syncthreads();
    if (threadIdx.x < 4 && s_counters[threadIdx.x]) atomicAdd(&counters[threadIdx.x], s_counters[threadIdx.x]);
}

int check_radius(const char *what, int r) {
    if (r < 1) { set_error("groundfilter: %s: a radius must be at least 1, got %d", what, r); return OBIA_E_INVALID; }
    if (r > RMAX) { set_error("groundfilter: %s: a radius must not exceed %d, got %d", what, RMAX, r); return OBIA_E_UNSUPPORTED; }
    return OBIA_OK;
}
Cloud cloud_of(const double *x, const double *y, const double *z, int64_t n, const double *t, int H, int W) {
    return Cloud{x, y, z, (long long)n, t[0], t[1], t[2], t[3], t[4], t[5], H, W};
}
int window_log2(int r) {                                         // p = floor(log2(2 r + 1))
    int p = 0;
    while ((2 << p) <= 2 * r + 1) ++p;
    return p;
}

// one line pass along the rows: src -> dst
void rows_pass(obia_ctx *ctx, int op, const float *src, float *dst, int H, int W, int r) {
    const dim3 grid = to_dim3(grids::morph_rows(H, W));
    if (op == OP_MIN) hipLaunchKernelGGL(morph_rows_kernel<OP_MIN>, grid, dim3(256), 0, ctx->stream, src, dst, H, W, r, window_log2(r));
    else hipLaunchKernelGGL(morph_rows_kernel<OP_MAX>, grid, dim3(256), 0, ctx->stream, src, dst, H, W, r, window_log2(r));
}
// ... and along the columns; thresh: the fold of a step of the threshold raster (a dilation)
void cols_pass(obia_ctx *ctx, int op, const float *src, float *dst, int H, int W, int r, float *thresh = nullptr, float dh = 0.0f, int first = 0) {
    const dim3 grid = to_dim3(grids::morph_cols(H, W));
    const size_t lds = (size_t)(CT + 2 * r) * CL * sizeof(unsigned);
    const int p = window_log2(r);
    if (thresh) hipLaunchKernelGGL((morph_cols_kernel<OP_MAX, true>), grid, dim3(CTHREADS), lds, ctx->stream, src, dst, H, W, r, p, dh, first, thresh);
    else if (op == OP_MIN) hipLaunchKernelGGL((morph_cols_kernel<OP_MIN, false>), grid, dim3(CTHREADS), lds, ctx->stream, src, dst, H, W, r, p, 0.0f, 0, thresh);
    else hipLaunchKernelGGL((morph_cols_kernel<OP_MAX, false>), grid, dim3(CTHREADS), lds, ctx->stream, src, dst, H, W, r, p, 0.0f, 0, thresh);
}

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_gf_cell_min_dev(obia_ctx *ctx, const double *x, const double *y, const double *z, int64_t n, const double *inv6, int H, int W,
                         uint32_t *keys) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"groundfilter", "cell min"};
    OBIA_TRY(refuse.n_or_none(n));
    if (!inv6 || Buffers().in(x, n > 0).in(y, n > 0).in(z, n > 0).out(keys).bad()) return refuse.buffers();
    OBIA_TRY(refuse.raster_below_2_31(H, W));
    if (n == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(gf_cell_min_kernel, to_dim3(grids::flat(n)), dim3(256), 0, ctx->stream, cloud_of(x, y, z, n, inv6, H, W), keys);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_gf_cell_min_finish_dev(obia_ctx *ctx, const uint32_t *keys, int H, int W, float *zmin) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"groundfilter", "cell min finish"};
    if (Buffers().out(zmin).in(keys).bad()) return refuse.buffers();
    OBIA_TRY(refuse.raster_below_2_31(H, W));
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        const long long npx = (long long)H * W;
        hipLaunchKernelGGL(gf_cell_min_finish_kernel, to_dim3(grids::flat(npx)), dim3(256), 0, ctx->stream, keys, npx, zmin);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_morph_filter_dev(obia_ctx *ctx, const float *src, int H, int W, int radius, int op, float *tmp, float *dst) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"groundfilter", "filter"};
    if (Buffers().out(dst).out(tmp).in(src).bad()) return refuse.buffers();
    OBIA_TRY(refuse.raster_below_2_31(H, W));
    if (op != OP_MIN && op != OP_MAX) { set_error("groundfilter: filter: op must be 0 (minimum) or 1 (maximum), got %d", op); return OBIA_E_INVALID; }
    OBIA_TRY(check_radius("filter", radius));
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        rows_pass(ctx, op, src, tmp, H, W, radius);
        OBIA_HIP_TRY(hipGetLastError());
        cols_pass(ctx, op, tmp, dst, H, W, radius);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_gf_threshold_dev(obia_ctx *ctx, const float *zmin, int H, int W, const int32_t *radii, const double *dh, int K, float *tmp0,
                          float *tmp1, float *surface, float *thresh) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"groundfilter", "threshold"};
    if (!radii || !dh || Buffers().out(surface).out(thresh).out(tmp0).out(tmp1).in(zmin).bad()) return refuse.buffers();
    OBIA_TRY(refuse.raster_below_2_31(H, W));
    if (K < 1 || K > OBIA_GF_MAX_STEPS) { set_error("groundfilter: threshold: K must be in 1 .. %d, got %d", OBIA_GF_MAX_STEPS, K); return OBIA_E_INVALID; }
    for (int k = 0; k < K; ++k) {
        OBIA_TRY(check_radius("threshold", radii[k]));
        if (!(std::isfinite(dh[k]) && dh[k] >= 0.0)) {
            set_error("groundfilter: threshold: dh[%d] must be finite and not negative, got %g", k, dh[k]);
            return OBIA_E_INVALID;
        }
    }
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        const float *S = zmin;
        for (int k = 0; k < K; ++k) {
            const int r = radii[k];
            rows_pass(ctx, OP_MIN, S, tmp0, H, W, r);
            cols_pass(ctx, OP_MIN, tmp0, tmp1, H, W, r);
            rows_pass(ctx, OP_MAX, tmp1, tmp0, H, W, r);
            cols_pass(ctx, OP_MAX, tmp0, surface, H, W, r, thresh, (float)dh[k], k == 0 ? 1 : 0);
            OBIA_HIP_TRY(hipGetLastError());
            S = surface;
        }
        return OBIA_OK;
    });
}

int obia_gf_classify_dev(obia_ctx *ctx, const double *x, const double *y, const double *z, int64_t n, const double *inv6,
                         const float *thresh, int H, int W, uint8_t *flags, uint64_t *counters) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"groundfilter", "classify"};
    OBIA_TRY(refuse.n_or_none(n));
    Buffers b;
    b.in(x, n > 0).in(y, n > 0).in(z, n > 0).in(thresh);
    if (!inv6 || b.out(flags, n > 0).out(counters).bad()) return refuse.buffers();
    OBIA_TRY(refuse.raster_below_2_31(H, W));
    if (n == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(gf_classify_kernel, to_dim3(grids::flat(n)), dim3(256), 0, ctx->stream, cloud_of(x, y, z, n, inv6, H, W), thresh, flags,
                           reinterpret_cast<unsigned long long *>(counters));
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

}  // extern "C"
