// rasterize.hip -- polygon rings -> label raster on gfx950 (the way back from segments.gpkg).
//
// Replaces rasterio.features.rasterize(shapes, fill=0, all_touched=False) of rasterise_slic_gpkg (obia/utils/cost.py:51-86).
// THE RULE (tests/rasterize_restatement.py states it in NumPy): everything in pixel coordinates, doubles, x = column
// axis, y = row axis, pixel (r, c) has its centre at (xc, yc) = (c + 0.5, r + 0.5).  A shape is a set of rings (every ring is closed
// by an edge from its last vertex back to its first); an edge (x0, y0) -> (x1, y1) COUNTS for a centre when
//     (y0 <= yc) != (y1 <= yc)   and   x0 + (yc - y0) * (x1 - x0) / (y1 - y0) <= xc
// (evaluated in this order, no FMA contraction: the Makefile compiles with -ffp-contract=off), and the shape covers the pixel iff an
// odd number of its edges count.  The pixel gets the value of the LAST shape in input order that covers it, else `fill`.
//
// The crossing abscissa of an edge on a row does not depend on the column, so no pixel is ever tested against an edge: an edge that
// counts on row r toggles the coverage of every column from  cs = the first column whose centre is >= the crossing  onwards, and the
// row's coverage is the prefix XOR of its toggles.  cs is decided with exact comparisons (floor(x), then x <= floor(x) + 0.5), so it
// is the rule above and not an approximation of it.  Two regimes:
//   * SMALL shapes (at most RS_MAX_EDGES edges, bounding box at most 64 x 64 pixel centres): one wave per shape, the edges staged
//     in LDS, lane = row of the bounding box, the row's 64 toggles in two 32-bit registers; after the prefix XOR the row masks go
//     through LDS so that lane = column for the stores.
//   * LARGE shapes: the bounding box is cut into bands of RL_BAND_ROWS rows, every edge is listed in the bands its y-range meets
//     (count, allocate, fill -- the order inside a list does not matter, toggles commute), and one workgroup per band and
//     RL_TILE_W columns collects the toggles of its band's edges in an LDS bit plane.
// "Last shape wins" is an atomicMax of the shape index into the plane pre-filled with -1 -- the same plane in any schedule -- and a
// last pass maps index -> value or fill.  All stores are plain vector stores / vector atomics.
#include <algorithm>

#include "slic.hpp"

namespace obia {

#ifndef OBIA_RAST_SMALL_EDGES
// Edges a shape may have and still take the one-wave path: 4 waves x 256 edges x 32 B = 32 KiB of LDS per workgroup, four
// workgroups per CU (the compiler's report: 4 waves per SIMD).  The segments of the tiler have a few dozen edges, so the limit
// decides nothing at BASELINE configs[2]; a lower one (more workgroups per CU) has not been timed yet -- build
// with -DOBIA_RAST_SMALL_EDGES=n and load the result through OBIA_HIP_LIB to try one.
#define OBIA_RAST_SMALL_EDGES 256
#endif
constexpr int RS_MAX_EDGES = OBIA_RAST_SMALL_EDGES;
constexpr int RS_SIDE = 64;          // rows = lanes, columns = bits of two 32-bit words
constexpr int RS_WAVES = 4;
constexpr int RL_BAND_ROWS = 8;
constexpr int RL_TILE_W = grids::RAST_LARGE_TILE_W;      // columns of one workgroup's bit plane: 8 rows x 64 words = 2 KiB of LDS
constexpr int RL_WORDS = RL_TILE_W / 32;

struct RastLarge { int s, r0, r1, c0, c1, vlo, nv, ring_lo, ring_hi; long long band_base; };
enum { RC_LARGE = 0, RC_BANDS = 1, RC_MAX_NV = 2, RC_MAX_W = 3, RC_ENTRIES = 4, RC_BAD = 5, RC_N = 6 };

// first row (column) whose centre r + 0.5 is >= y, clamped to [-2, 2^31): exact comparisons only
__device__ __forceinline__ int first_centre_ge(double y) {
    const double yc = fmin(fmax(y, -2.0), 2147483000.0);
    const double f = floor(yc);
    return (int)f + ((f + 0.5 < yc) ? 1 : 0);
}

__device__ __forceinline__ bool edge_counts(double y0, double y1, double yc) { return (y0 <= yc) != (y1 <= yc); }
__device__ __forceinline__ double edge_crossing(double x0, double y0, double x1, double y1, double yc) {
    return x0 + (yc - y0) * (x1 - x0) / (y1 - y0);
}

// ---- ring table: checks, and the first ring of every shape ------------------------------------------------------------------------
// ring_shape is non-decreasing, so shape s owns rings [start[s], start[s + 1]); a shape without rings gets an empty range
__global__ __launch_bounds__(256) void rast_ring_table_kernel(const int64_t *__restrict__ ring_offset, const int32_t *__restrict__ ring_shape,
                                                              long long R, int S, int *__restrict__ start,
                                                              unsigned long long *__restrict__ ctr) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int prev = r == 0 ? -1 : ring_shape[r - 1], cur = ring_shape[r];
    const int64_t a = ring_offset[r], b = ring_offset[r + 1];
    if (prev < -1 || cur < prev || cur < 0 || cur >= S || a < 0 || b < a || (r == 0 && a != 0)) { atomicAdd(&ctr[RC_BAD], 1ull); return; }
    for (int s = prev + 1; s <= cur; ++s) start[s] = (int)r;
    if (r == R - 1)
        for (int s = cur + 1; s <= S; ++s) start[s] = (int)R;
}

// ---- small shapes (and the plan of the large ones) -----------------------------------------------------------------------------
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ uint32_t prefix_xor32(uint32_t w) {
    w ^= w << 1; w ^= w << 2; w ^= w << 4; w ^= w << 8; w ^= w << 16;
    return w;
}

__global__ __launch_bounds__(RS_WAVES * 64) void rast_small_kernel(const double2 *__restrict__ xy, const int64_t *__restrict__ ring_offset,
                                                                   const int *__restrict__ start, int S, int H, int W,
                                                                   int32_t *__restrict__ out, RastLarge *__restrict__ large,
                                                                   unsigned long long *__restrict__ ctr) {
    __shared__ double4 s_edge[RS_WAVES][RS_MAX_EDGES];
    __shared__ uint2 s_mask[RS_WAVES][RS_SIDE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long sl = (long long)blockIdx.x * RS_WAVES + wv;
    const bool valid = sl < S;
    const int s = valid ? (int)sl : 0;
    int ring_lo = 0, ring_hi = 0, vlo = 0, nv = 0;
    if (valid) {
        ring_lo = start[s];
        ring_hi = start[s + 1];
        vlo = (int)ring_offset[ring_lo];
        nv = (int)ring_offset[ring_hi] - vlo;
    }
    nv = __builtin_amdgcn_readfirstlane(nv);
    const bool stage = nv <= RS_MAX_EDGES;
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int r = ring_lo; r < ring_hi; ++r) {
        const int a = (int)ring_offset[r], b = (int)ring_offset[r + 1];
        for (int i = a + lane; i < b; i += 64) {
            const double2 p = xy[i];
            xmin = fmin(xmin, p.x); xmax = fmax(xmax, p.x);
            ymin = fmin(ymin, p.y); ymax = fmax(ymax, p.y);
            if (stage) {
                const double2 q = xy[i + 1 < b ? i + 1 : a];     // the last vertex is joined to the first
                s_edge[wv][i - vlo] = make_double4(p.x, p.y, q.x, q.y);
            }
        }
    }
    xmin = wave_min(xmin); ymin = wave_min(ymin); xmax = wave_max(xmax); ymax = wave_max(ymax);
    // rows whose centre lies in [ymin, ymax); columns from the first centre >= xmin to the last centre < xmax, one more on either
    // side because a crossing is a rounded value and may leave [xmin, xmax] by an ulp
    int r0 = 0, r1 = -1, c0 = 0, c1 = -1;
    if (nv > 0) {
        r0 = max(first_centre_ge(ymin), 0);
        r1 = min(first_centre_ge(ymax) - 1, H - 1);
        c0 = max(first_centre_ge(xmin) - 1, 0);
        c1 = min(first_centre_ge(xmax), W - 1);
    }
    const bool some = r0 <= r1 && c0 <= c1;
    const bool small = some && stage && r1 - r0 < RS_SIDE && c1 - c0 < RS_SIDE;
    if (some && !small && lane == 0) {
        const unsigned long long l = atomicAdd(&ctr[RC_LARGE], 1ull);
        RastLarge L;
        L.s = s; L.r0 = r0; L.r1 = r1; L.c0 = c0; L.c1 = c1; L.vlo = vlo; L.nv = nv; L.ring_lo = ring_lo; L.ring_hi = ring_hi;
        L.band_base = (long long)atomicAdd(&ctr[RC_BANDS], (unsigned long long)((r1 - r0) / RL_BAND_ROWS + 1));
        atomicMax(&ctr[RC_MAX_NV], (unsigned long long)nv);
        atomicMax(&ctr[RC_MAX_W], (unsigned long long)(c1 - c0 + 1));
        large[l] = L;
    }
    __syncthreads();                                            // the staged edges are visible to every lane
    uint32_t lo = 0, hi = 0;
    if (small && r0 + lane <= r1) {
        const double yc = (double)(r0 + lane) + 0.5;
        const double left = (double)c0 + 0.5, beyond = (double)c0 + (RS_SIDE - 0.5);
        for (int e = 0; e < nv; ++e) {
            const double4 E = s_edge[wv][e];
            if (!edge_counts(E.y, E.w, yc)) continue;
            const double x = edge_crossing(E.x, E.y, E.z, E.w, yc);
            int bit;
            if (x <= left) bit = 0;
            else if (x > beyond) continue;                       // first toggled column is past the 64th
            else {
                const double f = floor(x);
                bit = (int)f - c0 + ((x <= f + 0.5) ? 0 : 1);
            }
            if (bit < 32) lo ^= 1u << bit;
            else if (bit < 64) hi ^= 1u << (bit - 32);
        }
        lo = prefix_xor32(lo);
        hi = prefix_xor32(hi);
        if (lo >> 31) hi = ~hi;
    }
    s_mask[wv][lane] = make_uint2(lo, hi);
    __syncthreads();
    if (small) {
        const int c = c0 + lane;
        for (int j = 0; j <= r1 - r0; ++j) {
            const uint2 m = s_mask[wv][j];
            const uint32_t w = lane < 32 ? m.x : m.y;
            if (((w >> (lane & 31)) & 1u) && c <= c1) atomicMax(&out[(long long)(r0 + j) * W + c], s);
        }
    }
}

// ---- large shapes: band lists ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rast_band_owner_kernel(const RastLarge *__restrict__ large, int *__restrict__ band_owner) {
    const RastLarge L = large[blockIdx.x];
    const int nb = (L.r1 - L.r0) / RL_BAND_ROWS + 1;
    for (int j = threadIdx.x; j < nb; j += blockDim.x) band_owner[L.band_base + j] = (int)blockIdx.x;
}

// COUNT: band_n[b] = edges whose rows meet band b.  FILL: the same walk writes (vertex, next vertex) into the band's slice.
template <bool FILL>
__global__ __launch_bounds__(256) void rast_band_bin_kernel(const double2 *__restrict__ xy, const int64_t *__restrict__ ring_offset,
                                                            const RastLarge *__restrict__ large, int *__restrict__ band_n,
                                                            const long long *__restrict__ band_off, int2 *__restrict__ entries) {
    const RastLarge L = large[blockIdx.x];
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < L.nv; i += gridDim.y * blockDim.x) {
        const int v = L.vlo + i;
        int lo = L.ring_lo, hi = L.ring_hi;                      // ring_offset[lo] <= v < ring_offset[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (ring_offset[mid] <= v) lo = mid; else hi = mid;
        }
        const int a = (int)ring_offset[lo], b = (int)ring_offset[lo + 1];
        const int j = v + 1 < b ? v + 1 : a;
        const double y0 = xy[v].y, y1 = xy[j].y;
        // the edge counts on the rows whose centre lies in [min(y0, y1), max(y0, y1))
        const int ra = max(first_centre_ge(fmin(y0, y1)), L.r0), rb = min(first_centre_ge(fmax(y0, y1)) - 1, L.r1);
        if (ra > rb) continue;
        for (int k = (ra - L.r0) / RL_BAND_ROWS; k <= (rb - L.r0) / RL_BAND_ROWS; ++k) {
            const long long band = L.band_base + k;
            const int at = atomicAdd(&band_n[band], 1);
            if (FILL) entries[band_off[band] + at] = make_int2(v, j);
        }
    }
}

// slice of every band in the entry array; the order of the slices is whatever the atomics give -- nothing reads across slices
__global__ __launch_bounds__(256) void rast_band_alloc_kernel(int *__restrict__ band_n, long long n_bands, long long *__restrict__ band_off,
                                                              unsigned long long *__restrict__ ctr) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bands) return;
    band_off[b] = (long long)atomicAdd(&ctr[RC_ENTRIES], (unsigned long long)band_n[b]);
}

__global__ __launch_bounds__(256) void rast_large_kernel(const double2 *__restrict__ xy, const RastLarge *__restrict__ large,
                                                         const int *__restrict__ band_owner, const int *__restrict__ band_n,
                                                         const long long *__restrict__ band_off, const int2 *__restrict__ entries,
                                                         int W, int32_t *__restrict__ out) {
    __shared__ uint32_t s_bits[RL_BAND_ROWS][RL_WORDS];
    __shared__ uint32_t s_carry[RL_BAND_ROWS];
    const long long band = blockIdx.x;
    const RastLarge L = large[band_owner[band]];
    const int br0 = L.r0 + (int)(band - L.band_base) * RL_BAND_ROWS;
    const int rows = min(RL_BAND_ROWS, L.r1 - br0 + 1);
    const int n = band_n[band];
    const int2 *__restrict__ ent = entries + band_off[band];
    const int n_tiles = (L.c1 - L.c0) / RL_TILE_W + 1;
    for (int tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const int tc0 = L.c0 + tile * RL_TILE_W;
        const double left = (double)tc0 + 0.5, beyond = (double)tc0 + (RL_TILE_W - 0.5);
        __syncthreads();                                         // the previous tile's stores have read the plane
        for (int i = threadIdx.x; i < RL_BAND_ROWS * RL_WORDS; i += blockDim.x) (&s_bits[0][0])[i] = 0;
        if (threadIdx.x < RL_BAND_ROWS) s_carry[threadIdx.x] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int2 e = ent[i];
            const double2 p = xy[e.x], q = xy[e.y];
            for (int k = 0; k < rows; ++k) {
                const double yc = (double)(br0 + k) + 0.5;
                if (!edge_counts(p.y, q.y, yc)) continue;
                const double x = edge_crossing(p.x, p.y, q.x, q.y, yc);
                if (x <= left) atomicXor(&s_carry[k], 1u);       // toggles the whole tile
                else if (!(x > beyond)) {
                    const double f = floor(x);
                    const int rel = (int)f - tc0 + ((x <= f + 0.5) ? 0 : 1);
                    if (rel < RL_TILE_W) atomicXor(&s_bits[k][rel >> 5], 1u << (rel & 31));
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < RL_BAND_ROWS * RL_WORDS; i += blockDim.x) (&s_bits[0][0])[i] = prefix_xor32((&s_bits[0][0])[i]);
        __syncthreads();
        if (threadIdx.x < rows) {                                // carry the parity from word to word along the row
            uint32_t c = s_carry[threadIdx.x] & 1u;
            for (int w = 0; w < RL_WORDS; ++w) {
                const uint32_t v = s_bits[threadIdx.x][w];
                s_bits[threadIdx.x][w] = c ? ~v : v;
                c ^= v >> 31;
            }
        }
        __syncthreads();
        for (int k = 0; k < rows; ++k)
            for (int col = threadIdx.x; col < RL_TILE_W; col += blockDim.x) {
                const int c = tc0 + col;
                if (c <= L.c1 && ((s_bits[k][col >> 5] >> (col & 31)) & 1u)) atomicMax(&out[(long long)(br0 + k) * W + c], L.s);
            }
    }
}

// ---- shape index -> value ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rast_value_kernel(int32_t *__restrict__ out, long long n, const int32_t *__restrict__ shape_value,
                                                         int32_t fill) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int s = out[i];
        out[i] = s < 0 ? fill : shape_value[s];
    }
}

static long long g_last_small = 0, g_last_large = 0;

int rasterize_polygons_dev(obia_ctx *ctx, const double *xy_pix, const int64_t *ring_offset, int64_t n_rings, const int32_t *ring_shape,
                           const int32_t *shape_value, int64_t n_shapes, int H, int W, int32_t fill, int32_t *out) {
    if (H <= 0 || W <= 0 || !out) { set_error("rasterize: bad output raster"); return OBIA_E_INVALID; }
    if (n_rings < 0 || n_shapes < 0) { set_error("rasterize: negative ring or shape count"); return OBIA_E_INVALID; }
    const long long n = (long long)H * W;
    if (n >= 0x80000000LL) { set_error("rasterize: raster of %lld pixels, the limit is 2^31 - 1", n); return OBIA_E_UNSUPPORTED; }
    if (n_shapes >= 0x80000000LL || n_rings >= 0x80000000LL) {
        set_error("rasterize: %lld shapes / %lld rings, the limit is 2^31 - 1", (long long)n_shapes, (long long)n_rings);
        return OBIA_E_UNSUPPORTED;
    }
    if (n_rings > 0 && (!xy_pix || !ring_offset || !ring_shape || !shape_value || n_shapes == 0)) {
        set_error("rasterize: rings without vertex, offset, shape or value table");
        return OBIA_E_INVALID;
    }
    g_last_small = g_last_large = 0;
    const int S = (int)n_shapes;
    OBIA_HIP_TRY(hipMemsetAsync(out, 0xff, (size_t)n * sizeof(int32_t), ctx->stream));      // every pixel: shape index -1
    const int g_px = (int)grids::rast_value(n).x.n;
    if (n_rings > 0) {
        Arena &A = ctx->arena;
        unsigned long long *ctr = A.get<unsigned long long>(RC_N);
        int *start = A.get<int>((size_t)S + 1);
        RastLarge *large = A.get<RastLarge>((size_t)S);
        if (!ctr || !start || !large) return OBIA_E_NOMEM;
        OBIA_HIP_TRY(hipMemsetAsync(ctr, 0, RC_N * sizeof(unsigned long long), ctx->stream));
        hipLaunchKernelGGL(rast_ring_table_kernel, dim3(cdiv(n_rings, 256)), dim3(256), 0, ctx->stream, ring_offset, ring_shape,
                           (long long)n_rings, S, start, ctr);
        unsigned long long bad = 0;
        int64_t V = 0;
        OBIA_TRY(read_back(ctx, &bad, ctr + RC_BAD, sizeof(bad)));
        OBIA_TRY(read_back(ctx, &V, ring_offset + n_rings, sizeof(V)));
        debug_sync(ctx, "rasterize: ring table");
        if (bad) {
            set_error("rasterize: ring_offset must start at 0 and not decrease, ring_shape must not decrease and lie in [0, n_shapes)");
            return OBIA_E_INVALID;
        }
        if (V >= 0x80000000LL) { set_error("rasterize: %lld vertices, the limit is 2^31 - 1", (long long)V); return OBIA_E_UNSUPPORTED; }
        const double2 *xy = reinterpret_cast<const double2 *>(xy_pix);
        hipLaunchKernelGGL(rast_small_kernel, dim3(cdiv(S, RS_WAVES)), dim3(RS_WAVES * 64), 0, ctx->stream, xy, ring_offset, start, S, H, W,
                           out, large, ctr);
        unsigned long long h[RC_N];
        OBIA_TRY(read_back(ctx, h, ctr, sizeof(h)));
        debug_sync(ctx, "rasterize: small shapes");
        const long long n_large = (long long)h[RC_LARGE], n_bands = (long long)h[RC_BANDS];
        g_last_large = n_large;
        g_last_small = S - n_large;
        if (n_large > 0) {
            if (n_bands >= 0x7fffffffLL) { set_error("rasterize: %lld row bands of large shapes", n_bands); return OBIA_E_UNSUPPORTED; }
            int *band_owner = A.get<int>((size_t)n_bands);
            int *band_n = A.get<int>((size_t)n_bands);
            long long *band_off = A.get<long long>((size_t)n_bands);
            if (!band_owner || !band_n || !band_off) return OBIA_E_NOMEM;
            OBIA_HIP_TRY(hipMemsetAsync(band_n, 0, (size_t)n_bands * sizeof(int), ctx->stream));
            const dim3 g_bin = to_dim3(grids::rast_band_bin(n_large, (long long)h[RC_MAX_NV]));
            hipLaunchKernelGGL(rast_band_owner_kernel, dim3((unsigned)n_large), dim3(256), 0, ctx->stream, large, band_owner);
            hipLaunchKernelGGL(rast_band_bin_kernel<false>, g_bin, dim3(256), 0, ctx->stream, xy, ring_offset, large, band_n, band_off,
                               (int2 *)nullptr);
            hipLaunchKernelGGL(rast_band_alloc_kernel, dim3(cdiv(n_bands, 256)), dim3(256), 0, ctx->stream, band_n, n_bands, band_off, ctr);
            unsigned long long n_ent = 0;
            OBIA_TRY(read_back(ctx, &n_ent, ctr + RC_ENTRIES, sizeof(n_ent)));
            debug_sync(ctx, "rasterize: band counts");
            if (n_ent > 0) {
                int2 *entries = A.get<int2>((size_t)n_ent);
                if (!entries) return OBIA_E_NOMEM;
                OBIA_HIP_TRY(hipMemsetAsync(band_n, 0, (size_t)n_bands * sizeof(int), ctx->stream));
                hipLaunchKernelGGL(rast_band_bin_kernel<true>, g_bin, dim3(256), 0, ctx->stream, xy, ring_offset, large, band_n, band_off,
                                   entries);
                debug_sync(ctx, "rasterize: band lists");
                const dim3 g_large = to_dim3(grids::rast_large(n_bands, (long long)h[RC_MAX_W]));
                hipLaunchKernelGGL(rast_large_kernel, g_large, dim3(256), 0, ctx->stream, xy, large, band_owner, band_n, band_off, entries, W,
                                   out);
                debug_sync(ctx, "rasterize: large shapes");
            }
        }
    }
    hipLaunchKernelGGL(rast_value_kernel, dim3(g_px), dim3(256), 0, ctx->stream, out, n, shape_value, fill);
    OBIA_HIP_TRY(hipGetLastError());
    debug_sync(ctx, "rasterize: values");
    return OBIA_OK;
}

}  // namespace obia

using namespace obia;

extern "C" {

int obia_rasterize_polygons_dev(obia_ctx *ctx, const double *xy_pix, const int64_t *ring_offset, int64_t n_rings,
                                const int32_t *ring_shape, const int32_t *shape_value, int64_t n_shapes, int H, int W, int32_t fill,
                                int32_t *out_hw) {
    OBIA_TRY(enter(ctx));
    return call_frame(ctx, FRAME_PLAIN, [&] {
        return rasterize_polygons_dev(ctx, xy_pix, ring_offset, n_rings, ring_shape, shape_value, n_shapes, H, W, fill, out_hw);
    });
}

int obia_rasterize_info(int64_t info[4]) {
    if (!info) { set_error("null pointer argument"); return OBIA_E_INVALID; }
    info[0] = g_last_small;
    info[1] = g_last_large;
    info[2] = RS_MAX_EDGES;
    info[3] = RS_SIDE;
    return OBIA_OK;
}

}  // extern "C"
