// sharpness.hip -- the sharpness raster (include/obia_sharpness.h): per-band min / max, normalise + grey + 3 x 3 Laplacian in one
// stencil pass, SciPy's running-sum box filter along both axes (alone, or for lap and lap * lap together with the variance written by the
// second pass), and the float32 percentile stretch.  DESIGN.md 3.5n.
//
// The box filter is a SERIAL recurrence in double along every line (scipy.ndimage.uniform_filter1d): its bits depend on the order of
// the additions as soon as the data's range exceeds what a double holds exactly, so one lane owns one line from its first sample to its
// last and carries the running sum in a register.  Parallelism is across lines only -- a 16384^2 plane has 256 waves of them --, so
// the kernels hide latency by issuing many independent loads before the dependent adds, not by occupancy:
//   axis 0 (box_cols_kernel): lanes are consecutive columns, every load and store is coalesced as it is; the row loop is unrolled.
//   axis 1 (box_rows_kernel): a lane owns a row, W floats from its neighbour.  Only the additions are serial: the division by win and
//     the rounding are independent per sample.  So a workgroup of four waves takes a band of 64 rows and moves along it in chunks of
//     columns: four waves load the chunk into LDS, coalesced, one wave walks it (a lane per row) and leaves the running sums there, four
//     waves divide, round and store coalesced.
// Every access is one float wide: the planes need no more than 4-byte alignment.
#include "common.hpp"
#include "../../include/obia_sharpness.h"

#include <algorithm>
#include <climits>

namespace obia {
namespace {

constexpr int MM_GRID = grids::SHARPNESS_MINMAX_PARTS;      // workgroups (at most) of the min / max pass: one partial record of six floats each
constexpr int LAP_TX = 64, LAP_TY = 32;   // output tile of one stencil workgroup (256 threads, 8 rows each)
constexpr int BOX_ROWS = 64;       // rows of one axis-1 workgroup: four waves, the first walks a lane per row
constexpr int BOX_CH1 = 64;        // columns per LDS chunk, one plane (box filter):  64 x 65 cells of 8 bytes = 32.5 KiB
constexpr int BOX_CH2 = 32;        // ... two planes (variance):                      2 x 64 x 33 cells        = 33 KiB
constexpr int BOX_UNROLL = 16;     // rows of axis 0 whose loads are issued together

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// BORDER_REFLECT_101 for p in [-1, n]; anything further out (a tile's overhang, never used) is clamped into the line
__device__ __forceinline__ int reflect101(long long p, int n) {
    if (p < 0) p = -p;
    if (p >= n) p = 2LL * (n - 1) - p;
    return (int)(p < 0 ? 0 : (p >= n ? n - 1 : p));
}

// SciPy's `reflect` (d c b a | a b c d | d c b a): period 2 n, any i
__device__ __forceinline__ int reflect_sym(long long i, int n) {
    const long long period = 2LL * n;
    long long m = i % period;
    if (m < 0) m += period;
    return (int)(m < n ? m : period - 1 - m);
}

// sum of a wave's 64 values in lane 0
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// ---------------------------------------------------------------------------------------------------------- band min / max
// partial record of workgroup g: part[6 g + b] = min of band b, part[6 g + 3 + b] = max of band b
__global__ __launch_bounds__(256) void band_minmax_kernel(const float *__restrict__ raster, long long npx, int C, int b0, int b1, int b2,
                                                          float *__restrict__ part, unsigned long long *__restrict__ bad) {
    __shared__ float s_v[4][6];
    const int band[3] = {b0, b1, b2};
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned nbad = 0;
    for (long long px = (long long)blockIdx.x * 256 + threadIdx.x; px < npx; px += (long long)gridDim.x * 256) {
        const float *p = raster + px * C;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float v = p[band[b]];
            nbad += finite_f(v) ? 0u : 1u;
            mn[b] = v < mn[b] ? v : mn[b];
            mx[b] = v > mx[b] ? v : mx[b];
        }
    }
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float a = __shfl_down(mn[b], off), c = __shfl_down(mx[b], off);
            mn[b] = a < mn[b] ? a : mn[b];
            mx[b] = c > mx[b] ? c : mx[b];
        }
    nbad = wave_sum(nbad);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            s_v[wave][b] = mn[b];
            s_v[wave][3 + b] = mx[b];
        }
        if (nbad) atomicAdd(bad, (unsigned long long)nbad);
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float r = s_v[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) {
            const float v = s_v[w][threadIdx.x];
            r = threadIdx.x < 3 ? (v < r ? v : r) : (v > r ? v : r);
        }
        part[6 * blockIdx.x + threadIdx.x] = r;
    }
}

// stats[b] = mn of band b, stats[3 + b] = rng = (max - mn) + 1e-8f.  Six waves: wave w reduces component w of the partial records.
__global__ __launch_bounds__(384) void band_stats_kernel(const float *__restrict__ part, int nparts, float *__restrict__ stats) {
    __shared__ float s_r[6];
    const int lane = threadIdx.x & 63, comp = threadIdx.x >> 6;
    const bool is_min = comp < 3;
    float r = is_min ? INFINITY : -INFINITY;
    for (int g = lane; g < nparts; g += 64) {
        const float v = part[6 * g + comp];
        r = is_min ? (v < r ? v : r) : (v > r ? v : r);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float v = __shfl_down(r, off);
        r = is_min ? (v < r ? v : r) : (v > r ? v : r);
    }
    if (lane == 0) s_r[comp] = r;
    __syncthreads();
    if (threadIdx.x < 3) {
        stats[threadIdx.x] = s_r[threadIdx.x];
        stats[3 + threadIdx.x] = (s_r[3 + threadIdx.x] - s_r[threadIdx.x]) + 1e-8f;
    }
}

// ------------------------------------------------------------------------------------------- normalise + grey + Laplacian
// One workgroup: a tile of LAP_TY x LAP_TX outputs.  The grey values of the tile and of a border of one pixel (REFLECT_101 at the
// raster's edges) are computed once into LDS; RASTER: from the three bands of the (H, W, C) raster and their statistics, else they are
// the plane `src` itself (and the non-finite ones among the tile's own pixels are counted).
template <bool RASTER>
__global__ __launch_bounds__(256) void laplacian_kernel(const float *__restrict__ src, int H, int W, int C, int b0, int b1, int b2,
                                                        const float *__restrict__ stats, int ntx, float *__restrict__ lap,
                                                        unsigned long long *__restrict__ bad) {
    __shared__ float s_g[LAP_TY + 2][LAP_TX + 2];
    const long long y0 = (long long)(blockIdx.x / ntx) * LAP_TY, x0 = (long long)(blockIdx.x % ntx) * LAP_TX;
    float mn[3] = {0, 0, 0}, rng[3] = {1, 1, 1};
    if (RASTER) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            mn[b] = stats[b];
            rng[b] = stats[3 + b];
        }
    }
    unsigned nbad = 0;
    for (int i = threadIdx.x; i < (LAP_TY + 2) * (LAP_TX + 2); i += 256) {
        const int ry = i / (LAP_TX + 2), rx = i - ry * (LAP_TX + 2);
        const int gy = reflect101(y0 - 1 + ry, H), gx = reflect101(x0 - 1 + rx, W);
        const long long px = (long long)gy * W + gx;
        float g;
        if (RASTER) {
            const float *p = src + px * C;
            const float v0 = (p[b0] - mn[0]) / rng[0], v1 = (p[b1] - mn[1]) / rng[1], v2 = (p[b2] - mn[2]) / rng[2];
            g = (v0 * 0.299f + v1 * 0.587f) + v2 * 0.114f;
        } else {
            g = src[px];
            const bool own = ry >= 1 && ry <= LAP_TY && rx >= 1 && rx <= LAP_TX && y0 - 1 + ry < H && x0 - 1 + rx < W;
            nbad += (own && !finite_f(g)) ? 1u : 0u;
        }
        s_g[ry][rx] = g;
    }
    if (!RASTER && bad) {
        nbad = wave_sum(nbad);
        if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, (unsigned long long)nbad);
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const long long x = x0 + tx;
    if (x >= W) return;
#pragma unroll
    for (int k = 0; k < LAP_TY / 4; ++k) {
        const int r = ty + 4 * k;
        const long long y = y0 + r;
        if (y >= H) break;
        const float a = s_g[r][tx], b = s_g[r][tx + 2], c = s_g[r + 1][tx + 1], d = s_g[r + 2][tx], e = s_g[r + 2][tx + 2];
        lap[y * W + x] = (((2.0f * a + 2.0f * b) + (-8.0f * c)) + 2.0f * d) + 2.0f * e;
    }
}

// ------------------------------------------------------------------------------------------------------------- flat pass
// The two rare flat passes over a plane, one kernel: `bad` != NULL counts the non-finite values of x (the box filter's input check);
// `out` != NULL writes the variance at win = 1, where mean = x and mean2 = (float)(x * x): out = mean2 - (float)(mean * mean).
__global__ __launch_bounds__(256) void flat_pass_kernel(const float *__restrict__ x, long long n, float *__restrict__ out,
                                                        unsigned long long *__restrict__ bad) {
    unsigned nbad = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = x[i];
        nbad += finite_f(v) ? 0u : 1u;
        if (out) {
            const float sq = v * v;
            out[i] = sq - sq;
        }
    }
    if (bad) {
        nbad = wave_sum(nbad);
        if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, (unsigned long long)nbad);
    }
}

// ------------------------------------------------------------------------------------------------------- LDS cells, axis 1
// One 8-byte cell per (row, column) of a chunk: first the pair {leading sample, trailing sample} as two floats, then -- written by the
// lane that has consumed the pair -- the running sum as a double.
__device__ __forceinline__ unsigned long long pack_pair(float lead, float trail) {
    return (unsigned long long)__float_as_uint(lead) | ((unsigned long long)__float_as_uint(trail) << 32);
}
__device__ __forceinline__ float pair_lead(unsigned long long c) { return __uint_as_float((unsigned)c); }
__device__ __forceinline__ float pair_trail(unsigned long long c) { return __uint_as_float((unsigned)(c >> 32)); }
__device__ __forceinline__ unsigned long long sum_cell(double t) { return (unsigned long long)__double_as_longlong(t); }
__device__ __forceinline__ double cell_sum(unsigned long long c) { return __longlong_as_double((long long)c); }

// ------------------------------------------------------------------------------------------------------ box filter, axis 0
// One wave, one lane per column, rows 0 .. H - 1: every load and store is coalesced as it is, and each lane divides for itself.  VAR:
// the input is lap; the recurrences of lap (-> out0) and of (float)(lap * lap) (-> out1) run together.  Rows s1 + 1 .. H - s2 - 1 need
// no reflection: there BOX_UNROLL rows are loaded before the first dependent add.
template <bool VAR>
__global__ __launch_bounds__(64) void box_cols_kernel(const float *__restrict__ in, int H, int W, int win, float *__restrict__ out0,
                                                      float *__restrict__ out1) {
    const long long col = (long long)blockIdx.x * 64 + threadIdx.x;
    if (col >= W) return;
    const float *p = in + col;
    float *q0 = out0 + col, *q1 = VAR ? out1 + col : nullptr;
    const long long s1 = win / 2, s2 = win - s1 - 1, n = H;
    const double dwin = (double)win;
    double t0 = 0.0, t1 = 0.0;
    for (long long l = -s1; l <= s2; ++l) {
        const float v = p[(long long)reflect_sym(l, H) * W];
        t0 += (double)v;
        if (VAR) t1 += (double)(v * v);
    }
    q0[0] = (float)(t0 / dwin);
    if (VAR) q1[0] = (float)(t1 / dwin);
    const long long i0 = std::min(n, s1 + 1), i1 = std::max(i0, n - s2);
    long long ll = 1;
    auto reflected = [&](long long to) {
        for (; ll < to; ++ll) {
            const float a = p[(long long)reflect_sym(ll + s2, H) * W], b = p[(long long)reflect_sym(ll - s1 - 1, H) * W];
            t0 += ((double)a - (double)b);
            q0[ll * W] = (float)(t0 / dwin);
            if (VAR) {
                t1 += ((double)(a * a) - (double)(b * b));
                q1[ll * W] = (float)(t1 / dwin);
            }
        }
    };
    reflected(i0);
    for (; ll + BOX_UNROLL <= i1; ll += BOX_UNROLL) {
        float a[BOX_UNROLL], b[BOX_UNROLL];
#pragma unroll
        for (int u = 0; u < BOX_UNROLL; ++u) {
            a[u] = p[(ll + u + s2) * W];
            b[u] = p[(ll + u - s1 - 1) * W];
        }
#pragma unroll
        for (int u = 0; u < BOX_UNROLL; ++u) {
            t0 += ((double)a[u] - (double)b[u]);
            q0[(ll + u) * W] = (float)(t0 / dwin);
            if (VAR) {
                t1 += ((double)(a[u] * a[u]) - (double)(b[u] * b[u]));
                q1[(ll + u) * W] = (float)(t1 / dwin);
            }
        }
    }
    for (; ll < i1; ++ll) {
        const float a = p[(ll + s2) * W], b = p[(ll - s1 - 1) * W];
        t0 += ((double)a - (double)b);
        q0[ll * W] = (float)(t0 / dwin);
        if (VAR) {
            t1 += ((double)(a * a) - (double)(b * b));
            q1[ll * W] = (float)(t1 / dwin);
        }
    }
    reflected(n);
}

// ------------------------------------------------------------------------------------------------------ box filter, axis 1
// One workgroup of four waves: rows row0 .. row0 + 63 of in0 (and in1 when VAR), the planes axis 0 wrote.  Per chunk of CH columns:
//   1. all four waves load the chunk's leading samples x(ll + s2) and trailing samples x(ll - s1 - 1), coalesced, into the cells;
//   2. the first wave walks: lane r owns row r, carries its running sum(s) in registers from chunk to chunk, and replaces each cell it
//      has consumed by the sum -- the only serial part, two conversions, a subtraction and an addition per sample;
//   3. all four waves divide (the IEEE double division is most of the arithmetic, and it is independent per sample), round to float32
//      and store coalesced.  VAR writes mean2 - (float)(mean * mean) instead of the mean.
// A chunk whose samples all exist as they are (no reflection, a whole band) takes unconditional, unrolled loads and stores.  Rows of
// cells are padded by one cell: the walking lanes read down a column of the tile.
template <bool VAR, int CH>
__global__ __launch_bounds__(256) void box_rows_kernel(const float *__restrict__ in0, const float *__restrict__ in1, int H, int W, int win,
                                                       float *__restrict__ out) {
    constexpr int NP = VAR ? 2 : 1;
    constexpr int PER_THREAD = BOX_ROWS * CH / 256;
    __shared__ unsigned long long s_c[NP][BOX_ROWS][CH + 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const long long row0 = (long long)blockIdx.x * BOX_ROWS, row = row0 + lane;
    const bool walker = tid < 64 && row < H;
    const bool full_band = row0 + BOX_ROWS <= H;
    const long long s1 = win / 2, s2 = win - s1 - 1;
    const double dwin = (double)win;
    double t0 = 0.0, t1 = 0.0;
    if (walker) {
        const float *p0 = in0 + row * W, *p1 = VAR ? in1 + row * W : nullptr;
        for (long long l = -s1; l <= s2; ++l) {
            const int i = reflect_sym(l, W);
            t0 += (double)p0[i];
            if (VAR) t1 += (double)p1[i];
        }
    }
    for (long long c0 = 0; c0 < W; c0 += CH) {
        const int nc = (int)(W - c0 < CH ? W - c0 : CH);
        const bool whole = full_band && nc == CH;
        if (whole && c0 - s1 - 1 >= 0 && c0 + nc - 1 + s2 < W) {
            // every sample of the tile exists as it is: unconditional loads, all issued before the first LDS store waits for one
#pragma unroll
            for (int k = 0; k < PER_THREAD; ++k) {
                const int i = tid + 256 * k, r = i / CH, j = i % CH;
                const long long at = (row0 + r) * W + c0 + j;
                s_c[0][r][j] = pack_pair(in0[at + s2], in0[at - s1 - 1]);
                if (VAR) s_c[1][r][j] = pack_pair(in1[at + s2], in1[at - s1 - 1]);
            }
        } else {
            for (int i = tid; i < BOX_ROWS * CH; i += 256) {
                const int r = i / CH, j = i % CH;
                if (row0 + r >= H || j >= nc) continue;
                const long long base = (row0 + r) * W;
                const int li = reflect_sym(c0 + j + s2, W), ti = reflect_sym(c0 + j - s1 - 1, W);
                s_c[0][r][j] = pack_pair(in0[base + li], in0[base + ti]);
                if (VAR) s_c[1][r][j] = pack_pair(in1[base + li], in1[base + ti]);
            }
        }
        __syncthreads();
        if (walker) {
#pragma unroll 8
            for (int j = 0; j < nc; ++j) {
                if (c0 + j > 0) {                       // column 0 is the first window itself
                    const unsigned long long c = s_c[0][lane][j];
                    t0 += ((double)pair_lead(c) - (double)pair_trail(c));
                    if (VAR) {
                        const unsigned long long d = s_c[1][lane][j];
                        t1 += ((double)pair_lead(d) - (double)pair_trail(d));
                    }
                }
                s_c[0][lane][j] = sum_cell(t0);
                if (VAR) s_c[1][lane][j] = sum_cell(t1);
            }
        }
        __syncthreads();
        if (whole) {
#pragma unroll
            for (int k = 0; k < PER_THREAD; ++k) {
                const int i = tid + 256 * k, r = i / CH, j = i % CH;
                const float mean = (float)(cell_sum(s_c[0][r][j]) / dwin);
                float res = mean;
                if (VAR) {
                    const float mean2 = (float)(cell_sum(s_c[1][r][j]) / dwin);
                    res = mean2 - mean * mean;
                }
                out[(row0 + r) * W + c0 + j] = res;
            }
        } else {
            for (int i = tid; i < BOX_ROWS * CH; i += 256) {
                const int r = i / CH, j = i % CH;
                if (row0 + r >= H || j >= nc) continue;
                const float mean = (float)(cell_sum(s_c[0][r][j]) / dwin);
                float res = mean;
                if (VAR) {
                    const float mean2 = (float)(cell_sum(s_c[1][r][j]) / dwin);
                    res = mean2 - mean * mean;
                }
                out[(row0 + r) * W + c0 + j] = res;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- stretch
__global__ __launch_bounds__(256) void stretch_f32_kernel(const float *__restrict__ x, long long n, double lo, double d, float *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        double v = ((double)x[i] - lo) / d;
        v = v < 0.0 ? 0.0 : v;                      // a NaN fails both comparisons and passes, as it passes np.clip
        v = v > 1.0 ? 1.0 : v;
        out[i] = (float)v;
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
int sharp_shape(const char *who, int H, int W) {
    if (H <= 0 || W <= 0) { set_error("%s: H and W must be positive, got %d x %d", who, H, W); return OBIA_E_INVALID; }
    if ((long long)H * W >= 4294967295LL) {
        set_error("%s: %lld pixels; the percentile select takes fewer than 2^32 - 1", who, (long long)H * W);
        return OBIA_E_UNSUPPORTED;
    }
    return OBIA_OK;
}

int sharp_win(const char *who, int win) {
    if (win < 1) { set_error("%s: win must be at least 1, got %d", who, win); return OBIA_E_INVALID; }
    if (win > OBIA_SHARP_MAX_WIN) { set_error("%s: win %d is larger than %d", who, win, OBIA_SHARP_MAX_WIN); return OBIA_E_UNSUPPORTED; }
    return OBIA_OK;
}

int clear_counter(obia_ctx *ctx, const char *who, int64_t *counter) {
    if (!counter) return OBIA_OK;
    if (Buffers().lone<8>(counter).bad()) { set_error("%s: nonfinite_out must be 8-byte aligned", who); return OBIA_E_INVALID; }
    OBIA_HIP_TRY(hipMemsetAsync(counter, 0, sizeof(int64_t), ctx->stream));
    return OBIA_OK;
}

template <bool RASTER>
void launch_laplacian(obia_ctx *ctx, const float *src, int H, int W, int C, const int32_t *b, const float *stats, float *lap,
                      int64_t *bad) {
    const int ntx = cdiv(W, LAP_TX), nty = cdiv(H, LAP_TY);
    hipLaunchKernelGGL(laplacian_kernel<RASTER>, dim3((unsigned)((long long)ntx * nty)), dim3(256), 0, ctx->stream, src, H, W, C,
                       b ? b[0] : 0, b ? b[1] : 0, b ? b[2] : 0, stats, ntx, lap, reinterpret_cast<unsigned long long *>(bad));
}

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_sharp_gray_lap_dev(obia_ctx *ctx, const float *raster, int H, int W, int C, const int32_t *bands3, float *lap_out,
                            int64_t *nonfinite_out) {
    OBIA_TRY(enter(ctx));
    if (!bands3 || C < 1 || Buffers().lone(raster).lone(lap_out).bad()) {
        set_error("sharp gray_lap: bad arguments");
        return OBIA_E_INVALID;
    }
    OBIA_TRY(sharp_shape("sharp gray_lap", H, W));
    for (int b = 0; b < 3; ++b)
        if (bands3[b] < 0 || bands3[b] >= C) { set_error("sharp gray_lap: band %d of %d", bands3[b], C); return OBIA_E_INVALID; }
    OBIA_TRY(clear_counter(ctx, "sharp gray_lap", nonfinite_out));
    const long long npx = (long long)H * W;
    const int nparts = (int)grids::sharpness_minmax(npx).x.n;
    ctx->arena.reset();
    float *part = ctx->arena.get<float>(6 * (size_t)MM_GRID);
    float *stats = ctx->arena.get<float>(8);
    unsigned long long *scratch_bad = ctx->arena.get<unsigned long long>(1);
    if (!part || !stats || !scratch_bad) return OBIA_E_NOMEM;
    unsigned long long *bad = nonfinite_out ? reinterpret_cast<unsigned long long *>(nonfinite_out) : scratch_bad;
    if (!nonfinite_out) OBIA_HIP_TRY(hipMemsetAsync(scratch_bad, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(band_minmax_kernel, dim3(nparts), dim3(256), 0, ctx->stream, raster, npx, C, bands3[0], bands3[1], bands3[2], part,
                       bad);
    hipLaunchKernelGGL(band_stats_kernel, dim3(1), dim3(384), 0, ctx->stream, part, nparts, stats);
    launch_laplacian<true>(ctx, raster, H, W, C, bands3, stats, lap_out, nullptr);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_sharp_laplacian_dev(obia_ctx *ctx, const float *gray, int H, int W, float *lap_out, int64_t *nonfinite_out) {
    OBIA_TRY(enter(ctx));
    if (Buffers().out(lap_out).in(gray).bad()) {
        set_error("sharp laplacian: bad arguments");
        return OBIA_E_INVALID;
    }
    OBIA_TRY(sharp_shape("sharp laplacian", H, W));
    OBIA_TRY(clear_counter(ctx, "sharp laplacian", nonfinite_out));
    launch_laplacian<false>(ctx, gray, H, W, 1, nullptr, nullptr, lap_out, nonfinite_out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_sharp_box_dev(obia_ctx *ctx, const float *plane, int H, int W, int win, float *work, float *out, int64_t *nonfinite_out) {
    OBIA_TRY(enter(ctx));
    if (Buffers().out(work).out(out).in(plane).bad()) {
        set_error("sharp box: bad arguments");
        return OBIA_E_INVALID;
    }
    OBIA_TRY(sharp_shape("sharp box", H, W));
    OBIA_TRY(sharp_win("sharp box", win));
    OBIA_TRY(clear_counter(ctx, "sharp box", nonfinite_out));
    const long long n = (long long)H * W;
    if (nonfinite_out)
        hipLaunchKernelGGL(flat_pass_kernel, dim3(flat_grid(n)), dim3(256), 0, ctx->stream, plane, n, (float *)nullptr,
                           reinterpret_cast<unsigned long long *>(nonfinite_out));
    if (win == 1) {
        OBIA_HIP_TRY(hipMemcpyAsync(out, plane, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        hipLaunchKernelGGL(box_cols_kernel<false>, dim3(cdiv(W, 64)), dim3(64), 0, ctx->stream, plane, H, W, win, work, (float *)nullptr);
        hipLaunchKernelGGL((box_rows_kernel<false, BOX_CH1>), dim3(cdiv(H, BOX_ROWS)), dim3(256), 0, ctx->stream, (const float *)work,
                           (const float *)nullptr, H, W, win, out);
    }
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_sharp_variance_dev(obia_ctx *ctx, const float *lap, int H, int W, int win, float *work, float *out) {
    OBIA_TRY(enter(ctx));
    if (Buffers().out(work).out(out).in(lap).bad()) {
        set_error("sharp variance: bad arguments");
        return OBIA_E_INVALID;
    }
    OBIA_TRY(sharp_shape("sharp variance", H, W));
    OBIA_TRY(sharp_win("sharp variance", win));
    const long long n = (long long)H * W;
    if (win == 1) {
        hipLaunchKernelGGL(flat_pass_kernel, dim3(flat_grid(n)), dim3(256), 0, ctx->stream, lap, n, out, (unsigned long long *)nullptr);
    } else {
        float *m1 = work, *m2 = work + n;
        hipLaunchKernelGGL(box_cols_kernel<true>, dim3(cdiv(W, 64)), dim3(64), 0, ctx->stream, lap, H, W, win, m1, m2);
        hipLaunchKernelGGL((box_rows_kernel<true, BOX_CH2>), dim3(cdiv(H, BOX_ROWS)), dim3(256), 0, ctx->stream, (const float *)m1,
                           (const float *)m2, H, W, win, out);
    }
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_sharp_stretch_f32_dev(obia_ctx *ctx, const float *plane, int64_t n, double lo, double hi, float *out) {
    OBIA_TRY(enter(ctx));
    if (n <= 0 || Buffers().lone(plane).lone(out).bad()) {
        set_error("sharp stretch: bad arguments");
        return OBIA_E_INVALID;
    }
    hipLaunchKernelGGL(stretch_f32_kernel, dim3(flat_grid(n)), dim3(256), 0, ctx->stream, plane, (long long)n, lo, hi - lo, out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

}  // extern "C"
