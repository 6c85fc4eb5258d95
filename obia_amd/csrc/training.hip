// training.hip -- the training-tile passes (include/obia_training.h): Gaussian blur of a uint8 image in 8.8 fixed point, the 3 x 3
// chamfer distance transform as two parallel passes, darkening + hard / feathered blend, min-max scaling to uint8.  DESIGN.md 3.5o.
//
// uint8 images start at any byte and a row of 3 W bytes is rarely a multiple of four.  As in image.hip every kernel that writes bytes
// cuts its output into the ALIGNED dwords of the address space: a dword that lies inside the payload is stored whole, the ones at a
// head and a tail byte by byte.  The flat kernels (compose, min-max) cut the whole image that way, the blur every row for itself.
#include "common.hpp"
#include "../../include/obia_training.h"

#include <algorithm>
#include <climits>

namespace obia {
namespace {

// ------------------------------------------------------------------------------------------------------------------- blur
constexpr int BL_TY = 32;                              // output rows of one workgroup
constexpr int BL_CH = 64;                              // aligned dwords per output row of one workgroup
constexpr int BL_COLS = 4 * BL_CH + 3;                 // byte columns they can touch: a row's first dword starts 0 .. 3 bytes early
constexpr int BL_HALO = OBIA_TRAIN_MAX_KSIZE / 2;      // 15 pixels
constexpr int BL_SROWS = BL_TY + 2 * BL_HALO;          // staged rows, at the most
constexpr int BL_SCOLS = 352;                          // staged byte columns, at the most: 259 + 2 * 15 * 3 = 349
constexpr int BL_HCOLS = 260;                          // columns of the 16-bit plane (259, padded)
constexpr int BL_MAX_W = INT_MAX / 3 - 1024;           // 3 W + a tile's overhang fits int
static_assert(BL_COLS + 2 * BL_HALO * 3 <= BL_SCOLS && BL_COLS <= BL_HCOLS, "blur tile");

// BORDER_REFLECT_101 applied as often as it takes (period 2 (n - 1)); a line of one reads index 0
__device__ __forceinline__ int reflect101_any(int p, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    int m = p % period;
    if (m < 0) m += period;
    return m < n ? m : period - m;
}

// One workgroup: rows y0 .. y0 + 31, and of each row the 64 aligned dwords tx * 64 ... of ITS address range -- byte columns
// c_lo .. c_lo + 258 of the row whatever its alignment.  1. those bytes and a halo of ry rows and rx pixels (reflected) into LDS as
// bytes; 2. the horizontal pass over every staged row into a 16-bit plane (at most 255 * 256); 3. the vertical pass out of it,
// rounded, packed into dwords.
template <int NCH>
__global__ __launch_bounds__(256) void blur_kernel(const uint8_t *__restrict__ src, int H, int W, int kx, int ky,
                                                   const int32_t *__restrict__ wx, const int32_t *__restrict__ wy, int ntx,
                                                   uint8_t *__restrict__ out) {
    __shared__ uint8_t s_p[BL_SROWS][BL_SCOLS];
    __shared__ uint16_t s_h[BL_SROWS][BL_HCOLS];
    __shared__ int s_w[2][OBIA_TRAIN_MAX_KSIZE + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * BL_TY, c_lo = 4 * BL_CH * tx - 3;
    const int rx = kx / 2, ry = ky / 2;
    const int rowbytes = W * NCH;
    const int nrows = min(BL_TY, H - y0);
    const int nsr = nrows + 2 * ry, nsc = BL_COLS + 2 * rx * NCH;
    if (tid < kx) s_w[0][tid] = wx[tid];
    if (tid >= 64 && tid - 64 < ky) s_w[1][tid - 64] = wy[tid - 64];
    for (int r = wave; r < nsr; r += 4) {
        const long long row = (long long)reflect101_any(y0 - ry + r, H) * rowbytes;
        for (int b = lane; b < nsc; b += 64) {
            const int gb = c_lo - rx * NCH + b;                     // byte column of the row, negative in front of it
            const int x = gb >= 0 ? gb / NCH : -((-gb + NCH - 1) / NCH);
            const int c = gb - x * NCH;
            s_p[r][b] = src[row + (long long)reflect101_any(x, W) * NCH + c];
        }
    }
    __syncthreads();
    for (int r = wave; r < nsr; r += 4)
        for (int j = lane; j < BL_COLS; j += 64) {
            int acc = 0;
            for (int t = 0; t < kx; ++t) acc += s_w[0][t] * (int)s_p[r][j + t * NCH];
            s_h[r][j] = (uint16_t)acc;
        }
    __syncthreads();
    for (int i = tid; i < nrows * BL_CH; i += 256) {
        const int r = i >> 6, k = i & 63;
        uint8_t *rowp = out + (long long)(y0 + r) * rowbytes;
        const int a = (int)((uintptr_t)rowp & 3);
        const int kk = BL_CH * tx + k;
        if (kk >= (rowbytes + a + 3) >> 2) continue;
        const int j0 = 4 * kk - a;                                   // of the row; (rowp + j0) is an aligned dword
        const int jl = j0 - c_lo;                                    // 0 .. 255
        int acc[4] = {0, 0, 0, 0};
        for (int t = 0; t < ky; ++t) {
            const int w = s_w[1][t];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += w * (int)s_h[r + t][jl + q];
        }
        if (j0 >= 0 && j0 + 4 <= rowbytes) {
            uint32_t v = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) v |= (uint32_t)((acc[q] + 32768) >> 16) << (8 * q);
            *reinterpret_cast<uint32_t *>(rowp + j0) = v;
        } else {
            for (int q = 0; q < 4; ++q)
                if (j0 + q >= 0 && j0 + q < rowbytes) rowp[j0 + q] = (uint8_t)((acc[q] + 32768) >> 16);
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- distance
constexpr int DT_HV = 62587, DT_DG = 89738, DT_MAX = INT_MAX >> 2;
constexpr int DT_SEG = OBIA_TRAIN_MAX_SIDE / 256;      // pixels one lane walks, at the most

// Pass 1, one workgroup per row: work[y][x] = min(distance along the row to its nearest zero pixel, R + 1).  The row goes through LDS;
// every lane walks a segment of `seg` pixels, the position of the last zero before a segment and of the first behind it come from a
// scan over the segments' own last and first zeros.
__global__ __launch_bounds__(256) void dist_rows_kernel(const uint8_t *__restrict__ src, int W, int R, int32_t *__restrict__ work) {
    __shared__ uint8_t s_z[OBIA_TRAIN_MAX_SIDE];
    __shared__ int s_d[OBIA_TRAIN_MAX_SIDE];
    __shared__ int s_last[256], s_first[256];
    constexpr int FAR_L = -(1 << 20), FAR_R = 1 << 20;
    const int tid = threadIdx.x;
    const uint8_t *p = src + (long long)blockIdx.x * W;
    int32_t *q = work + (long long)blockIdx.x * W;
    for (int x = tid; x < W; x += 256) s_z[x] = p[x];
    __syncthreads();
    const int seg = (W + 255) / 256, x0 = tid * seg;
    int last = FAR_L, first = FAR_R;
    for (int i = 0; i < seg; ++i) {
        const int x = x0 + i;
        if (x < W && s_z[x] == 0) {
            last = x;
            first = first == FAR_R ? x : first;
        }
    }
    s_last[tid] = last;
    s_first[tid] = first;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int a = tid >= off ? s_last[tid - off] : FAR_L, b = tid + off < 256 ? s_first[tid + off] : FAR_R;
        __syncthreads();
        s_last[tid] = max(s_last[tid], a);
        s_first[tid] = min(s_first[tid], b);
        __syncthreads();
    }
    int cur = tid > 0 ? s_last[tid - 1] : FAR_L;
    for (int i = 0; i < seg; ++i) {
        const int x = x0 + i;
        if (x >= W) break;
        if (s_z[x] == 0) cur = x;
        s_d[x] = x - cur;
    }
    cur = tid < 255 ? s_first[tid + 1] : FAR_R;
    for (int i = seg - 1; i >= 0; --i) {
        const int x = x0 + i;
        if (x >= W) continue;
        if (s_z[x] == 0) cur = x;
        s_d[x] = min(min(s_d[x], cur - x), R + 1);
    }
    __syncthreads();
    for (int x = tid; x < W; x += 256) q[x] = s_d[x];
}

// Pass 2, one lane per pixel: the minimum over the rows |dy| <= R of HV * (max - min) + DG * min of (|dy|, that row's distance), rows
// whose nearest zero is farther than R columns ignored.  Walks outwards and stops where HV * |dy| alone is no better than what it has.
__global__ __launch_bounds__(256) void dist_min_kernel(const int32_t *__restrict__ work, int H, int W, int R, float *__restrict__ dist) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)H * W) return;
    const int y = (int)(i / W);
    int best = DT_MAX;
    for (int a = 0; a <= R; ++a) {
        const bool up = y - a >= 0, down = a > 0 && y + a < H;
        if ((!up && !down && a > 0) || DT_HV * a >= best) break;
        if (up) {
            const int d = work[i - (long long)a * W];
            if (d <= R) best = min(best, DT_HV * (max(a, d) - min(a, d)) + DT_DG * min(a, d));
        }
        if (down) {
            const int d = work[i + (long long)a * W];
            if (d <= R) best = min(best, DT_HV * (max(a, d) - min(a, d)) + DT_DG * min(a, d));
        }
    }
    dist[i] = (float)best * (1.0f / 65536.0f);
}

// ---------------------------------------------------------------------------------------------------------------- compose
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

template <bool FEATHER>
__global__ __launch_bounds__(256) void compose_kernel(const uint8_t *__restrict__ tile, const uint8_t *__restrict__ blurred,
                                                      const uint8_t *__restrict__ mask, const float *__restrict__ dist, long long npx,
                                                      const uint8_t *__restrict__ lut, float feather, uint8_t *__restrict__ out,
                                                      unsigned long long *__restrict__ bad) {
    __shared__ uint8_t s_t[256];
    s_t[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int a = (int)((uintptr_t)out & 3);
    const long long nb = 3 * npx, nchunks = (nb + a + 3) / 4;
    unsigned nbad = 0;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < nchunks; k += (long long)gridDim.x * 256) {
        const long long j0 = 4 * k - a;
        uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long j = j0 + q;
            if (j < 0 || j >= nb) continue;
            const long long px = j / 3;
            const uint32_t m = mask[px], t = tile[j], bg = s_t[blurred[j]];
            nbad += (j - 3 * px == 0 && m > 1u) ? 1u : 0u;           // once per pixel
            if (FEATHER) {
                float al = 1.0f - dist[px] / feather;
                al = al < 0.0f ? 0.0f : al;
                al = al > 1.0f ? 1.0f : al;
                float o = (al * (float)t) + ((1.0f - al) * (float)bg);
                o = o < 0.0f ? 0.0f : o;
                o = o > 255.0f ? 255.0f : o;
                v[q] = (uint32_t)(int)o;
            } else {
                v[q] = m ? t : bg;
            }
        }
        if (j0 >= 0 && j0 + 4 <= nb) {
            *reinterpret_cast<uint32_t *>(out + j0) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
            for (int q = 0; q < 4; ++q)
                if (j0 + q >= 0 && j0 + q < nb) out[j0 + q] = (uint8_t)v[q];
        }
    }
    nbad = wave_sum(nbad);
    if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, (unsigned long long)nbad);
}

// ---------------------------------------------------------------------------------------------------------------- min-max
constexpr int MM_PARTS = OBIA_TRAIN_MINMAX_WORK / 2;   // workgroups of the reduction, at the most

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// minimum and maximum of a workgroup's 256 pairs, in every thread
__device__ __forceinline__ void group_minmax(float &mn, float &mx, float (*s_v)[2]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float a = __shfl_xor(mn, off), c = __shfl_xor(mx, off);
        mn = a < mn ? a : mn;
        mx = c > mx ? c : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        s_v[threadIdx.x >> 6][0] = mn;
        s_v[threadIdx.x >> 6][1] = mx;
    }
    __syncthreads();
    mn = s_v[0][0];
    mx = s_v[0][1];
    for (int w = 1; w < 4; ++w) {
        mn = s_v[w][0] < mn ? s_v[w][0] : mn;
        mx = s_v[w][1] > mx ? s_v[w][1] : mx;
    }
}

// part[g] = minimum, part[MM_PARTS + g] = maximum of workgroup g's share
__global__ __launch_bounds__(256) void minmax_reduce_kernel(const float *__restrict__ x, long long n, float *__restrict__ part,
                                                            unsigned long long *__restrict__ bad) {
    __shared__ float s_v[4][2];
    float mn = INFINITY, mx = -INFINITY;
    unsigned nbad = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = x[i];
        nbad += finite_f(v) ? 0u : 1u;
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    nbad = wave_sum(nbad);
    if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, (unsigned long long)nbad);
    group_minmax(mn, mx, s_v);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = mn;
        part[MM_PARTS + blockIdx.x] = mx;
    }
}

__global__ __launch_bounds__(256) void minmax_scale_kernel(const float *__restrict__ x, long long n, const float *__restrict__ part,
                                                           int nparts, uint8_t *__restrict__ out) {
    __shared__ float s_v[4][2];
    float mn = INFINITY, mx = -INFINITY;
    if ((int)threadIdx.x < nparts) {
        mn = part[threadIdx.x];
        mx = part[MM_PARTS + threadIdx.x];
    }
    group_minmax(mn, mx, s_v);
    const bool flat = mn == mx;
    const float d = mx - mn;
    auto scale = [&](float v) -> uint32_t {
        if (flat) return 0u;
        float s = (255.0f * (v - mn)) / d;
        s = s > 0.0f ? s : 0.0f;
        s = s < 255.0f ? s : 255.0f;
        return (uint32_t)(int)s;
    };
    const int a = (int)((uintptr_t)out & 3);
    const long long nchunks = (n + a + 3) / 4;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < nchunks; k += (long long)gridDim.x * 256) {
        const long long j0 = 4 * k - a;
        if (j0 >= 0 && j0 + 4 <= n) {
            uint32_t w = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) w |= scale(x[j0 + i]) << (8 * i);
            *reinterpret_cast<uint32_t *>(out + j0) = w;
        } else {
            for (int i = 0; i < 4; ++i)
                if (j0 + i >= 0 && j0 + i < n) out[j0 + i] = (uint8_t)scale(x[j0 + i]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
int clear_counter(obia_ctx *ctx, const char *who, int64_t *counter) {
    if (Buffers().lone<8>(counter).bad()) { set_error("%s: the counter must be an 8-byte aligned device pointer", who); return OBIA_E_INVALID; }
    OBIA_HIP_TRY(hipMemsetAsync(counter, 0, sizeof(int64_t), ctx->stream));
    return OBIA_OK;
}

bool odd_ksize(int k) { return k >= 1 && k <= OBIA_TRAIN_MAX_KSIZE && (k & 1); }

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_train_blur_u8_dev(obia_ctx *ctx, const uint8_t *src, int H, int W, int nch, int kx, int ky, const int32_t *wx, const int32_t *wy,
                           uint8_t *out) {
    OBIA_TRY(enter(ctx));
    if (Buffers().out(out).in(src).lone(wx).lone(wy).bad()) {
        set_error("train blur: bad arguments");
        return OBIA_E_INVALID;
    }
    if (H <= 0 || W <= 0) { set_error("train blur: H and W must be positive, got %d x %d", H, W); return OBIA_E_INVALID; }
    if (nch != 1 && nch != 3) { set_error("train blur: 1 or 3 channels, got %d", nch); return OBIA_E_INVALID; }
    if (!odd_ksize(kx) || !odd_ksize(ky)) {
        set_error("train blur: kx and ky must be odd and in 1..%d, got (%d, %d)", OBIA_TRAIN_MAX_KSIZE, kx, ky);
        return OBIA_E_INVALID;
    }
    if (W > BL_MAX_W) { set_error("train blur: W %d is larger than %d", W, BL_MAX_W); return OBIA_E_UNSUPPORTED; }
    const int ntx = cdiv(((long long)W * nch + 6) >> 2, BL_CH);
    const long long ngroups = (long long)ntx * cdiv(H, BL_TY);
    if (ngroups > INT_MAX) { set_error("train blur: %d x %d is too large", H, W); return OBIA_E_UNSUPPORTED; }
    if (nch == 3)
        hipLaunchKernelGGL(blur_kernel<3>, dim3((unsigned)ngroups), dim3(256), 0, ctx->stream, src, H, W, kx, ky, wx, wy, ntx, out);
    else
        hipLaunchKernelGGL(blur_kernel<1>, dim3((unsigned)ngroups), dim3(256), 0, ctx->stream, src, H, W, kx, ky, wx, wy, ntx, out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_train_distance_dev(obia_ctx *ctx, const uint8_t *src, int H, int W, int R, int32_t *work, float *dist_out) {
    OBIA_TRY(enter(ctx));
    if (Buffers().out(work).out(dist_out).lone(src).bad()) {
        set_error("train distance: bad arguments");
        return OBIA_E_INVALID;
    }
    if (H <= 0 || W <= 0) { set_error("train distance: H and W must be positive, got %d x %d", H, W); return OBIA_E_INVALID; }
    if (R < 0) { set_error("train distance: R must not be negative, got %d", R); return OBIA_E_INVALID; }
    if (H > OBIA_TRAIN_MAX_SIDE || W > OBIA_TRAIN_MAX_SIDE) {
        set_error("train distance: %d x %d; a side may be %d at the most", H, W, OBIA_TRAIN_MAX_SIDE);
        return OBIA_E_UNSUPPORTED;
    }
    static_assert(DT_SEG * 256 == OBIA_TRAIN_MAX_SIDE, "one lane walks at most DT_SEG pixels of a row");
    static_assert((long long)DT_DG * OBIA_TRAIN_MAX_SIDE < DT_MAX, "no finite distance reaches DIST_MAX");
    R = std::min(R, OBIA_TRAIN_MAX_SIDE);                            // nothing is farther
    hipLaunchKernelGGL(dist_rows_kernel, dim3(H), dim3(256), 0, ctx->stream, src, W, R, work);
    hipLaunchKernelGGL(dist_min_kernel, dim3(cdiv((long long)H * W, 256)), dim3(256), 0, ctx->stream, (const int32_t *)work, H, W, R,
                       dist_out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_train_compose_u8_dev(obia_ctx *ctx, const uint8_t *tile, const uint8_t *blurred, const uint8_t *mask, const float *dist, int H,
                              int W, const uint8_t *darken_lut, double feather, uint8_t *out, int64_t *bad_mask_out) {
    OBIA_TRY(enter(ctx));
    if (Buffers().out(out).in(tile).in(blurred).lone(mask).lone(darken_lut).lone(dist, OPTIONAL).bad()) {
        set_error("train compose: bad arguments");
        return OBIA_E_INVALID;
    }
    if (H <= 0 || W <= 0) { set_error("train compose: H and W must be positive, got %d x %d", H, W); return OBIA_E_INVALID; }
    if (dist && !((float)feather > 0.0f)) { set_error("train compose: a feathered blend needs feather > 0, got %g", feather); return OBIA_E_INVALID; }
    OBIA_TRY(clear_counter(ctx, "train compose", bad_mask_out));
    const long long npx = (long long)H * W;
    unsigned long long *bad = reinterpret_cast<unsigned long long *>(bad_mask_out);
    const unsigned grid = (unsigned)grids::training_compose(npx).x.n;
    if (dist)
        hipLaunchKernelGGL(compose_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, tile, blurred, mask, dist, npx, darken_lut,
                           (float)feather, out, bad);
    else
        hipLaunchKernelGGL(compose_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, tile, blurred, mask, dist, npx, darken_lut, 0.0f,
                           out, bad);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_train_minmax_u8_dev(obia_ctx *ctx, const float *x, int64_t n, float *work, uint8_t *out, int64_t *nonfinite_out) {
    OBIA_TRY(enter(ctx));
    if (n <= 0 || Buffers().out(work).in(x).lone(out).bad()) {
        set_error("train minmax: bad arguments");
        return OBIA_E_INVALID;
    }
    OBIA_TRY(clear_counter(ctx, "train minmax", nonfinite_out));
    const int nparts = (int)grids::training_minmax_reduce(n).x.n;
    hipLaunchKernelGGL(minmax_reduce_kernel, dim3(nparts), dim3(256), 0, ctx->stream, x, (long long)n, work,
                       reinterpret_cast<unsigned long long *>(nonfinite_out));
    hipLaunchKernelGGL(minmax_scale_kernel, to_dim3(grids::training_minmax_scale(n)), dim3(256), 0, ctx->stream, x, (long long)n, (const float *)work,
                       nparts, out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

}  // extern "C"
