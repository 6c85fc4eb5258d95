// image.hip -- the image-preview passes (include/obia_image.h): percentile stretch to uint8, grey plane + 256-bin histogram, table
// look-up, CLAHE, find_boundaries(mode="outer") and the boundary overlay.  DESIGN.md 3.5m.
//
// uint8 rasters may start at any byte and a row of 3 W bytes is rarely a multiple of four, so every kernel that writes bytes cuts its
// output into the ALIGNED dwords of the address space ("chunks"): a chunk that lies inside the payload is stored as whole dwords, the
// chunk at the head and the one at the tail byte by byte.  Reads go the other way round: load_dwords() fetches the aligned dwords that
// cover a run of bytes and shifts them into place (v_alignbyte_b32); every dword it touches holds at least one byte of the run, so it
// never reads a dword the caller does not own a byte of.
#include "common.hpp"
#include "../../include/obia_image.h"

#include <algorithm>
#include <climits>

namespace obia {
namespace {

// ---------------------------------------------------------------------------------------------------------------- helpers
// bytes p[0 .. 4 N) as N dwords; all of them must be readable
template <int N> __device__ __forceinline__ void load_dwords(const uint8_t *p, uint32_t (&s)[N]) {
    const uint32_t b = (uint32_t)((uintptr_t)p & 3);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - b);
    uint32_t d[N + 1];
#pragma unroll
    for (int i = 0; i < N; ++i) d[i] = q[i];
    if (b == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) s[i] = d[i];
    } else {
        d[N] = q[N];                                  // holds p[4 N - b ...]: bytes of the run
#pragma unroll
        for (int i = 0; i < N; ++i) s[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], b);
    }
}

// One count into a workgroup's LDS histogram.  Called by every lane of a wave together.  A wave whose active lanes all hold the same
// value (a flat image: the contention case) adds their number once instead of serialising 64 atomics on one word.
__device__ __forceinline__ void hist_add(unsigned *s_h, int v, bool active) {
    const unsigned long long m = __ballot(active);
    if (m == 0) return;
    const int lead = __ffsll((long long)m) - 1;
    const int first = __shfl(v, lead);
    if (__ballot(active && v != first) == 0) {
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(&s_h[first], (unsigned)__popcll(m));
    } else if (active) {
        atomicAdd(&s_h[v], 1u);
    }
}

__device__ __forceinline__ uint32_t sat_u8(int v) { return (uint32_t)min(max(v, 0), 255); }

// ---------------------------------------------------------------------------------------------------------------- stretch
__device__ __forceinline__ uint32_t stretch_u8(double x, double lo, double d) {
    double v = (255.0 * (x - lo)) / d;
    v = v > 0.0 ? v : 0.0;
    v = v < 255.0 ? v : 255.0;
    return (uint32_t)(int)v;
}

template <typename F>
__global__ __launch_bounds__(256) void stretch_kernel(const F *__restrict__ x, long long n, double lo, double d, uint8_t *__restrict__ out) {
    const int a = (int)((uintptr_t)out & 3);
    const long long nchunks = (n + a + 3) / 4;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < nchunks; k += (long long)gridDim.x * 256) {
        const long long j0 = 4 * k - a;
        if (j0 >= 0 && j0 + 4 <= n) {
            uint32_t w = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) w |= stretch_u8((double)x[j0 + i], lo, d) << (8 * i);
            *reinterpret_cast<uint32_t *>(out + j0) = w;
        } else {
            for (int i = 0; i < 4; ++i)
                if (j0 + i >= 0 && j0 + i < n) out[j0 + i] = (uint8_t)stretch_u8((double)x[j0 + i], lo, d);
        }
    }
}

// ------------------------------------------------------------------------------------------------- grey plane + histogram
__device__ __forceinline__ uint32_t gray_of(uint32_t rgb) {    // bytes R, G, B from the low end
    return (9798u * (rgb & 255u) + 19235u * ((rgb >> 8) & 255u) + 3735u * ((rgb >> 16) & 255u) + 16384u) >> 15;
}

// chunk k: pixels 4 k - a .. 4 k - a + 3, a = misalignment of gray_out (0 without one)
__global__ __launch_bounds__(256) void gray_hist_kernel(const uint8_t *__restrict__ px, int nch, long long n, uint8_t *__restrict__ gray,
                                                        unsigned long long *__restrict__ hist) {
    __shared__ unsigned s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const int a = gray ? (int)((uintptr_t)gray & 3) : 0;
    const long long nchunks = (n + a + 3) / 4;
    for (long long kb = (long long)blockIdx.x * 256; kb < nchunks; kb += (long long)gridDim.x * 256) {
        const long long k = kb + threadIdx.x;
        const long long j0 = 4 * k - a;
        const bool full = k < nchunks && j0 >= 0 && j0 + 4 <= n;
        uint32_t g[4] = {0, 0, 0, 0};
        bool on[4] = {false, false, false, false};
        if (full) {
            if (nch == 3) {
                uint32_t s[3];
                load_dwords<3>(px + 3 * j0, s);
                g[0] = gray_of(s[0]);
                g[1] = gray_of((s[0] >> 24) | (s[1] << 8));
                g[2] = gray_of((s[1] >> 16) | (s[2] << 16));
                g[3] = gray_of(s[2] >> 8);
            } else {
                uint32_t s[1];
                load_dwords<1>(px + j0, s);
#pragma unroll
                for (int i = 0; i < 4; ++i) g[i] = (s[0] >> (8 * i)) & 255u;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) on[i] = true;
            if (gray) *reinterpret_cast<uint32_t *>(gray + j0) = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
        } else if (k < nchunks) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long j = j0 + i;
                if (j < 0 || j >= n) continue;
                on[i] = true;
                g[i] = nch == 3 ? gray_of((uint32_t)px[3 * j] | ((uint32_t)px[3 * j + 1] << 8) | ((uint32_t)px[3 * j + 2] << 16)) : px[j];
                if (gray) gray[j] = (uint8_t)g[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) hist_add(s_h, (int)g[i], on[i]);
    }
    __syncthreads();
    if (s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)s_h[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------------------- look-up
template <int REP>
__global__ __launch_bounds__(256) void lut_kernel(const uint8_t *__restrict__ in, long long n, const uint8_t *__restrict__ lut,
                                                  uint8_t *__restrict__ out) {
    __shared__ uint8_t s_t[256];
    s_t[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int a = (int)((uintptr_t)out & 3);
    const long long nb = n * REP;
    const long long nchunks = (nb + a + 3) / 4;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < nchunks; k += (long long)gridDim.x * 256) {
        const long long j0 = 4 * k - a;
        if (j0 >= 0 && j0 + 4 <= nb) {
            uint32_t w = 0;
            if (REP == 1) {
                uint32_t s[1];
                load_dwords<1>(in + j0, s);
#pragma unroll
                for (int i = 0; i < 4; ++i) w |= (uint32_t)s_t[(s[0] >> (8 * i)) & 255u] << (8 * i);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) w |= (uint32_t)s_t[in[(j0 + i) / REP]] << (8 * i);
            }
            *reinterpret_cast<uint32_t *>(out + j0) = w;
        } else {
            for (int i = 0; i < 4; ++i)
                if (j0 + i >= 0 && j0 + i < nb) out[j0 + i] = s_t[in[(j0 + i) / REP]];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ CLAHE
// OpenCV's borderInterpolate(p, len, BORDER_REFLECT_101) for p >= 0
__device__ __forceinline__ int reflect101(int p, int len) {
    if (p < len) return p;
    if (len == 1) return 0;
    do {
        p = p < 0 ? -p : 2 * (len - 1) - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

// histograms of the 64 tiles of the padded image; blockIdx.x = tile, blockIdx.y = slab of `rows` tile rows
__global__ __launch_bounds__(256) void clahe_hist_kernel(const uint8_t *__restrict__ in, int H, int W, int nch, int ch, int th, int tw,
                                                         int rows, unsigned *__restrict__ hist) {
    __shared__ unsigned s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const int tile = blockIdx.x, ty = tile >> 3, tx = tile & 7;
    const int r1 = min(th, ((int)blockIdx.y + 1) * rows);
    for (int r = blockIdx.y * rows; r < r1; ++r) {
        const int sy = reflect101(ty * th + r, H);
        const uint8_t *row = in + (long long)sy * W * nch + ch;
        for (int xb = 0; xb < tw; xb += 256) {
            const int x = xb + threadIdx.x;
            const bool active = x < tw;
            int v = 0;
            if (active) v = row[(long long)reflect101(tx * tw + x, W) * nch];
            hist_add(s_h, v, active);
        }
    }
    __syncthreads();
    if (s_h[threadIdx.x]) atomicAdd(&hist[tile * 256 + threadIdx.x], s_h[threadIdx.x]);
}

// clip, redistribute, running sum, table: one workgroup per tile, one lane per bin (OpenCV's CLAHE_CalcLut_Body)
__global__ __launch_bounds__(256) void clahe_lut_kernel(const unsigned *__restrict__ hist, int clip, float lut_scale,
                                                        uint8_t *__restrict__ lut) {
    __shared__ int s_a[256];
    const int tid = threadIdx.x, tile = blockIdx.x;
    int h = (int)hist[tile * 256 + tid];
    s_a[tid] = max(h - clip, 0);
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) s_a[tid] += s_a[tid + off];
        __syncthreads();
    }
    const int excess = s_a[0];
    __syncthreads();
    const int batch = excess / 256;
    const int residual = excess - batch * 256;
    h = min(h, clip) + batch;
    if (residual) {
        const int step = max(256 / residual, 1);
        if (tid % step == 0 && tid / step < residual) ++h;
    }
    s_a[tid] = h;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {           // inclusive integer scan
        const int add = tid >= off ? s_a[tid - off] : 0;
        __syncthreads();
        s_a[tid] += add;
        __syncthreads();
    }
    lut[tile * 256 + tid] = (uint8_t)sat_u8(__float2int_rn((float)s_a[tid] * lut_scale));
}

constexpr int CL_ROWS = grids::CLAHE_ROWS;     // rows of one interpolation workgroup (256 columns wide)

__global__ __launch_bounds__(256) void clahe_interp_kernel(const uint8_t *__restrict__ in, int H, int W, int nch, int ch, int th, int tw,
                                                           const uint8_t *__restrict__ lut, uint8_t *__restrict__ out) {
    __shared__ uint32_t s_lut[64 * 256 / 4];
    const uint32_t *lut4 = reinterpret_cast<const uint32_t *>(lut);      // arena memory: aligned
    for (int i = threadIdx.x; i < 64 * 256 / 4; i += 256) s_lut[i] = lut4[i];
    __syncthreads();
    const uint8_t *s_t = reinterpret_cast<const uint8_t *>(s_lut);
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const float inv_tw = 1.0f / (float)tw, inv_th = 1.0f / (float)th;
    const float txf = (float)x * inv_tw - 0.5f;
    int tx1 = (int)floorf(txf);
    int tx2 = tx1 + 1;
    const float xa = txf - (float)tx1, xa1 = 1.0f - xa;
    tx1 = max(tx1, 0);
    tx2 = min(tx2, 7);
    // row blocks of CL_ROWS rows, strided over grid.y (grids::image_clahe_interp); 64-bit: H + CL_ROWS may pass 2^31
    for (long long yb = (long long)blockIdx.y * CL_ROWS; yb < H; yb += (long long)gridDim.y * CL_ROWS) {
        const int y1 = (int)min((long long)H, yb + CL_ROWS);
        for (int y = (int)yb; y < y1; ++y) {
            const float tyf = (float)y * inv_th - 0.5f;
            int ty1 = (int)floorf(tyf);
            int ty2 = ty1 + 1;
            const float ya = tyf - (float)ty1, ya1 = 1.0f - ya;
            ty1 = max(ty1, 0);
            ty2 = min(ty2, 7);
            const long long at = ((long long)y * W + x) * nch + ch;
            const int v = in[at];
            const float l11 = (float)s_t[(ty1 * 8 + tx1) * 256 + v], l12 = (float)s_t[(ty1 * 8 + tx2) * 256 + v];
            const float l21 = (float)s_t[(ty2 * 8 + tx1) * 256 + v], l22 = (float)s_t[(ty2 * 8 + tx2) * 256 + v];
            const float res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya;
            out[at] = (uint8_t)sat_u8(__float2int_rn(res));
        }
    }
}

// -------------------------------------------------------------------------------------------------------------- boundaries
// find_boundaries(mode="outer", background=0) of the pixel in the middle of a 3 x 3 window; neighbours outside the raster are given
// as copies of a pixel inside the window (clamped coordinates), which changes neither the maximum nor the minimum
__device__ __forceinline__ bool outer_boundary(const int32_t (&r0)[3], const int32_t (&r1)[3], const int32_t (&r2)[3]) {
    const int32_t c = r1[1];
    const bool b = r0[1] != c || r2[1] != c || r1[0] != c || r1[2] != c;
    if (!b) return false;
    if (c == 0) return true;
    int32_t mx = c, mn = c;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        mx = max(mx, max(r0[i], max(r1[i], r2[i])));
        mn = min(mn, min(r0[i] == 0 ? INT_MAX : r0[i], min(r1[i] == 0 ? INT_MAX : r1[i], r2[i] == 0 ? INT_MAX : r2[i])));
    }
    return mx != mn;
}

// boundary flags of NPX consecutive pixels q0 .. q0 + NPX - 1 of row y (pixels outside the row give a flag nobody reads)
template <int NPX>
__device__ __forceinline__ void boundary_flags(const int32_t *__restrict__ lab, int H, int W, int y, int q0, bool (&flag)[NPX]) {
    const int32_t *up = lab + (long long)max(y - 1, 0) * W, *mid = lab + (long long)y * W, *dn = lab + (long long)min(y + 1, H - 1) * W;
    int32_t a[NPX + 2], b[NPX + 2], c[NPX + 2];
#pragma unroll
    for (int i = 0; i < NPX + 2; ++i) {
        const int x = min(max(q0 - 1 + i, 0), W - 1);
        a[i] = up[x];
        b[i] = mid[x];
        c[i] = dn[x];
    }
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
        const int32_t r0[3] = {a[i], a[i + 1], a[i + 2]}, r1[3] = {b[i], b[i + 1], b[i + 2]}, r2[3] = {c[i], c[i + 1], c[i + 2]};
        flag[i] = outer_boundary(r0, r1, r2);
    }
}

__global__ __launch_bounds__(256) void boundaries_kernel(const int32_t *__restrict__ lab, int H, int W, uint8_t *__restrict__ out) {
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        uint8_t *orow = out + (long long)y * W;
        const int a = (int)((uintptr_t)orow & 3);
        const int nchunks = (int)(((long long)W + a + 3) / 4);
        for (int k = blockIdx.x * 256 + threadIdx.x; k < nchunks; k += gridDim.x * 256) {
            const int x0 = 4 * k - a;
            bool f[4];
            boundary_flags<4>(lab, H, W, y, x0, f);
            if (x0 >= 0 && x0 + 4 <= W) {
                *reinterpret_cast<uint32_t *>(orow + x0) = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (x0 + i >= 0 && x0 + i < W) orow[x0 + i] = (uint8_t)f[i];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- mark
// Chunk k of a row: the 12 aligned bytes that start 12 k - a bytes into the row's 3 W (a: misalignment of the row's first byte).
// They belong to at most five pixels q0 .. q0 + 4; the five results are packed into a 15-byte stream and shifted by the r0 = 0..2
// bytes of pixel q0 that lie in front of the chunk.
__global__ __launch_bounds__(256) void mark_kernel(const uint8_t *__restrict__ img, int nch, const int32_t *__restrict__ lab, int H, int W,
                                                   const uint8_t *__restrict__ table, uint32_t color, uint8_t *__restrict__ out) {
    __shared__ uint8_t s_t[256];
    s_t[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const int nbytes = 3 * W;
    const long long total = (long long)H * W * 3;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        uint8_t *orow = out + (long long)y * nbytes;
        const int a = (int)((uintptr_t)orow & 3);
        const int nchunks = (nbytes + a + 11) / 12;
        for (int k = blockIdx.x * 256 + threadIdx.x; k < nchunks; k += gridDim.x * 256) {
            const int j0 = 12 * k - a;                  // >= -3
            const int q0 = (j0 + 3) / 3 - 1;            // floor(j0 / 3)
            const uint32_t r0 = (uint32_t)(j0 - 3 * q0);
            bool f[5];
            boundary_flags<5>(lab, H, W, y, q0, f);
            uint32_t p[5] = {0, 0, 0, 0, 0};            // the image's three bytes of each pixel
            const long long pix0 = (long long)y * W + q0;
            if (nch == 3 && q0 >= 0 && pix0 * 3 + 16 <= total) {
                uint32_t s[4];
                load_dwords<4>(img + pix0 * 3, s);
                p[0] = s[0] & 0xFFFFFFu;
                p[1] = ((s[0] >> 24) | (s[1] << 8)) & 0xFFFFFFu;
                p[2] = ((s[1] >> 16) | (s[2] << 16)) & 0xFFFFFFu;
                p[3] = s[2] >> 8;
                p[4] = s[3] & 0xFFFFFFu;
            } else {
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    if (q0 + i < 0 || q0 + i >= W) continue;
                    if (nch == 3) {
                        const uint8_t *s = img + (pix0 + i) * 3;
                        p[i] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
                    } else {
                        p[i] = 0x010101u * (uint32_t)img[pix0 + i];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 5; ++i)
                p[i] = f[i] ? color
                            : (uint32_t)s_t[p[i] & 255u] | ((uint32_t)s_t[(p[i] >> 8) & 255u] << 8) | ((uint32_t)s_t[(p[i] >> 16) & 255u] << 16);
            const uint32_t s0 = p[0] | (p[1] << 24), s1 = (p[1] >> 8) | (p[2] << 16), s2 = (p[2] >> 16) | (p[3] << 8), s3 = p[4];
            const uint32_t o0 = __builtin_amdgcn_alignbyte(s1, s0, r0), o1 = __builtin_amdgcn_alignbyte(s2, s1, r0),
                           o2 = __builtin_amdgcn_alignbyte(s3, s2, r0);
            if (j0 >= 0 && j0 + 12 <= nbytes) {
                uint32_t *o = reinterpret_cast<uint32_t *>(orow + j0);
                o[0] = o0;
                o[1] = o1;
                o[2] = o2;
            } else {
                const uint32_t o[3] = {o0, o1, o2};
#pragma unroll
                for (int i = 0; i < 12; ++i)
                    if (j0 + i >= 0 && j0 + i < nbytes) orow[j0 + i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
            }
        }
    }
}

constexpr long long MAX_W = INT_MAX / 3 - 8;      // 3 W + 14 fits int

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_image_stretch_u8_dev(obia_ctx *ctx, const void *plane, int is_f64, int64_t n, double lo, double hi, uint8_t *out) {
    OBIA_TRY(enter(ctx));
    if (!plane || !out || n <= 0 || ((uintptr_t)plane & (is_f64 ? 7 : 3))) {
        set_error("image stretch: bad arguments");
        return OBIA_E_INVALID;
    }
    if (lo == hi) {
        OBIA_HIP_TRY(hipMemsetAsync(out, 0, (size_t)n, ctx->stream));
        return OBIA_OK;
    }
    const dim3 grid = to_dim3(grids::image_stretch(n));
    const double d = hi - lo;
    if (is_f64)
        hipLaunchKernelGGL(stretch_kernel<double>, grid, dim3(256), 0, ctx->stream, (const double *)plane, (long long)n, lo, d, out);
    else
        hipLaunchKernelGGL(stretch_kernel<float>, grid, dim3(256), 0, ctx->stream, (const float *)plane, (long long)n, lo, d, out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_image_gray_hist_dev(obia_ctx *ctx, const uint8_t *pixels, int nch, int64_t n, uint8_t *gray_out, int64_t *hist256_out) {
    OBIA_TRY(enter(ctx));
    if (!pixels || !hist256_out || (nch != 1 && nch != 3) || n <= 0 || n > (int64_t)INT_MAX || ((uintptr_t)hist256_out & 7)) {
        set_error("image gray_hist: bad arguments (nch 1 or 3, 1 <= n < 2^31)");
        return OBIA_E_INVALID;
    }
    OBIA_HIP_TRY(hipMemsetAsync(hist256_out, 0, 256 * sizeof(int64_t), ctx->stream));
    hipLaunchKernelGGL(gray_hist_kernel, to_dim3(grids::image_gray_hist(n)), dim3(256), 0, ctx->stream, pixels, nch, (long long)n,
                       gray_out, reinterpret_cast<unsigned long long *>(hist256_out));
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_image_lut_u8_dev(obia_ctx *ctx, const uint8_t *in, int64_t n, const uint8_t *lut256, int rep, uint8_t *out) {
    OBIA_TRY(enter(ctx));
    if (!in || !lut256 || !out || n <= 0 || (rep != 1 && rep != 3)) {
        set_error("image lut: bad arguments (rep 1 or 3)");
        return OBIA_E_INVALID;
    }
    const dim3 grid = to_dim3(grids::image_lut(n, rep));
    if (rep == 1)
        hipLaunchKernelGGL(lut_kernel<1>, grid, dim3(256), 0, ctx->stream, in, (long long)n, lut256, out);
    else
        hipLaunchKernelGGL(lut_kernel<3>, grid, dim3(256), 0, ctx->stream, in, (long long)n, lut256, out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_image_clahe_u8_dev(obia_ctx *ctx, const uint8_t *in, int H, int W, int nch, int ch, uint8_t *out) {
    OBIA_TRY(enter(ctx));
    if (!in || !out || in == out || H < 8 || W < 8 || nch < 1 || nch > 4 || ch < 0 || ch >= nch || W > INT_MAX - 8 || H > INT_MAX - 8) {
        set_error("image clahe: bad arguments (H, W >= 8, 0 <= ch < nch <= 4, out is not in)");
        return OBIA_E_INVALID;
    }
    // cv::CLAHE::apply: no padding when both sides divide by 8, else 8 - side % 8 on BOTH (a full 8 on a side that divides)
    const bool pad = (W % 8) || (H % 8);
    const int th = (pad ? H + 8 - H % 8 : H) / 8, tw = (pad ? W + 8 - W % 8 : W) / 8;
    const long long area = (long long)th * tw;
    if (area > 46340LL * 46340LL) {
        set_error("image clahe: a tile of %d x %d pixels overflows its int32 histogram", th, tw);
        return OBIA_E_UNSUPPORTED;
    }
    const int clip = std::max((int)(2.0 * (double)area / 256), 1);
    const float lut_scale = 255.0f / (float)(int)area;
    ctx->arena.reset();
    unsigned *hist = ctx->arena.get<unsigned>(64 * 256);
    uint8_t *lut = ctx->arena.get<uint8_t>(64 * 256);
    if (!hist || !lut) return OBIA_E_NOMEM;
    OBIA_HIP_TRY(hipMemsetAsync(hist, 0, 64 * 256 * sizeof(unsigned), ctx->stream));
    const int rows = (int)grids::image_clahe_hist_rows(th, tw);      // ~16 K pixels per workgroup; grid.y <= 65535
    hipLaunchKernelGGL(clahe_hist_kernel, to_dim3(grids::image_clahe_hist(th, tw)), dim3(256), 0, ctx->stream, in, H, W, nch, ch, th, tw, rows, hist);
    hipLaunchKernelGGL(clahe_lut_kernel, dim3(64), dim3(256), 0, ctx->stream, hist, clip, lut_scale, lut);
    hipLaunchKernelGGL(clahe_interp_kernel, to_dim3(grids::image_clahe_interp(H, W)), dim3(256), 0, ctx->stream, in, H, W, nch, ch, th, tw, lut,
                       out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_image_boundaries_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, uint8_t *out) {
    OBIA_TRY(enter(ctx));
    if (!labels || !out || H <= 0 || W <= 0 || W > MAX_W) { set_error("image boundaries: bad arguments"); return OBIA_E_INVALID; }
    hipLaunchKernelGGL(boundaries_kernel, to_dim3(grids::image_rows(H, W)), dim3(256), 0, ctx->stream, labels, H, W, out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_image_mark_u8_dev(obia_ctx *ctx, const uint8_t *image, int nch, const int32_t *labels, int H, int W, const uint8_t *table256,
                           const uint8_t *rgb3, uint8_t *out) {
    OBIA_TRY(enter(ctx));
    if (!image || !labels || !table256 || !rgb3 || !out || (nch != 1 && nch != 3) || H <= 0 || W <= 0 || W > MAX_W) {
        set_error("image mark: bad arguments (nch 1 or 3)");
        return OBIA_E_INVALID;
    }
    const uint32_t color = (uint32_t)rgb3[0] | ((uint32_t)rgb3[1] << 8) | ((uint32_t)rgb3[2] << 16);
    hipLaunchKernelGGL(mark_kernel, to_dim3(grids::image_rows(H, W)), dim3(256), 0, ctx->stream, image, nch, labels, H, W, table256, color, out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

}  // extern "C"
