// cost.hip -- the cost surface of obia/utils/cost.py (`make_cost_surface` and its layers) on gfx950.
//   bands     : one pass over the interleaved (H, W, 8) WorldView-3 raster -> the C band and 1 - ndvi(R, N1) (float32)
//   ndvi      : ndvi of two planes, float32 (the public `ndvi`)
//   sobel     : scipy.ndimage.sobel along both axes (mode "nearest"), then hypot, float32
//   select    : exact NaN-excluding order statistics of a float32 / float64 plane (radix select on order-preserving keys)
//   entropy   : uint8 quantisation of the C band + skimage's rank entropy over disk(3), float64
//   normalise : clip to (lo, hi), rescale, nan_to_num, float64 out (the public `normalise`)
//   combine   : the four normalised layers (label edges computed on the fly), weighted, clipped, float32
// Every stage restates the reference's arithmetic operation for operation (the library is built with -ffp-contract=off);
// the percentile interpolation itself runs on the host from the order statistics select returns.
#include "common.hpp"
#include "wave_ops.hpp"

#include <cmath>

namespace obia {
namespace {

// np.clip(x, lo, hi): max then min, a NaN x propagates, NaN bounds propagate, ties keep x
template <typename T> __device__ __forceinline__ T np_clip(T x, T lo, T hi) {
    const T m = (x != x) ? x : (x >= lo ? x : lo);
    return (m != m) ? m : (m <= hi ? m : hi);
}

// np.nan_to_num((np.clip(x, lo, hi) - lo) / (hi - lo)) in float64
__device__ __forceinline__ double stretch(double x, double lo, double hi) {
    const double v = (np_clip(x, lo, hi) - lo) / (hi - lo);
    if (v != v) return 0.0;
    if (v == INFINITY) return 1.7976931348623157e308;
    if (v == -INFINITY) return -1.7976931348623157e308;
    return v;
}

// np.clip((nir - red) / (nir + red + 1e-9), -1, 1) in float32 (1e-9 is a weak Python float: float32(1e-9))
__device__ __forceinline__ float ndvi_f32(float red, float nir) {
    const float eps = (float)1e-9;
    const float v = (nir - red) / ((nir + red) + eps);
    return np_clip(v, -1.0f, 1.0f);
}

// ---------------------------------------------------------------------------------------------------------------- bands
__global__ __launch_bounds__(256) void cost_bands_kernel(const float *__restrict__ hwc, long long n, float *__restrict__ pan,
                                                         float *__restrict__ gap) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float4 a = ld_stream_f4(hwc + 8 * i);        // C  B  G  Y
        const float4 b = ld_stream_f4(hwc + 8 * i + 4);    // R  RE N1 N2
        pan[i] = a.x;
        gap[i] = 1.0f - ndvi_f32(b.x, b.z);
    }
}

__global__ __launch_bounds__(256) void cost_ndvi_kernel(const float *__restrict__ red, const float *__restrict__ nir, long long n,
                                                        float *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) out[i] = ndvi_f32(red[i], nir[i]);
}

// ---------------------------------------------------------------------------------------------------------------- sobel
// scipy's correlate1d keeps each line in double and detects the symmetry of the weights: [-1, 0, 1] is evaluated as
// x[0] * 0 + (x[-1] - x[+1]) * -1, [1, 2, 1] as x[0] * 2 + (x[-1] + x[+1]) * 1; the first pass is stored as float32.
constexpr int SB_TW = grids::COST_SOBEL_TW, SB_TH = grids::COST_SOBEL_TH;

__device__ __forceinline__ float sobel_diff(float m, float c, float p) {
    return (float)(((double)c * 0.0) + (((double)m - (double)p) * -1.0));
}
__device__ __forceinline__ float sobel_smooth(float m, float c, float p) {
    return (float)(((double)c * 2.0) + (((double)m + (double)p) * 1.0));
}
// np.hypot in float32 (glibc hypotf): inf wins over NaN, otherwise the double square root rounded once
__device__ __forceinline__ float hypot_f32(float x, float y) {
    if (__builtin_isinf(x) || __builtin_isinf(y)) return INFINITY;
    const double xd = x, yd = y;
    return (float)__builtin_sqrt(xd * xd + yd * yd);
}

__global__ __launch_bounds__(256) void cost_sobel_kernel(const float *__restrict__ chm, int H, int W, float *__restrict__ grad) {
    __shared__ float t[SB_TH + 2][SB_TW + 3];
    const int x0 = blockIdx.x * SB_TW;
    for (int by = blockIdx.y; by * SB_TH < H; by += gridDim.y) {
        const int y0 = by * SB_TH;
        __syncthreads();
        for (int i = threadIdx.x; i < (SB_TH + 2) * (SB_TW + 2); i += 256) {
            const int ly = i / (SB_TW + 2), lx = i - ly * (SB_TW + 2);
            const int gy = min(max(y0 - 1 + ly, 0), H - 1), gx = min(max(x0 - 1 + lx, 0), W - 1);   // mode "nearest"
            t[ly][lx] = chm[(long long)gy * W + gx];
        }
        __syncthreads();
        const int tx = threadIdx.x & 63;
        const int x = x0 + tx;
        for (int r = threadIdx.x >> 6; r < SB_TH; r += 4) {
            const int y = y0 + r;
            if (y >= H || x >= W) continue;
            // dx: [-1, 0, 1] along x on rows y-1, y, y+1, then [1, 2, 1] along y;  dy: the other way round
            const float h0 = sobel_diff(t[r][tx], t[r][tx + 1], t[r][tx + 2]);
            const float h1 = sobel_diff(t[r + 1][tx], t[r + 1][tx + 1], t[r + 1][tx + 2]);
            const float h2 = sobel_diff(t[r + 2][tx], t[r + 2][tx + 1], t[r + 2][tx + 2]);
            const float v0 = sobel_diff(t[r][tx], t[r + 1][tx], t[r + 2][tx]);
            const float v1 = sobel_diff(t[r][tx + 1], t[r + 1][tx + 1], t[r + 2][tx + 1]);
            const float v2 = sobel_diff(t[r][tx + 2], t[r + 1][tx + 2], t[r + 2][tx + 2]);
            grad[(long long)y * W + x] = hypot_f32(sobel_smooth(h0, h1, h2), sobel_smooth(v0, v1, v2));
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- select
// Order statistics of the non-NaN values: keys that sort like the floats (sign bit flipped for positives, all bits for
// negatives), resolved digit by digit from the top.  Up to four target ranks (the two neighbours of each of the two
// virtual indices) are resolved in the same passes; targets that share their known prefix share one histogram, so an
// element feeds at most one.  Every pass also records the smallest and largest key of each prefix group: a group whose
// keys are all equal ends its targets at once, so tie-heavy planes (few distinct values) stop after one or two passes
// instead of walking all digits, and no candidate set is ever built.
constexpr int SEL_MAXB = 12;                 // widest digit: 4096 bins
constexpr int SEL_NB = 1 << SEL_MAXB;
constexpr int SEL_THREADS = grids::COST_SELECT_THREADS;

struct SelState {
    unsigned long long n;                    // valid (non-NaN) values        } read back together
    unsigned long long value[4];             // resolved keys of the targets  }
    unsigned long long rank[4];              // rank of each target inside its prefix group
    unsigned long long prefix[4];            // key bits resolved so far
    unsigned long long gprefix[4];           // prefix of each active group
    unsigned long long gmin[4], gmax[4];     // key range of each active group (this pass)
    int done[4];
    int group_of[4];
    int ngroups;
    int all_done;
};

template <typename F> struct KeyOf;
template <> struct KeyOf<float> {
    typedef uint32_t K;
    static constexpr int bits = 32, levels = 3;
    static constexpr int width(int l) { return l < 2 ? 11 : 10; }
    __device__ static K key(float v) {
        const uint32_t u = __float_as_uint(v);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
};
template <> struct KeyOf<double> {
    typedef uint64_t K;
    static constexpr int bits = 64, levels = 6;
    static constexpr int width(int l) { return l < 5 ? 12 : 4; }
    __device__ static K key(double v) {
        const uint64_t u = (uint64_t)__double_as_longlong(v);
        return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
    }
};
template <typename F> constexpr int consumed_bits(int l) { return l == 0 ? 0 : consumed_bits<F>(l - 1) + KeyOf<F>::width(l - 1); }

__global__ void sel_init_kernel(SelState *st, unsigned *hist) {
    for (int i = threadIdx.x; i < 4 * SEL_NB; i += blockDim.x) hist[i] = 0;
    if (threadIdx.x == 0) {
        st->n = 0;
        for (int t = 0; t < 4; ++t) {
            st->value[t] = st->rank[t] = st->prefix[t] = st->gprefix[t] = 0;
            st->gmin[t] = ~0ull;
            st->gmax[t] = 0;
            st->done[t] = 0;
            st->group_of[t] = 0;
        }
        st->ngroups = 1;
        st->all_done = 0;
    }
}

template <typename F, int L>
__global__ __launch_bounds__(SEL_THREADS) void sel_pass_kernel(const F *__restrict__ x, long long n, SelState *__restrict__ st,
                                                               unsigned *__restrict__ hist) {
    typedef KeyOf<F> KO;
    typedef typename KO::K K;
    constexpr int W = KO::width(L), NB = 1 << W;
    constexpr int CONS = consumed_bits<F>(L);
    constexpr int SHIFT = KO::bits - CONS - W;
    constexpr int VEC = 16 / sizeof(F);
    __shared__ unsigned h[4 * NB];
    if (st->all_done) return;
    const int ng = st->ngroups;
    K gp[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) gp[g] = (K)st->gprefix[g];
    for (int i = threadIdx.x; i < ng * NB; i += SEL_THREADS) h[i] = 0;
    __syncthreads();

    K lmin[4], lmax[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) { lmin[g] = ~(K)0; lmax[g] = 0; }
    const int lane = threadIdx.x & 63;

    auto one = [&](F v, bool in) {
        const bool valid = in && (v == v);
        const K k = KO::key(v);
        int g = -1;
        if constexpr (L == 0) {
            g = valid ? 0 : -1;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < ng && valid && (K)(k >> (KO::bits - CONS)) == gp[j]) g = j;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (g == j) { lmin[j] = k < lmin[j] ? k : lmin[j]; lmax[j] = k > lmax[j] ? k : lmax[j]; }
        const int slot = g < 0 ? -1 : g * NB + (int)((k >> SHIFT) & (K)(NB - 1));
        // lanes that hit the same bin as the first active lane add once (constant and few-valued planes)
        const unsigned long long act = __ballot(slot >= 0);
        if (act) {
            const int leader = __ffsll((long long)act) - 1;
            const int s0 = __shfl(slot, leader);
            const unsigned long long same = __ballot(slot == s0);
            if (slot == s0) {
                if (lane == leader) atomicAdd(&h[s0], (unsigned)__popcll(same));
            } else if (slot >= 0) {
                atomicAdd(&h[slot], 1u);
            }
        }
    };

    const long long nv = n / VEC;
    const long long stride = (long long)gridDim.x * SEL_THREADS;
    for (long long i = (long long)blockIdx.x * SEL_THREADS + threadIdx.x; i - threadIdx.x < nv; i += stride) {
        // the whole wave stays in the loop (ballots), lanes past the end feed nothing
        const bool in = i < nv;
        if (sizeof(F) == 4) {
            float4 q = in ? ld_stream_f4(x + VEC * i) : make_float4(0.f, 0.f, 0.f, 0.f);
            one((F)q.x, in); one((F)q.y, in); one((F)q.z, in); one((F)q.w, in);
        } else {
            const double *p = reinterpret_cast<const double *>(x) + VEC * i;
            const double a = in ? p[0] : 0.0, b = in ? p[1] : 0.0;
            one((F)a, in); one((F)b, in);
        }
    }
    if (blockIdx.x == 0 && n > nv * VEC) {   // the last n % VEC values (uniform over the block)
        const long long i = nv * VEC + threadIdx.x;
        const bool in = i < n;
        one(in ? x[i] : (F)0, in);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ng * NB; i += SEL_THREADS)
        if (h[i]) atomicAdd(&hist[i], h[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned long long mn = lmin[j], mx = lmax[j];
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        if (lane == 0 && j < ng && mn <= mx) {
            atomicMin(&st->gmin[j], mn);
            atomicMax(&st->gmax[j], mx);
        }
    }
}

template <typename F, int L>
__global__ __launch_bounds__(256) void sel_resolve_kernel(SelState *__restrict__ st, unsigned *__restrict__ hist, double q_lo, double q_hi) {
    typedef KeyOf<F> KO;
    constexpr int W = KO::width(L), NB = 1 << W;
    constexpr int PER = NB >= 256 ? NB / 256 : 1;
    __shared__ unsigned long long s_chunk[256];
    __shared__ unsigned long long s_below;
    __shared__ int s_bin;
    __shared__ int s_stop;
    const int tid = threadIdx.x;
    if (st->all_done) return;
    if (L == 0) {
        unsigned long long c = 0;
        for (int b = tid * PER; b < (tid + 1) * PER && b < NB; ++b) c += hist[b];
        s_chunk[tid] = c;
        __syncthreads();
        if (tid == 0) {
            unsigned long long nn = 0;
            for (int i = 0; i < 256; ++i) nn += s_chunk[i];
            st->n = nn;
            s_stop = nn == 0;
            if (nn == 0) {
                st->all_done = 1;
            } else {
                // virtual index (n - 1) * q (np.quantile, method "linear"); at or past the last index both neighbours are the last value
                const double q[2] = {q_lo, q_hi};
                for (int k = 0; k < 2; ++k) {
                    const double v = (double)(nn - 1) * q[k];
                    unsigned long long a, b;
                    if (v >= (double)(nn - 1)) {
                        a = b = nn - 1;
                    } else {
                        a = (unsigned long long)floor(v);
                        b = a + 1;
                    }
                    st->rank[2 * k] = a;
                    st->rank[2 * k + 1] = b;
                }
            }
        }
        __syncthreads();
        if (s_stop) return;
    }
    for (int t = 0; t < 4; ++t) {
        if (st->done[t]) continue;                        // uniform: every thread reads the same word
        const int g = st->group_of[t];
        if (st->gmin[g] == st->gmax[g]) {                 // every key of the group is the same: that is the target
            __syncthreads();
            if (tid == 0) { st->value[t] = st->gmin[g]; st->done[t] = 1; }
            __syncthreads();
            continue;
        }
        const unsigned *hg = hist + g * NB;
        unsigned long long c = 0;
        for (int b = tid * PER; b < (tid + 1) * PER && b < NB; ++b) c += hg[b];
        s_chunk[tid] = c;
        __syncthreads();
        if (tid == 0) {                                   // exclusive scan of 256 chunk sums
            unsigned long long run = 0;
            for (int i = 0; i < 256; ++i) { const unsigned long long v = s_chunk[i]; s_chunk[i] = run; run += v; }
        }
        __syncthreads();
        const unsigned long long r = st->rank[t];
        const unsigned long long base = s_chunk[tid];
        if (tid * PER < NB && r >= base && (tid == 255 || r < s_chunk[tid + 1])) {
            unsigned long long below = base;
            for (int b = tid * PER; b < (tid + 1) * PER && b < NB; ++b) {
                if (r < below + hg[b]) { s_bin = b; s_below = below; break; }
                below += hg[b];
            }
        }
        __syncthreads();
        if (tid == 0) {
            st->prefix[t] = (st->prefix[t] << W) | (unsigned long long)s_bin;
            st->rank[t] = r - s_below;
            if (L == KO::levels - 1) { st->value[t] = st->prefix[t]; st->done[t] = 1; }
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0) {                                       // groups of the next pass: one per distinct prefix
        int ng = 0, left = 0;
        for (int t = 0; t < 4; ++t) {
            if (st->done[t]) continue;
            ++left;
            int g = -1;
            for (int j = 0; j < ng; ++j)
                if (st->gprefix[j] == st->prefix[t]) g = j;
            if (g < 0) { g = ng++; st->gprefix[g] = st->prefix[t]; }
            st->group_of[t] = g;
        }
        for (int j = 0; j < 4; ++j) { st->gmin[j] = ~0ull; st->gmax[j] = 0; }
        st->ngroups = ng;
        st->all_done = left == 0;
    }
    for (int i = tid; i < 4 * SEL_NB; i += 256) hist[i] = 0;
}

template <typename F, int L> void sel_launch_level(obia_ctx *ctx, const F *x, long long n, SelState *st, unsigned *hist, double q_lo,
                                                   double q_hi, int grid) {
    hipLaunchKernelGGL((sel_pass_kernel<F, L>), dim3(grid), dim3(SEL_THREADS), 0, ctx->stream, x, n, st, hist);
    hipLaunchKernelGGL((sel_resolve_kernel<F, L>), dim3(1), dim3(256), 0, ctx->stream, st, hist, q_lo, q_hi);
}

template <typename F> int sel_run(obia_ctx *ctx, const F *x, long long n, double q_lo, double q_hi, int64_t *n_valid, uint64_t *bits4) {
    ctx->arena.reset();
    SelState *st = ctx->arena.get<SelState>(1);
    unsigned *hist = ctx->arena.get<unsigned>(4 * SEL_NB);
    if (!st || !hist) return OBIA_E_NOMEM;
    const long long nv = n / (16 / (long long)sizeof(F));
    const int grid = (int)grids::cost_select(nv).x.n;
    hipLaunchKernelGGL(sel_init_kernel, dim3(1), dim3(256), 0, ctx->stream, st, hist);
    sel_launch_level<F, 0>(ctx, x, n, st, hist, q_lo, q_hi, grid);
    sel_launch_level<F, 1>(ctx, x, n, st, hist, q_lo, q_hi, grid);
    sel_launch_level<F, 2>(ctx, x, n, st, hist, q_lo, q_hi, grid);
    if constexpr (KeyOf<F>::levels > 3) {
        sel_launch_level<F, 3>(ctx, x, n, st, hist, q_lo, q_hi, grid);
        sel_launch_level<F, 4>(ctx, x, n, st, hist, q_lo, q_hi, grid);
        sel_launch_level<F, 5>(ctx, x, n, st, hist, q_lo, q_hi, grid);
    }
    OBIA_HIP_TRY(hipGetLastError());
    unsigned long long h[5];                              // n, value[4]: the one read-back of the plane
    OBIA_TRY(read_back(ctx, h, st, sizeof(h)));
    *n_valid = (int64_t)h[0];
    typedef typename KeyOf<F>::K K;
    const K top = (K)1 << (KeyOf<F>::bits - 1);
    for (int t = 0; t < 4; ++t) {
        const K k = (K)h[1 + t];
        bits4[t] = (uint64_t)((k & top) ? (K)(k ^ top) : (K)~k);   // key -> the float's bits
    }
    return OBIA_OK;
}

// -------------------------------------------------------------------------------------------------------------- entropy
// skimage.filters.rank.entropy(u8, disk(3)): per pixel, the histogram of the 29 taps inside the image, then
// e -= p * log(p) / ln 2 over the grey levels in ascending order (p = count / pop).  The terms come from a host table
// T[pop][count] built with libm log; a lane sorts the taps of two vertically adjacent pixels at once (16-bit halves of one
// 32-bit word, packed min / max) and walks the sorted runs.
constexpr int EN_TW = grids::COST_ENTROPY_TW, EN_TH = grids::COST_ENTROPY_TH, EN_R = 3;
constexpr int EN_LW = EN_TW + 2 * EN_R, EN_LH = EN_TH + 2 * EN_R;
constexpr int EN_TCOLS = 32;                  // T is [30][32]; T[p][0] = 0 (a step that ends no run subtracts zero)

typedef unsigned short en_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
    const en_u16x2 r = __builtin_elementwise_min(__builtin_bit_cast(en_u16x2, a), __builtin_bit_cast(en_u16x2, b));
    return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {
    const en_u16x2 r = __builtin_elementwise_max(__builtin_bit_cast(en_u16x2, a), __builtin_bit_cast(en_u16x2, b));
    return __builtin_bit_cast(uint32_t, r);
}

// taps of disk(3) inside a raster of H x W around (y, x)
__device__ __forceinline__ int disk3_pop(int y, int x, int H, int W) {
    if (y >= EN_R && y + EN_R < H && x >= EN_R && x + EN_R < W) return 29;
    int c = 0;
#pragma unroll
    for (int dy = -EN_R; dy <= EN_R; ++dy) {
        const int r = (dy == 0) ? 3 : (dy == -3 || dy == 3) ? 0 : 2;
        if (y + dy < 0 || y + dy >= H) continue;
        c += min(W - 1, x + r) - max(0, x - r) + 1;
    }
    return c;
}

__global__ __launch_bounds__(256) void cost_entropy_kernel(const float *__restrict__ pan, int H, int W, double lo, double hi,
                                                           const double *__restrict__ table, double *__restrict__ out) {
    __shared__ unsigned short tile[EN_LH][EN_LW + 2];
    __shared__ double T[30 * EN_TCOLS];
    for (int i = threadIdx.x; i < 30 * EN_TCOLS; i += 256) T[i] = table[i];
    const int x0 = blockIdx.x * EN_TW;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int by = blockIdx.y; by * EN_TH < H; by += gridDim.y) {
        const int y0 = by * EN_TH;
        __syncthreads();
        for (int i = threadIdx.x; i < EN_LH * EN_LW; i += 256) {
            const int ly = i / EN_LW, lx = i - ly * EN_LW;
            const int gy = y0 - EN_R + ly, gx = x0 - EN_R + lx;
            unsigned short q = 0xFFFF;                    // outside the raster: sorts after every grey level, never counted
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                // (normalise(pan) * 255).astype(uint8), float64
                const double s = stretch((double)pan[(long long)gy * W + gx], lo, hi) * 255.0;
                q = (unsigned short)(s >= 255.0 ? 255 : s > 0.0 ? (int)s : 0);
            }
            tile[ly][lx] = q;
        }
        __syncthreads();
        const int x = x0 + tx;
#pragma unroll 1
        for (int pr = 0; pr < 2; ++pr) {
            const int r = ty * 4 + 2 * pr;                // output rows r and r + 1 of the tile
            const int y = y0 + r;
            if (x >= W || y >= H) continue;
            uint32_t v[32];
            int k = 0;
#pragma unroll
            for (int dy = -EN_R; dy <= EN_R; ++dy) {
                const int rr = (dy == 0) ? 3 : (dy == -3 || dy == 3) ? 0 : 2;
#pragma unroll
                for (int dx = -rr; dx <= rr; ++dx)
                    v[k++] = (uint32_t)tile[r + EN_R + dy][tx + EN_R + dx] | ((uint32_t)tile[r + 1 + EN_R + dy][tx + EN_R + dx] << 16);
            }
            v[29] = v[30] = v[31] = 0xFFFFFFFFu;
            // bitonic sort of 32 packed pairs
#pragma unroll
            for (int kk = 2; kk <= 32; kk <<= 1) {
#pragma unroll
                for (int j = kk >> 1; j > 0; j >>= 1) {
#pragma unroll
                    for (int i = 0; i < 32; ++i) {
                        const int l = i ^ j;
                        if (l > i) {
                            const uint32_t a = v[i], b = v[l];
                            if ((i & kk) == 0) { v[i] = pk_min(a, b); v[l] = pk_max(a, b); }
                            else { v[i] = pk_max(a, b); v[l] = pk_min(a, b); }
                        }
                    }
                }
            }
            const double *TA = T + disk3_pop(y, x, H, W) * EN_TCOLS;
            const double *TB = T + (y + 1 < H ? disk3_pop(y + 1, x, H, W) : 0) * EN_TCOLS;
            double eA = 0.0, eB = 0.0;
            int runA = 1, runB = 1;
            // v[29] is always a sentinel, so every run of grey levels ends inside 0..28
#pragma unroll
            for (int i = 0; i < 29; ++i) {
                const bool endA = (v[i] & 0xFFFFu) != (v[i + 1] & 0xFFFFu);
                const bool endB = (v[i] >> 16) != (v[i + 1] >> 16);
                eA -= TA[endA ? runA : 0];
                eB -= TB[endB ? runB : 0];
                runA = endA ? 1 : runA + 1;
                runB = endB ? 1 : runB + 1;
            }
            out[(long long)y * W + x] = eA;
            if (y + 1 < H) out[(long long)(y + 1) * W + x] = eB;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ normalise
template <typename F>
__global__ __launch_bounds__(256) void cost_normalise_kernel(const F *__restrict__ x, long long n, double lo, double hi,
                                                             double *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        out[i] = stretch((double)x[i], lo, hi);
}

// -------------------------------------------------------------------------------------------------------- edges, combine
__device__ __forceinline__ bool is_edge(const int32_t *__restrict__ lab, int H, int W, int y, int x, long long i) {
    const int32_t l = lab[i];
    return (x + 1 < W && lab[i + 1] != l) || (y + 1 < H && lab[i + W] != l);
}

__global__ __launch_bounds__(256) void cost_edge_count_kernel(const int32_t *__restrict__ lab, int H, int W,
                                                              unsigned long long *__restrict__ n_edge) {
    unsigned cnt = 0;
    for (int y = blockIdx.y; y < H; y += gridDim.y)
        for (int x = blockIdx.x * 256 + threadIdx.x; x < W; x += gridDim.x * 256) cnt += is_edge(lab, H, W, y, x, (long long)y * W + x);
    cnt = block_sum<256>(cnt);
    if (threadIdx.x == 0 && cnt) atomicAdd(n_edge, (unsigned long long)cnt);
}

struct CombineArgs {
    double lo[4], hi[4];     // grad, gap, tex, edge
    double w[4];
};

// cost = ((w_grad * grad + w_gap * gap) + w_tex * tex) + w_slic * edge in float64, clip(0, 1), float32, NaN -> -9999
__global__ __launch_bounds__(256) void cost_combine_kernel(const float *__restrict__ grad, const float *__restrict__ gap,
                                                           const double *__restrict__ tex, const int32_t *__restrict__ lab, int H,
                                                           int W, CombineArgs a, float *__restrict__ out) {
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        for (int x = blockIdx.x * 256 + threadIdx.x; x < W; x += gridDim.x * 256) {
            const long long i = (long long)y * W + x;
            const double g = stretch((double)grad[i], a.lo[0], a.hi[0]);
            const double p = stretch((double)gap[i], a.lo[1], a.hi[1]);
            const double t = stretch(tex[i], a.lo[2], a.hi[2]);
            const double e = lab ? stretch(is_edge(lab, H, W, y, x, i) ? 1.0 : 0.0, a.lo[3], a.hi[3]) : 0.0;
            const double c = np_clip(((a.w[0] * g + a.w[1] * p) + a.w[2] * t) + a.w[3] * e, 0.0, 1.0);
            const float f = (float)c;
            out[i] = (f != f) ? -9999.0f : f;
        }
    }
}

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_cost_bands_f32_dev(obia_ctx *ctx, const float *hwc8, int64_t n_pixels, float *pan_out, float *gap_out) {
    OBIA_TRY(enter(ctx));
    if (!hwc8 || !pan_out || !gap_out || n_pixels <= 0 || ((uintptr_t)hwc8 & 15)) {
        set_error("cost bands: bad arguments (the raster must be 16-byte aligned)");
        return OBIA_E_INVALID;
    }
    hipLaunchKernelGGL(cost_bands_kernel, dim3(flat_grid(n_pixels)), dim3(256), 0, ctx->stream, hwc8, (long long)n_pixels, pan_out, gap_out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_cost_ndvi_f32_dev(obia_ctx *ctx, const float *red, const float *nir, int64_t n, float *out) {
    OBIA_TRY(enter(ctx));
    if (!red || !nir || !out || n <= 0) { set_error("cost ndvi: bad arguments"); return OBIA_E_INVALID; }
    hipLaunchKernelGGL(cost_ndvi_kernel, dim3(flat_grid(n)), dim3(256), 0, ctx->stream, red, nir, (long long)n, out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_cost_sobel_f32_dev(obia_ctx *ctx, const float *chm, int H, int W, float *grad_out) {
    OBIA_TRY(enter(ctx));
    if (!chm || !grad_out || H <= 0 || W <= 0) { set_error("cost sobel: bad arguments"); return OBIA_E_INVALID; }
    hipLaunchKernelGGL(cost_sobel_kernel, to_dim3(grids::cost_sobel(H, W)), dim3(256), 0, ctx->stream, chm, H, W, grad_out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_cost_select_dev(obia_ctx *ctx, const void *plane, int is_f64, int64_t n, double q_lo, double q_hi, int64_t *n_valid_out,
                         uint64_t *bits4_out) {
    OBIA_TRY(enter(ctx));
    if (!plane || !n_valid_out || !bits4_out || n <= 0 || n >= (int64_t)0xFFFFFFFFll || ((uintptr_t)plane & 15)) {
        set_error("cost select: bad arguments (1 <= n < 2^32 values, 16-byte aligned)");
        return OBIA_E_INVALID;
    }
    return is_f64 ? sel_run<double>(ctx, (const double *)plane, n, q_lo, q_hi, n_valid_out, bits4_out)
                  : sel_run<float>(ctx, (const float *)plane, n, q_lo, q_hi, n_valid_out, bits4_out);
}

int obia_cost_entropy_f32_dev(obia_ctx *ctx, const float *pan, int H, int W, double lo, double hi, const double *table_30x32,
                              double *out) {
    OBIA_TRY(enter(ctx));
    if (!pan || !table_30x32 || !out || H <= 0 || W <= 0) { set_error("cost entropy: bad arguments"); return OBIA_E_INVALID; }
    hipLaunchKernelGGL(cost_entropy_kernel, to_dim3(grids::cost_entropy(H, W)), dim3(256), 0, ctx->stream, pan, H, W, lo, hi, table_30x32, out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_cost_normalise_dev(obia_ctx *ctx, const void *plane, int is_f64, int64_t n, double lo, double hi, double *out) {
    OBIA_TRY(enter(ctx));
    if (!plane || !out || n <= 0) { set_error("cost normalise: bad arguments"); return OBIA_E_INVALID; }
    const dim3 grid(flat_grid(n));
    if (is_f64)
        hipLaunchKernelGGL(cost_normalise_kernel<double>, grid, dim3(256), 0, ctx->stream, (const double *)plane, (long long)n, lo, hi, out);
    else
        hipLaunchKernelGGL(cost_normalise_kernel<float>, grid, dim3(256), 0, ctx->stream, (const float *)plane, (long long)n, lo, hi, out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_cost_edge_count_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, int64_t *n_edge_out) {
    OBIA_TRY(enter(ctx));
    if (!labels || !n_edge_out || H <= 0 || W <= 0) { set_error("cost edge count: bad arguments"); return OBIA_E_INVALID; }
    ctx->arena.reset();
    unsigned long long *d_n = ctx->arena.get<unsigned long long>(1);
    if (!d_n) return OBIA_E_NOMEM;
    OBIA_HIP_TRY(hipMemsetAsync(d_n, 0, sizeof(unsigned long long), ctx->stream));
    // a few thousand workgroups striding over the rows: one atomic each (a workgroup per row segment made one per 256 pixels,
    // and same-word atomics serialise device-wide)
    hipLaunchKernelGGL(cost_edge_count_kernel, to_dim3(grids::cost_edge_count(H, W)), dim3(256), 0, ctx->stream, labels, H, W, d_n);
    OBIA_HIP_TRY(hipGetLastError());
    unsigned long long h = 0;
    OBIA_TRY(read_back(ctx, &h, d_n, sizeof(h)));
    *n_edge_out = (int64_t)h;
    return OBIA_OK;
}

int obia_cost_combine_dev(obia_ctx *ctx, const float *grad, const float *gap, const double *tex, const int32_t *labels, int H, int W,
                          const double *lo4, const double *hi4, const double *w4, float *out) {
    OBIA_TRY(enter(ctx));
    if (!grad || !gap || !tex || !lo4 || !hi4 || !w4 || !out || H <= 0 || W <= 0) {
        set_error("cost combine: bad arguments");
        return OBIA_E_INVALID;
    }
    CombineArgs a;
    for (int k = 0; k < 4; ++k) { a.lo[k] = lo4[k]; a.hi[k] = hi4[k]; a.w[k] = w4[k]; }
    hipLaunchKernelGGL(cost_combine_kernel, to_dim3(grids::cost_rows(H, W)), dim3(256), 0, ctx->stream, grad, gap, tex, labels, H, W, a, out);
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

}  // extern "C"
