// points.hip -- point clouds (include/obia_points.h): points to the canopy height model and the density raster, points to the
// segments of a label raster, and the point-cloud columns of the objects table from that join.  DESIGN.md 3.5s.
//
// Everything a point adds is an integer -- a count, a sum of uint16 intensities or of their squares, a maximum on the key of a
// float32 -- and every update is an integer atomic, so the state is the same bits for every order of the points, every cut of the
// cloud into calls and every schedule.  The join is the hot path: a workgroup takes OBIA_POINTS_CHUNK consecutive points (scan order
// keeps the neighbours of the array in few segments), sums equal (row, bin) keys and equal rows in two LDS hash tables and then
// touches global memory once per occupied slot.  A key that finds no slot in a few probes is added to global memory directly.
#include "common.hpp"
#include "../../include/obia_points.h"

#include <climits>
#include <cmath>

namespace obia {
namespace {

constexpr int CHUNK = OBIA_POINTS_CHUNK, PT = OBIA_POINTS_TABLE, RT = OBIA_POINTS_ROWS, PROBES = OBIA_POINTS_PROBES;
static_assert((PT & (PT - 1)) == 0 && (RT & (RT - 1)) == 0, "the tables must be powers of two");
static_assert((size_t)PT * 8 + (size_t)RT * 28 <= 32 * 1024, "five workgroups of a CU share its LDS");
static_assert(CHUNK % 256 == 0 && (long long)CHUNK * 65535ll * 65535ll < (1ll << 62), "a chunk's sum of squares fits 64 bits");

struct Cloud {
    const double *x, *y;
    const float *z;
    const unsigned short *intensity;
    long long n;
    double a, b, d, e, xoff, yoff;
    int H, W;
};

// flat pixel index of point i, -1 outside: the rule of sample_labels_kernel (consumers.hip); a NaN fails every comparison
__device__ __forceinline__ long long pixel_of(const Cloud &C, long long i) {
    const double X = C.x[i], Y = C.y[i];
    const double col = floor(C.a * X + C.b * Y + C.xoff), row = floor(C.d * X + C.e * Y + C.yoff);
    if (col >= 0.0 && col < (double)C.W && row >= 0.0 && row < (double)C.H) return (long long)row * C.W + (long long)col;
    return -1;
}

// atomicMax on a value that only ever grows, skipped when a plain load already shows as much: the load may be stale, but a stale value
// is an earlier and so a smaller one, and then the atomic runs.  A running maximum of m points changes about ln(m) times, so most
// points of a populated pixel or segment cost a load instead of an atomic.
__device__ __forceinline__ void raise_max(unsigned *p, unsigned k) {
    if (*p < k) atomicMax(p, k);
}

__global__ __launch_bounds__(256) void points_rasters_kernel(Cloud C, unsigned *__restrict__ zk, unsigned *__restrict__ count) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < C.n; i += (long long)gridDim.x * 256) {
        const long long px = pixel_of(C, i);
        if (px < 0) continue;
        atomicAdd(&count[px], 1u);
        const float z = C.z[i];
        if (isfinite(z)) raise_max(&zk[px], zkey(z));
    }
}

__global__ __launch_bounds__(256) void points_finish_kernel(const unsigned *__restrict__ zk, const unsigned *__restrict__ count, long long npx,
                                                            float area, float *__restrict__ chm, float *__restrict__ density) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npx; i += (long long)gridDim.x * 256) {
        const unsigned k = zk[i];
        chm[i] = k ? zunkey(k) : __uint_as_float(0x7fc00000u);
        density[i] = (float)count[i] / area;
    }
}

struct SegArgs {
    Cloud C;
    const int *labels;
    int start_label, N, nz;
    double dz;
    unsigned *profile, *top, *n_int;
    unsigned long long *s1, *s2, *counters;
};

// the slot that holds `k1` (a key + 1; 0: empty) or takes it, -1 when PROBES slots from its home are held by other keys
__device__ __forceinline__ int claim(unsigned *keys, unsigned mask, unsigned k1, unsigned home) {
    unsigned slot = home & mask;
    for (int p = 0; p < PROBES; ++p) {
        const unsigned seen = atomicCAS(&keys[slot], 0u, k1);
        if (seen == 0u || seen == k1) return (int)slot;
        slot = (slot + 1) & mask;
    }
    return -1;
}

__global__ __launch_bounds__(256) void points_segments_kernel(SegArgs A) {
    __shared__ unsigned pkey[PT], pcnt[PT];                      // (row * nz + bin) + 1 and its count
    __shared__ unsigned rkey[RT], rtop[RT], rn[RT];              // row + 1, the largest key of z, the count of intensities
    __shared__ unsigned long long rs1[RT], rs2[RT];
    __shared__ unsigned long long s_counters[4];
    const int tid = threadIdx.x;
    const bool radiometric = A.C.intensity != nullptr;
    for (int i = tid; i < PT; i += 256) { pkey[i] = 0; pcnt[i] = 0; }
    for (int i = tid; i < RT; i += 256) { rkey[i] = 0; rtop[i] = 0; rn[i] = 0; rs1[i] = 0; rs2[i] = 0; }
    if (tid < 4) s_counters[tid] = 0;
    __syncthreads();
    unsigned n_outside = 0, n_norow = 0, n_range = 0, n_profile = 0;       // of this lane: below 2^31 / 256
    const long long n_chunks = (A.C.n + CHUNK - 1) / CHUNK;
    for (long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const long long lo = chunk * CHUNK, hi = lo + CHUNK < A.C.n ? lo + CHUNK : A.C.n;
        for (long long i = lo + tid; i < hi; i += 256) {
            const long long px = pixel_of(A.C, i);
            if (px < 0) { n_outside += 1; continue; }
            const long long s = (long long)A.labels[px] - (long long)A.start_label;
            if (s < 0 || s >= (long long)A.N) { n_norow += 1; continue; }
            const float z = A.C.z[i];
            int bin = -1;
            if (isfinite(z) && z >= 0.0f) {
                const double q = floor((double)z / A.dz);
                if (q < (double)A.nz) bin = (int)q;
            }
            if (bin >= 0) n_profile += 1; else n_range += 1;
            const unsigned zk = bin >= 0 ? zkey(z) : 0u;
            if (bin >= 0 || radiometric) {
                const unsigned long long v = radiometric ? (unsigned long long)A.C.intensity[i] : 0ull;
                const int slot = claim(rkey, RT - 1, (unsigned)s + 1u, ((unsigned)s * 2654435761u) >> 16);
                if (slot >= 0) {
                    if (bin >= 0) atomicMax(&rtop[slot], zk);
                    if (radiometric) {
                        atomicAdd(&rn[slot], 1u);
                        atomicAdd(&rs1[slot], v);
                        atomicAdd(&rs2[slot], v * v);
                    }
                } else {
                    if (bin >= 0) raise_max(&A.top[s], zk);
                    if (radiometric) {
                        atomicAdd(&A.n_int[s], 1u);
                        atomicAdd(&A.s1[s], v);
                        atomicAdd(&A.s2[s], v * v);
                    }
                }
            }
            if (bin >= 0) {
                const unsigned key = (unsigned)s * (unsigned)A.nz + (unsigned)bin;          // < N * nz < 2^31
                const int slot = claim(pkey, PT - 1, key + 1u, (key * 2654435761u) >> 15);
                if (slot >= 0) atomicAdd(&pcnt[slot], 1u);
                else atomicAdd(&A.profile[key], 1u);
            }
        }
        __syncthreads();
        // one global atomic per occupied slot and value; the lane that reads an entry clears it, so the tables are empty again
        for (int slot = tid; slot < PT; slot += 256) {
            const unsigned k1 = pkey[slot];
            if (!k1) continue;
            atomicAdd(&A.profile[k1 - 1u], pcnt[slot]);
            pkey[slot] = 0;
            pcnt[slot] = 0;
        }
        for (int slot = tid; slot < RT; slot += 256) {
            const unsigned k1 = rkey[slot];
            if (!k1) continue;
            const unsigned s = k1 - 1u;
            if (rtop[slot]) raise_max(&A.top[s], rtop[slot]);
            if (rn[slot]) {
                atomicAdd(&A.n_int[s], rn[slot]);
                atomicAdd(&A.s1[s], rs1[slot]);
                atomicAdd(&A.s2[s], rs2[slot]);
            }
            rkey[slot] = 0; rtop[slot] = 0; rn[slot] = 0; rs1[slot] = 0; rs2[slot] = 0;
        }
        __syncthreads();
    }
    if (n_outside) atomicAdd(&s_counters[0], (unsigned long long)n_outside);
    if (n_norow) atomicAdd(&s_counters[1], (unsigned long long)n_norow);
    if (n_range) atomicAdd(&s_counters[2], (unsigned long long)n_range);
    if (n_profile) atomicAdd(&s_counters[3], (unsigned long long)n_profile);
    __syncthreads();
    if (tid < 4 && s_counters[tid]) atomicAdd(&A.counters[tid], s_counters[tid]);
}

struct ColArgs {
    const unsigned *profile, *top, *n_int;
    const unsigned long long *s1, *s2;
    int N, nz, j0;
    double k, kdz;
    long long *n_points;
    double *ch, *pai, *fhd, *mean_i, *var_i, *pad;
};

__global__ __launch_bounds__(256) void points_columns_kernel(ColArgs A) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= A.N) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const unsigned *c = A.profile + s * A.nz;
    unsigned long long n_all = 0, n_below = 0;
    for (int j = 0; j < A.nz; ++j) {
        const unsigned long long cj = c[j];
        if (A.pad) {
            const unsigned long long T = n_all, E = n_all + cj;
            double v;
            if (E == 0) v = nan;
            else if (cj == 0) v = 0.0;
            else if (T == 0) v = nan;
            else v = log((double)E / (double)T) / A.kdz;
            A.pad[s * A.nz + j] = v;
        }
        n_all += cj;
        if (j < A.j0) n_below += cj;
    }
    const unsigned long long n_can = n_all - n_below;
    double h = 0.0;
    if (n_can)
        for (int j = A.j0; j < A.nz; ++j) {
            const unsigned cj = c[j];
            if (!cj) continue;
            const double p = (double)cj / (double)n_can;
            h = h + p * log(p);
        }
    A.n_points[s] = (long long)n_all;
    A.ch[s] = n_all ? (double)zunkey(A.top[s]) : nan;
    A.pai[s] = (n_all && n_below) ? log((double)n_all / (double)n_below) / A.k : nan;
    A.fhd[s] = n_can ? -h : nan;
    const unsigned long long n = A.n_int[s];
    double mean = nan, var = nan;
    if (n) {
        const unsigned long long a = A.s1[s], b = A.s2[s];
        const unsigned long long lo1 = n * b, hi1 = __umul64hi(n, b), lo2 = a * a, hi2 = __umul64hi(a, a);
        const unsigned long long lo = lo1 - lo2, hi = hi1 - hi2 - (lo1 < lo2 ? 1ull : 0ull);      // n s2 >= s1^2 (Cauchy-Schwarz)
        mean = (double)a / (double)n;
        var = ((double)hi * 18446744073709551616.0 + (double)lo) / ((double)n * (double)n);
    }
    A.mean_i[s] = mean;
    A.var_i[s] = var;
}

// the columns of a cloud: whenever there is a point
Buffers &list_cloud(Buffers &b, const double *x, const double *y, const float *z, int64_t n) { return b.in(x, n > 0).in(y, n > 0).in(z, n > 0); }
Cloud cloud_of(const double *x, const double *y, const float *z, const uint16_t *intensity, int64_t n, const double *t, int H, int W) {
    return Cloud{x, y, z, intensity, (long long)n, t[0], t[1], t[2], t[3], t[4], t[5], H, W};
}
bool positive(double v) { return std::isfinite(v) && v > 0.0; }

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_points_rasters_dev(obia_ctx *ctx, const double *x, const double *y, const float *z, int64_t n, const double *inv6, int H, int W,
                            uint32_t *zk, uint32_t *count) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"points", "rasters"};
    OBIA_TRY(refuse.n_or_none(n));
    Buffers b;
    if (!inv6 || list_cloud(b, x, y, z, n).out(zk).out(count).bad()) return refuse.buffers();
    OBIA_TRY(refuse.raster(H, W));
    if (n == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(points_rasters_kernel, dim3(flat_grid(n)), dim3(256), 0, ctx->stream, cloud_of(x, y, z, nullptr, n, inv6, H, W), zk,
                           count);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_points_rasters_finish_dev(obia_ctx *ctx, const uint32_t *zk, const uint32_t *count, int H, int W, double pixel_area, float *chm,
                                   float *density) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"points", "rasters finish"};
    if (Buffers().out(chm).out(density).in(zk).in(count).bad()) return refuse.buffers();
    OBIA_TRY(refuse.raster(H, W));
    if (!positive(pixel_area)) { set_error("points: rasters finish: pixel_area must be finite and positive, got %g", pixel_area); return OBIA_E_INVALID; }
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        const long long npx = (long long)H * W;
        hipLaunchKernelGGL(points_finish_kernel, dim3(flat_grid(npx)), dim3(256), 0, ctx->stream, zk, count, npx, (float)pixel_area, chm, density);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_points_segments_dev(obia_ctx *ctx, const double *x, const double *y, const float *z, const uint16_t *intensity, int64_t n,
                             const double *inv6, const int32_t *labels, int H, int W, int32_t start_label, int32_t N, int32_t nz, double dz,
                             uint32_t *profile, uint32_t *top, uint32_t *n_int, uint64_t *s1, uint64_t *s2, uint64_t *counters) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"points", "segments"};
    OBIA_TRY(refuse.n_or_none(n));
    Buffers b;
    list_cloud(b, x, y, z, n).in(intensity, OPTIONAL).in(labels);
    if (!inv6 || b.out(profile).out(top).out(n_int).out(s1).out(s2).out(counters).bad()) return refuse.buffers();
    OBIA_TRY(refuse.raster(H, W));
    if (N < 0 || nz < 1) { set_error("points: segments: N must not be negative and nz at least 1, got %d and %d", N, nz); return OBIA_E_INVALID; }
    if (nz > OBIA_POINTS_MAX_NZ) { set_error("points: segments: nz must not exceed %d, got %d", OBIA_POINTS_MAX_NZ, nz); return OBIA_E_UNSUPPORTED; }
    if ((long long)N * nz > (long long)INT_MAX) { set_error("points: segments: N * nz must be below 2^31, got %d x %d", N, nz); return OBIA_E_UNSUPPORTED; }
    if (!positive(dz)) { set_error("points: segments: dz must be finite and positive, got %g", dz); return OBIA_E_INVALID; }
    if (n == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        SegArgs A{};
        A.C = cloud_of(x, y, z, intensity, n, inv6, H, W);
        A.labels = labels; A.start_label = start_label; A.N = N; A.nz = nz; A.dz = dz;
        A.profile = profile; A.top = top; A.n_int = n_int;
        A.s1 = reinterpret_cast<unsigned long long *>(s1);
        A.s2 = reinterpret_cast<unsigned long long *>(s2);
        A.counters = reinterpret_cast<unsigned long long *>(counters);
        // every chunk its own workgroup up to five per CU of 256, which then take the chunks in turn
        const unsigned grid = (unsigned)grids::points_segments(n).x.n;
        hipLaunchKernelGGL(points_segments_kernel, dim3(grid), dim3(256), 0, ctx->stream, A);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_points_segment_columns_dev(obia_ctx *ctx, const uint32_t *profile, const uint32_t *top, const uint32_t *n_int, const uint64_t *s1,
                                    const uint64_t *s2, int32_t N, int32_t nz, double dz, double min_height, double k, int64_t *n_points,
                                    double *ch, double *pai, double *fhd, double *mean_intensity, double *variance_intensity, double *pad) {
    OBIA_TRY(enter(ctx));
    Buffers b;
    b.in(profile).in(top).in(n_int).in(s1).in(s2);
    if (b.out(n_points).out(ch).out(pai).out(fhd).out(mean_intensity).out(variance_intensity).out(pad, OPTIONAL).bad())
        return Refusal{"points", "segment columns"}.buffers();
    if (N < 1 || nz < 1) { set_error("points: segment columns: N and nz must be at least 1, got %d and %d", N, nz); return OBIA_E_INVALID; }
    if (nz > OBIA_POINTS_MAX_NZ) { set_error("points: segment columns: nz must not exceed %d, got %d", OBIA_POINTS_MAX_NZ, nz); return OBIA_E_UNSUPPORTED; }
    if ((long long)N * nz > (long long)INT_MAX) { set_error("points: segment columns: N * nz must be below 2^31, got %d x %d", N, nz); return OBIA_E_UNSUPPORTED; }
    if (!positive(dz) || !positive(k) || !std::isfinite(min_height)) {
        set_error("points: segment columns: dz and k must be finite and positive and min_height finite, got %g, %g, %g", dz, k, min_height);
        return OBIA_E_INVALID;
    }
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        ColArgs A{};
        A.profile = profile; A.top = top; A.n_int = n_int;
        A.s1 = reinterpret_cast<const unsigned long long *>(s1);
        A.s2 = reinterpret_cast<const unsigned long long *>(s2);
        A.N = N; A.nz = nz;
        A.j0 = (int)std::min(std::max(std::ceil(min_height / dz), 0.0), (double)nz);
        A.k = k; A.kdz = k * dz;
        A.n_points = reinterpret_cast<long long *>(n_points);
        A.ch = ch; A.pai = pai; A.fhd = fhd; A.mean_i = mean_intensity; A.var_i = variance_intensity; A.pad = pad;
        hipLaunchKernelGGL(points_columns_kernel, dim3(cdiv(N, 256)), dim3(256), 0, ctx->stream, A);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

}  // extern "C"
