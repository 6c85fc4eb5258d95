// boxes.hip -- segments and detection boxes (include/obia_boxes.h): the area every segment shares with every box, the winning box of
// a segment, the dissolve by that assignment, IoU and greedy non-maximum suppression.  DESIGN.md 3.5r.
//
// On a label raster the join needs no geometry: the area a segment shares with an axis-aligned box is a sum over the segment's pixels
// of (column overlap) x (row overlap), and only the box's first and last column and row weigh other than 1.  One workgroup walks the
// footprint of one box and counts, per label, the pixels of the nine (column class, row class) combinations into a hash table in LDS
// with integer atomics; the area is formed from the nine counts in one fixed order.  The winner of a segment is found with two integer
// atomics on global memory -- a 64-bit maximum on the bit pattern of the area, then a minimum on the box index among the boxes that
// reach it -- so nothing depends on the schedule and two runs agree bit for bit.
#include "common.hpp"
#include "grid_cells.hpp"
#include "../../include/obia_boxes.h"

#include <climits>
#include <cmath>

namespace obia {
namespace {

constexpr int CAP = OBIA_BOXES_TABLE;                 // labels of the LDS table; a power of two
constexpr int NCNT = 10;                              // nine class counts and `meets`
static_assert((CAP & (CAP - 1)) == 0, "OBIA_BOXES_TABLE must be a power of two");
static_assert((size_t)CAP * (NCNT + 1) * 4 <= 60 * 1024, "the table must fit the LDS of one workgroup");

enum Mode { MODE_MAX = 0, MODE_MIN = 1, MODE_COUNT = 2, MODE_WRITE = 3 };
enum Flag { F_NONFINITE = 0, F_ORDER = 1, F_HUGE = 2, F_OVER = 3, F_BAD = 4, F_LIMIT = 5, N_FLAGS = 8 };
enum : unsigned char { ST_UNDECIDED = 0, ST_KEPT = 1, ST_NOT = 2 };

// first and last footprint index on an axis of N pixels; first > last: empty
__device__ __forceinline__ void footprint(double lo, double hi, int N, int &i0, int &i1) {
    i0 = (int)fmax(0.0, fmin(ceil(lo) - 1.0, (double)N));
    i1 = (int)fmin((double)(N - 1), fmax(floor(hi), -1.0));
}

// class of the footprint index c on an axis: 0 L / T, 1 I, 2 R / B, 3 Z
__device__ __forceinline__ int axis_class(int c, double lo, double hi) {
    const double a = (double)c, b = (double)c + 1.0;
    if (b == lo || a == hi) return 3;
    if (a < lo) return 0;
    if (b > hi) return 2;
    return 1;
}

__global__ __launch_bounds__(256) void boxes_check_kernel(const double *__restrict__ boxes, int n, int H, int W, int check_footprint,
                                                          int *__restrict__ flags) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;       // past n in the last workgroup: up to 2^31 + 254
    if (k >= n) return;
    const double x0 = boxes[4 * (long long)k], y0 = boxes[4 * (long long)k + 1], x1 = boxes[4 * (long long)k + 2],
                 y1 = boxes[4 * (long long)k + 3];
    if (!(isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1))) { flags[F_NONFINITE] = 1; return; }
    if (!(x0 <= x1 && y0 <= y1)) { flags[F_ORDER] = 1; return; }
    if (check_footprint) {
        int c0, c1, r0, r1;
        footprint(x0, x1, W, c0, c1);
        footprint(y0, y1, H, r0, r1);
        if (c1 >= c0 && r1 >= r0 && (long long)(c1 - c0 + 1) * (long long)(r1 - r0 + 1) > (long long)INT_MAX) flags[F_HUGE] = 1;
    }
}

struct WalkArgs {
    const int *labels; int H, W;
    const double *boxes; int n, n_labels;
    int *passes;                       // P of every box; MODE_MAX and MODE_COUNT double it where a pass did not fit
    unsigned char *pending;            // MODE_MAX, MODE_COUNT: boxes still to do (all of them when `first`)
    int first;
    unsigned long long *best;          // (n_labels + 1): bits(area) + 1 of the largest area, 0: no pair
    int *assigned;                     // (n_labels + 1): MODE_MIN
    long long *count_out;              // MODE_COUNT
    const long long *offset; long long total;          // MODE_WRITE
    int *box_out, *seg_out, *meets_out; double *area_out;
    int *flags;
};

template <int MODE> __global__ __launch_bounds__(256) void boxes_walk_kernel(WalkArgs A) {
    __shared__ int keys[CAP];
    __shared__ int cnt[CAP * NCNT];
    __shared__ int s_over, s_pairs;
    constexpr bool DETERMINES = MODE == MODE_MAX || MODE == MODE_COUNT;
    const int tid = threadIdx.x;
    bool clean = false;                // the table is all zero: an emit leaves it so, a walk that did not fit does not
    for (long long next = blockIdx.x; next < A.n; next += gridDim.x) {      // a workgroup takes one box at a time
        const int b = (int)next;
        if (DETERMINES && !A.first && !A.pending[b]) continue;
        const double x0 = A.boxes[4 * (long long)b], y0 = A.boxes[4 * (long long)b + 1], x1 = A.boxes[4 * (long long)b + 2],
                     y1 = A.boxes[4 * (long long)b + 3];
        int c0, c1, r0, r1;
        footprint(x0, x1, A.W, c0, c1);
        footprint(y0, y1, A.H, r0, r1);
        if (c1 < c0 || r1 < r0) {
            if (tid == 0) {
                if (DETERMINES) A.pending[b] = 0;
                if (MODE == MODE_COUNT) A.count_out[b] = 0;
            }
            continue;
        }
        const unsigned fw = (unsigned)(c1 - c0 + 1), npix = fw * (unsigned)(r1 - r0 + 1);     // < 2^31: boxes_check_kernel
        // the one L / T and the one R / B index of a footprint are its first and its last
        const double wx[3] = {fmin(x1, (double)c0 + 1.0) - x0, 1.0, x1 - (double)c1};
        const double wy[3] = {fmin(y1, (double)r0 + 1.0) - y0, 1.0, y1 - (double)r1};
        const int pgiven = A.passes[b];
        const unsigned P = pgiven > 1 ? (unsigned)pgiven : 1u;
        // Every lane's last read of s_over and s_pairs for the box before lies in front of a barrier that lane 0 has passed: the one
        // that ends a pass, or the one on the way out of a walk that did not fit.  So this reset cannot overtake such a read.
        if (tid == 0) { s_over = 0; s_pairs = 0; }
        bool over = false;
        for (unsigned p = 0; p < P; ++p) {
            if (!clean) {
                for (int i = tid; i < CAP; i += 256) keys[i] = 0;
                for (int i = tid; i < CAP * NCNT; i += 256) cnt[i] = 0;
            }
            __syncthreads();
            for (unsigned t = tid; t < npix; t += 256) {
                const unsigned r = t / fw, c = t - r * fw;
                const int lab = A.labels[(long long)(r0 + (int)r) * A.W + (c0 + (int)c)];
                if (lab < 1 || lab > A.n_labels) continue;
                if (P > 1 && (unsigned)lab % P != p) continue;
                unsigned slot = ((unsigned)lab * 2654435761u) >> 16 & (CAP - 1);
                int probes = 0;
                for (; probes < CAP; ++probes) {
                    const int seen = atomicCAS(&keys[slot], 0, lab);
                    if (seen == 0 || seen == lab) break;
                    slot = (slot + 1) & (CAP - 1);
                }
                if (probes == CAP) { s_over = 1; continue; }
                const int ca = axis_class(c0 + (int)c, x0, x1), cb = axis_class(r0 + (int)r, y0, y1);
                atomicAdd(&cnt[slot * NCNT + 9], 1);
                if (ca < 3 && cb < 3) atomicAdd(&cnt[slot * NCNT + cb * 3 + ca], 1);
            }
            __syncthreads();
            clean = false;
            over = s_over != 0;                                  // the same in every lane: nothing writes it between the two barriers
            if (over) {
                __syncthreads();                                 // all lanes have read the flag before lane 0 goes on to the next box
                break;
            }
            for (int slot = tid; slot < CAP; slot += 256) {
                const int lab = keys[slot];
                if (!lab) continue;
                double area = 0.0;
                for (int j = 0; j < 3; ++j)
                    for (int i = 0; i < 3; ++i) {
                        const int nab = cnt[slot * NCNT + j * 3 + i];
                        if (nab) area = area + (wx[i] * wy[j]) * (double)nab;
                    }
                const unsigned long long akey = (unsigned long long)__double_as_longlong(area) + 1ull;
                if (MODE == MODE_MAX) {
                    atomicMax(&A.best[lab], akey);
                } else if (MODE == MODE_MIN) {
                    if (A.best[lab] == akey) atomicMin(&A.assigned[lab], b);
                } else if (MODE == MODE_COUNT) {
                    atomicAdd(&s_pairs, 1);
                } else {
                    const long long pos = A.offset[b] + (long long)atomicAdd(&s_pairs, 1);
                    if (pos >= 0 && pos < A.total) {
                        A.box_out[pos] = b;
                        A.seg_out[pos] = lab;
                        A.area_out[pos] = area;
                        A.meets_out[pos] = cnt[slot * NCNT + 9];
                    } else {
                        A.flags[F_BAD] = 1;
                    }
                }
                keys[slot] = 0;                                  // the lane that read an entry clears it: no full clear per box
                for (int i = 0; i < NCNT; ++i) cnt[slot * NCNT + i] = 0;
            }
            __syncthreads();
            clean = true;
        }
        if (tid != 0) continue;
        if (over) {
            if (DETERMINES) {
                if (P >= (1u << 30)) A.flags[F_LIMIT] = 1;
                A.passes[b] = (int)(P >= (1u << 30) ? P : 2 * P);
                A.pending[b] = 1;
                atomicAdd(&A.flags[F_OVER], 1);
            } else {
                A.flags[F_BAD] = 1;
            }
        } else {
            if (DETERMINES) A.pending[b] = 0;
            if (MODE == MODE_COUNT) A.count_out[b] = s_pairs;
        }
    }
}

__global__ __launch_bounds__(256) void boxes_fill_i32_kernel(int *__restrict__ p, long long n, int v) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) p[i] = v;
}

__global__ __launch_bounds__(256) void boxes_winner_kernel(const unsigned long long *__restrict__ best, long long n, int *__restrict__ assigned,
                                                           double *__restrict__ area) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const unsigned long long k = best[i];
        if (!k) assigned[i] = -1;
        area[i] = k ? __longlong_as_double((long long)(k - 1ull)) : 0.0;
    }
}

__global__ __launch_bounds__(256) void boxes_dissolve_kernel(const int *__restrict__ labels, long long n, const int *__restrict__ assigned,
                                                             int n_labels, int *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int l = labels[i];
        int v = 0;
        if (l >= 1 && l <= n_labels) {
            const int a = assigned[l];
            v = a >= 0 ? a + 1 : 0;
        }
        out[i] = v;
    }
}

// Python's max(a, b) and min(a, b) of two floats: the first unless the second is strictly beyond it
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }

// calculate_iou (obia/detection/utils.py:63-81) in float64, this order, nothing contracted
__device__ __forceinline__ double iou_of(const double *__restrict__ A, const double *__restrict__ B) {
    const double ax0 = A[0], ay0 = A[1], ax1 = A[2], ay1 = A[3], bx0 = B[0], by0 = B[1], bx1 = B[2], by1 = B[3];
    const double dw = py_min(ax1, bx1) - py_max(ax0, bx0), dh = py_min(ay1, by1) - py_max(ay0, by0);
    const double iw = dw > 0.0 ? dw : 0.0, ih = dh > 0.0 ? dh : 0.0;
    const double inter = iw * ih;
    const double area_a = (ax1 - ax0) * (ay1 - ay0), area_b = (bx1 - bx0) * (by1 - by0);
    return inter / (((area_a + area_b) - inter) + 1e-6);
}

__global__ __launch_bounds__(256) void boxes_iou_kernel(const double *__restrict__ a, long long na, const double *__restrict__ b, long long nb,
                                                        double *__restrict__ out) {
    for (long long i = blockIdx.y; i < na; i += gridDim.y)
        for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nb; j += (long long)gridDim.x * 256)
            out[i * nb + j] = iou_of(a + 4 * i, b + 4 * j);
}

// One round (seed_table.hip: seedtab_round_kernel): an undecided box with a kept earlier suppressor is not kept; one whose earlier
// suppressors are all decided, none of them kept, is kept; the others wait and are counted.
__global__ __launch_bounds__(256) void boxes_nms_round_kernel(const double *__restrict__ boxes, const int *__restrict__ pos,
                                                              const int *__restrict__ group, const long long *__restrict__ skey, int n,
                                                              long long ncx, double thr, const uint8_t *__restrict__ state_in,
                                                              uint8_t *__restrict__ state_out, int *remaining) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;       // past n in the last workgroup: up to 2^31 + 254
    bool waits = false;
    if (k < n) {
        unsigned char s = state_in[k];
        if (s == ST_UNDECIDED) {
            const double *mine = boxes + 4 * (long long)k;
            const int me = pos[k], g = group ? group[k] : 0;
            bool covered = false, pending = false;
            for_cells(skey, n, skey[k], ncx, [&](int q) {
                const unsigned char sq = state_in[q];
                if (sq != ST_NOT && pos[q] < me && (!group || group[q] == g) && iou_of(boxes + 4 * (long long)q, mine) > thr) {
                    covered |= sq == ST_KEPT;
                    pending |= sq == ST_UNDECIDED;
                }
            });
            s = covered ? ST_NOT : pending ? ST_UNDECIDED : ST_KEPT;
            waits = s == ST_UNDECIDED;
        }
        state_out[k] = s;
    }
    const unsigned long long m = __ballot(waits);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(remaining, __popcll(m));
}

__global__ __launch_bounds__(256) void boxes_nms_keep_kernel(const uint8_t *__restrict__ state, int n, uint8_t *__restrict__ keep_out) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;       // past n in the last workgroup: up to 2^31 + 254
    if (k < n) keep_out[k] = state[k] == ST_KEPT ? 1 : 0;
}

// the boxes are finite and ordered, and (with a raster) no footprint has 2^31 pixels or more; leaves flags (N_FLAGS ints) all zero
int check_boxes(obia_ctx *ctx, const char *what, const double *boxes, int64_t n, int H, int W, bool with_raster, int *flags) {
    OBIA_TRY(fill_async(ctx, flags, 0, N_FLAGS * sizeof(int)));
    hipLaunchKernelGGL(boxes_check_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, boxes, (int)n, H, W, with_raster ? 1 : 0, flags);
    OBIA_HIP_TRY(hipGetLastError());
    int f[N_FLAGS];
    OBIA_TRY(read_back(ctx, f, flags, sizeof f));
    if (f[F_NONFINITE]) { set_error("boxes: %s: a box coordinate is not finite", what); return OBIA_E_NONFINITE; }
    if (f[F_ORDER]) { set_error("boxes: %s: a box has x0 > x1 or y0 > y1", what); return OBIA_E_INVALID; }
    if (f[F_HUGE]) { set_error("boxes: %s: a box covers 2^31 pixels or more", what); return OBIA_E_UNSUPPORTED; }
    return OBIA_OK;
}

// workgroups of a walk: every box its own up to 4096, which then take the boxes in turn
unsigned walk_grid(int64_t n) { return (unsigned)grids::boxes_walk(n).x.n; }

// MODE_MAX or MODE_COUNT over all boxes, again over those a pass of which did not fit, P doubled, until none is left
template <int MODE> int walk_until_fit(obia_ctx *ctx, WalkArgs &A, int64_t n) {
    hipLaunchKernelGGL(boxes_fill_i32_kernel, dim3(flat_grid(n)), dim3(256), 0, ctx->stream, A.passes, (long long)n, 1);
    OBIA_HIP_TRY(hipGetLastError());
    A.first = 1;
    for (int attempt = 0;; ++attempt) {
        hipLaunchKernelGGL(boxes_walk_kernel<MODE>, dim3(walk_grid(n)), dim3(256), 0, ctx->stream, A);
        OBIA_HIP_TRY(hipGetLastError());
        int f[N_FLAGS];
        OBIA_TRY(read_back(ctx, f, A.flags, sizeof f));
        if (!f[F_OVER]) return OBIA_OK;
        if (f[F_LIMIT] || attempt >= 32) { set_error("boxes: a footprint did not fit the table in 2^30 passes"); return OBIA_E_INTERNAL; }
        OBIA_TRY(fill_async(ctx, A.flags, 0, N_FLAGS * sizeof(int)));
        A.first = 0;
    }
}

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_boxes_assign_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, const double *boxes, int64_t n, int32_t n_labels,
                          int32_t *assigned_out, double *area_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"boxes", "assign"};
    if (Buffers().out(assigned_out).out(area_out).in(labels).in(boxes).bad()) return refuse.buffers();
    OBIA_TRY(refuse.n(n));
    OBIA_TRY(refuse.raster(H, W, n_labels));
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        const long long m = (long long)n_labels + 1;
        WalkArgs A{};
        A.labels = labels; A.H = H; A.W = W; A.boxes = boxes; A.n = (int)n; A.n_labels = n_labels;
        A.flags = ctx->arena.get<int>(N_FLAGS);
        A.passes = ctx->arena.get<int>(n);
        A.pending = ctx->arena.get<unsigned char>(n);
        A.best = ctx->arena.get<unsigned long long>(m);
        A.assigned = assigned_out;
        if (!A.flags || !A.passes || !A.pending || !A.best) return OBIA_E_NOMEM;
        OBIA_TRY(check_boxes(ctx, "assign", boxes, n, H, W, true, A.flags));
        OBIA_TRY(fill_async(ctx, A.best, 0, m * sizeof(unsigned long long)));
        hipLaunchKernelGGL(boxes_fill_i32_kernel, dim3(flat_grid(m)), dim3(256), 0, ctx->stream, assigned_out, m, INT_MAX);
        OBIA_HIP_TRY(hipGetLastError());
        OBIA_TRY(walk_until_fit<MODE_MAX>(ctx, A, n));
        hipLaunchKernelGGL(boxes_walk_kernel<MODE_MIN>, dim3(walk_grid(n)), dim3(256), 0, ctx->stream, A);
        OBIA_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(boxes_winner_kernel, dim3(flat_grid(m)), dim3(256), 0, ctx->stream, (const unsigned long long *)A.best, m,
                           assigned_out, area_out);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_boxes_pair_count_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, const double *boxes, int64_t n, int32_t n_labels,
                              int64_t *count_out, int32_t *passes_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"boxes", "pair count"};
    if (Buffers().out(count_out).out(passes_out).in(labels).in(boxes).bad()) return refuse.buffers();
    OBIA_TRY(refuse.n(n));
    OBIA_TRY(refuse.raster(H, W, n_labels));
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        WalkArgs A{};
        A.labels = labels; A.H = H; A.W = W; A.boxes = boxes; A.n = (int)n; A.n_labels = n_labels;
        A.flags = ctx->arena.get<int>(N_FLAGS);
        A.pending = ctx->arena.get<unsigned char>(n);
        A.passes = passes_out;
        A.count_out = reinterpret_cast<long long *>(count_out);
        if (!A.flags || !A.pending) return OBIA_E_NOMEM;
        OBIA_TRY(check_boxes(ctx, "pair count", boxes, n, H, W, true, A.flags));
        return walk_until_fit<MODE_COUNT>(ctx, A, n);
    });
}

int obia_boxes_pair_write_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, const double *boxes, int64_t n, int32_t n_labels,
                              const int64_t *offset, const int32_t *passes, int64_t total, int32_t *box_out, int32_t *segment_out,
                              double *area_out, int32_t *meets_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"boxes", "pair write"};
    if (Buffers().out(box_out).out(segment_out).out(area_out).out(meets_out).in(labels).in(boxes).in(offset).in(passes).bad())
        return refuse.buffers();
    OBIA_TRY(refuse.n(n));
    OBIA_TRY(refuse.raster(H, W, n_labels));
    if (total < 1) { set_error("boxes: pair write: total must be at least 1, got %lld", (long long)total); return OBIA_E_INVALID; }
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        WalkArgs A{};
        A.labels = labels; A.H = H; A.W = W; A.boxes = boxes; A.n = (int)n; A.n_labels = n_labels;
        A.flags = ctx->arena.get<int>(N_FLAGS);
        if (!A.flags) return OBIA_E_NOMEM;
        A.passes = const_cast<int *>(passes);             // MODE_WRITE only reads it
        A.offset = reinterpret_cast<const long long *>(offset);
        A.total = total;
        A.box_out = box_out; A.seg_out = segment_out; A.area_out = area_out; A.meets_out = meets_out;
        OBIA_TRY(check_boxes(ctx, "pair write", boxes, n, H, W, true, A.flags));
        hipLaunchKernelGGL(boxes_walk_kernel<MODE_WRITE>, dim3(walk_grid(n)), dim3(256), 0, ctx->stream, A);
        OBIA_HIP_TRY(hipGetLastError());
        int f[N_FLAGS];
        OBIA_TRY(read_back(ctx, f, A.flags, sizeof f));
        if (f[F_BAD]) { set_error("boxes: pair write: offset, passes and total are not those of the count"); return OBIA_E_INVALID; }
        return OBIA_OK;
    });
}

int obia_boxes_dissolve_dev(obia_ctx *ctx, const int32_t *labels, int64_t npx, const int32_t *assigned, int32_t n_labels, int32_t *out) {
    OBIA_TRY(enter(ctx));
    if (Buffers().out(out).in(labels).in(assigned).bad()) return Refusal{"boxes", "dissolve"}.buffers();
    if (npx < 1) { set_error("boxes: dissolve: npx must be at least 1, got %lld", (long long)npx); return OBIA_E_INVALID; }
    if (n_labels < 0 || n_labels == INT_MAX) { set_error("boxes: dissolve: n_labels must be in 0 .. 2^31 - 2, got %d", n_labels); return OBIA_E_INVALID; }
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(boxes_dissolve_kernel, dim3(flat_grid(npx)), dim3(256), 0, ctx->stream, labels, (long long)npx, assigned, n_labels,
                           out);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_boxes_iou_dev(obia_ctx *ctx, const double *a, int64_t na, const double *b, int64_t nb, double *out) {
    OBIA_TRY(enter(ctx));
    if (Buffers().out(out).in(a).in(b).bad()) return Refusal{"boxes", "iou"}.buffers();
    if (na < 1 || nb < 1 || na > ((int64_t)1 << 62) / nb) {
        set_error("boxes: iou: na and nb must be at least 1 and na * nb below 2^62, got %lld x %lld", (long long)na, (long long)nb);
        return OBIA_E_INVALID;
    }
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        const dim3 grid = to_dim3(grids::boxes_iou(na, nb));
        hipLaunchKernelGGL(boxes_iou_kernel, grid, dim3(256), 0, ctx->stream, a, (long long)na, b, (long long)nb, out);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_boxes_nms_dev(obia_ctx *ctx, const double *boxes, const int32_t *pos, const int32_t *group, const int64_t *key, int64_t n,
                       int64_t ncx, double iou_threshold, uint8_t *keep_out, int32_t *rounds_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"boxes", "nms"};
    if (Buffers().out(keep_out).in(boxes).in(pos).in(group, OPTIONAL).in(key).bad()) return refuse.buffers();
    OBIA_TRY(refuse.n(n));
    if (ncx < 3) { set_error("boxes: nms: ncx must be at least 3, got %lld", (long long)ncx); return OBIA_E_INVALID; }
    if (!(iou_threshold >= 0.0)) { set_error("boxes: nms: iou_threshold must be at least 0, got %g", iou_threshold); return OBIA_E_INVALID; }
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        const int N = (int)n;
        int *flags = ctx->arena.get<int>(N_FLAGS);
        int *remaining = ctx->arena.get<int>(4);
        uint8_t *state[2] = {ctx->arena.get<uint8_t>(n), ctx->arena.get<uint8_t>(n)};
        if (!flags || !remaining || !state[0] || !state[1]) return OBIA_E_NOMEM;
        OBIA_TRY(check_boxes(ctx, "nms", boxes, n, 1, 1, false, flags));
        OBIA_TRY(fill_async(ctx, state[0], ST_UNDECIDED, n));
        const dim3 grid(cdiv(n, 256)), block(256);
        const long long *skey = reinterpret_cast<const long long *>(key);
        int64_t rounds = 0;
        int cur = 0;
        for (;;) {
            if (rounds >= n) {
                set_error("boxes: nms did not settle within n = %lld rounds", (long long)n);
                return OBIA_E_INTERNAL;
            }
            OBIA_TRY(fill_async(ctx, remaining, 0, 4 * sizeof(int)));
            hipLaunchKernelGGL(boxes_nms_round_kernel, grid, block, 0, ctx->stream, boxes, pos, group, skey, N, (long long)ncx, iou_threshold,
                               (const uint8_t *)state[cur], state[cur ^ 1], remaining);
            OBIA_HIP_TRY(hipGetLastError());
            int left = 0;
            OBIA_TRY(read_back(ctx, &left, remaining, sizeof(int)));
            cur ^= 1;
            rounds += 1;
            if (!left) break;
        }
        hipLaunchKernelGGL(boxes_nms_keep_kernel, grid, block, 0, ctx->stream, (const uint8_t *)state[cur], N, keep_out);
        OBIA_HIP_TRY(hipGetLastError());
        if (rounds_out) *rounds_out = (int32_t)rounds;
        return OBIA_OK;
    });
}

}  // extern "C"
