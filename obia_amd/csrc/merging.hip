// merging.hip -- region merging on the segment graph alone (include/obia_merging.h): the fusion cost of every edge, the merge of the
// node tables of disjoint pairs, and the contraction of the CSR under a root column.  DESIGN.md 3.5x.
//
// The cost owns one lane per entry and the pair merge one lane per row, as the table kernels of adjacency.hip do: the order of a
// floating-point sum is part of its definition.  Both ends of an edge compute the cost from (min, max), so the two directions hold the
// same bits.
//
// The contraction is a segmented sort and reduce by key.  A first kernel adds up, per root row, the entries that go to it; the caller
// forms the prefix sum.  The count pass then (1) gathers: a group of 8 lanes per source row takes a ticket in the root row's cursor
// (an integer atomic) and copies its entries, mapped through root, to the root row's stretch of the scratch -- an entry that would
// point from the row to itself is kept as the key DROP, the largest int, so every stretch is filled; (2) sorts and combines every
// stretch where it lies, binned by length: up to 8 entries by a group of 8 lanes, up to 32 by a group of 32, an entry per lane in
// registers, ranked against the others of the group with shuffles; longer rows by a workgroup with a bitonic network whose
// comparators all point the same way, so that a row of any length is sorted as if it were padded with DROP to a power of two -- in LDS
// up to OBIA_MERGE_ROW_CAP entries, in the scratch itself above.  The order in which the tickets were taken decides where an entry
// lies before the sort and nothing after it: keys are sorted, equal keys are summed with integers.  The write pass is a copy.
//
// Nothing here takes memory from the context's workspace: every buffer is the caller's.  Every atomic is an integer atomic.
#include "csr.hpp"
#include "../../include/obia_merging.h"

#include <climits>

namespace obia {
namespace {

constexpr int CAP = OBIA_MERGE_ROW_CAP;
constexpr int DROP = INT_MAX;                                    // above every neighbour: N + 1 <= 2^31 - 2
static_assert((CAP & (CAP - 1)) == 0 && CAP >= 64, "the LDS sort takes a power of two");
static_assert((size_t)CAP * 12 + 256 * 4 + 257 * 8 + 64 <= 64 * 1024, "row and chunk tables fit the LDS of a workgroup");

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double canon(double x) { return x != x ? quiet_nan() : x; }

// a stretch of the scratch: raw_ptr[r] .. raw_ptr[r + 1] - 1, inside 0 .. nnz - 1
__device__ __forceinline__ void stretch(const long long *raw_ptr, int r, long long nnz, long long &lo, long long &hi) {
    lo = raw_ptr[r];
    hi = raw_ptr[r + 1];
    if (lo < 0) lo = 0;
    if (lo > nnz) lo = nnz;
    if (hi > nnz) hi = nnz;
    if (hi < lo) hi = lo;
}

struct Tables {
    const long long *area; const double *mean; const double *m2; int F; const long long *perimeter; const int *box;
};
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// ---- the fusion cost: a lane per entry ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void merge_cost_kernel(Csr G, Tables T, const double *__restrict__ w, double w_color, double w_compact,
                                                         double *__restrict__ cost) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < G.nnz; e += (long long)gridDim.x * 256) {
        const int j = G.neighbor[e];
        double out = quiet_nan();
        if (is_real(G, j)) {
            const int i = row_of(G, e);
            const long long a = i < j ? i : j, b = i < j ? j : i;
            const double fa = (double)T.area[a], fb = (double)T.area[b];
            const double fm = fa + fb;
            const double share = (fa * fb) / fm;
            double colour = 0.0;
            for (int f = 0; f < T.F; ++f) {
                const double ma = T.m2[a * T.F + f], mb = T.m2[b * T.F + f];
                const double d = T.mean[b * T.F + f] - T.mean[a * T.F + f];
                const double dd = d * d;
                const double cross = dd * share;
                const double mm = (ma + mb) + cross;
                const double sm = fm * __builtin_sqrt(mm / fm);
                const double sa = fa * __builtin_sqrt(ma / fa);
                const double sb = fb * __builtin_sqrt(mb / fb);
                const double h = sm - (sa + sb);
                const double wh = w[f] * h;
                colour = colour + wh;
            }
            const long long pa = T.perimeter[a], pb = T.perimeter[b];
            const double la = (double)pa, lb = (double)pb, lm = (double)(pa + pb - 2 * G.border[e]);
            const int *xa = T.box + a * 4, *xb = T.box + b * 4;
            const long long ha = (long long)xa[2] - xa[0], wa = (long long)xa[3] - xa[1];
            const long long hb = (long long)xb[2] - xb[0], wb = (long long)xb[3] - xb[1];
            const long long hm = (long long)imax(xa[2], xb[2]) - imin(xa[0], xb[0]), wm = (long long)imax(xa[3], xb[3]) - imin(xa[1], xb[1]);
            const double ba = 2.0 * (double)(ha + wa), bb = 2.0 * (double)(hb + wb), bm = 2.0 * (double)(hm + wm);
            const double ca = fa * (la / __builtin_sqrt(fa));
            const double cb = fb * (lb / __builtin_sqrt(fb));
            const double hc = fm * (lm / __builtin_sqrt(fm)) - (ca + cb);
            const double ta = fa * (la / ba);
            const double tb = fb * (lb / bb);
            const double hs = fm * (lm / bm) - (ta + tb);
            const double u = w_compact * hc;
            const double v = (1.0 - w_compact) * hs;
            const double shape = u + v;
            const double t1 = w_color * colour;
            const double t2 = (1.0 - w_color) * shape;
            out = canon(t1 + t2);
        }
        cost[e] = out;
    }
}

// ---- the merge of the node tables of every pair: a lane per row ---------------------------------------------------------------------
struct TablesOut {
    long long *area; double *mean; double *m2; long long *perimeter; int *box;
};
__device__ __forceinline__ int partner_of(const int *partner, int N, int i) {
    const int p = partner[i];
    if (p < 0 || p >= N || p == i) return -1;
    return partner[p] == i ? p : -1;
}
__global__ __launch_bounds__(256) void merge_pairs_kernel(Csr G, const int *__restrict__ partner, Tables T, TablesOut O) {
    const int F = T.F;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < G.N; i += (long long)gridDim.x * 256) {
        const long long p = partner_of(partner, G.N, (int)i);
        if (p < 0) {                                             // no partner: the row as it is
            O.area[i] = T.area[i];
            O.perimeter[i] = T.perimeter[i];
            for (int k = 0; k < 4; ++k) O.box[i * 4 + k] = T.box[i * 4 + k];
            for (int f = 0; f < F; ++f) {
                O.mean[i * F + f] = canon(T.mean[i * F + f]);
                O.m2[i * F + f] = canon(T.m2[i * F + f]);
            }
        } else if (p < i) {                                      // the larger of a pair: empty from now on
            O.area[i] = 0;
            O.perimeter[i] = 0;
            for (int k = 0; k < 4; ++k) O.box[i * 4 + k] = 0;
            for (int f = 0; f < F; ++f) {
                O.mean[i * F + f] = quiet_nan();
                O.m2[i * F + f] = quiet_nan();
            }
        } else {                                                 // the smaller: the union
            const long long a = i, b = p;
            const double fa = (double)T.area[a], fb = (double)T.area[b];
            const double fm = fa + fb;
            const double share = (fa * fb) / fm, step = fb / fm;
            for (int f = 0; f < F; ++f) {
                const double d = T.mean[b * F + f] - T.mean[a * F + f];
                const double dd = d * d;
                const double cross = dd * share;
                const double mm = (T.m2[a * F + f] + T.m2[b * F + f]) + cross;
                const double move = d * step;
                O.mean[a * F + f] = canon(T.mean[a * F + f] + move);
                O.m2[a * F + f] = canon(mm);
            }
            long long lo, hi, shared = 0;
            row_range(G, (int)a, lo, hi);
            for (long long e = lo; e < hi; ++e)
                if (G.neighbor[e] == (int)b) { shared = G.border[e]; break; }
            O.area[a] = T.area[a] + T.area[b];
            O.perimeter[a] = T.perimeter[a] + T.perimeter[b] - 2 * shared;
            O.box[a * 4] = imin(T.box[a * 4], T.box[b * 4]);
            O.box[a * 4 + 1] = imin(T.box[a * 4 + 1], T.box[b * 4 + 1]);
            O.box[a * 4 + 2] = imax(T.box[a * 4 + 2], T.box[b * 4 + 2]);
            O.box[a * 4 + 3] = imax(T.box[a * 4 + 3], T.box[b * 4 + 3]);
        }
    }
}

// ---- contraction ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool in_rows(int r, int N) { return r >= 0 && r < N; }

__global__ __launch_bounds__(256) void contract_rows_kernel(Csr G, const int *__restrict__ root, unsigned long long *raw_count) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < G.N; i += (long long)gridDim.x * 256) {
        const int r = root[i];
        if (!in_rows(r, G.N)) continue;
        long long lo, hi;
        row_range(G, (int)i, lo, hi);
        if (hi > lo) atomicAdd(&raw_count[r], (unsigned long long)(hi - lo));
    }
}

// a group of 8 lanes per source row: a ticket in the root row's cursor, then the mapped entries into the root row's stretch
__global__ __launch_bounds__(256) void contract_gather_kernel(Csr G, const int *__restrict__ root, const long long *__restrict__ raw_ptr,
                                                              int *cursor, int *__restrict__ key_work, long long *__restrict__ border_work) {
    const int gl = threadIdx.x & 7;
    const long long groups = (long long)gridDim.x * 32;
    for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) >> 3; i < G.N; i += groups) {
        const int r = root[i];
        if (!in_rows(r, G.N)) continue;                          // the same in all 8 lanes
        long long lo, hi;
        row_range(G, (int)i, lo, hi);
        const long long len = hi - lo;
        if (len <= 0) continue;
        int base = 0;
        if (gl == 0) base = atomicAdd(&cursor[r], (int)len);
        base = __shfl(base, 0, 8);
        long long s_lo, s_hi;
        stretch(raw_ptr, r, G.nnz, s_lo, s_hi);
        for (long long k = gl; k < len; k += 8) {
            const int j = G.neighbor[lo + k];
            int key;
            if (is_real(G, j)) {
                const int rj = root[j];
                key = (!in_rows(rj, G.N) || rj == r) ? DROP : rj;
            } else {
                key = j == G.N ? G.N : G.N + 1;
            }
            const long long dst = s_lo + (long long)base + k;
            if (dst >= s_lo && dst < s_hi) {
                key_work[dst] = key;
                border_work[dst] = G.border[lo + k];
            }
        }
    }
}

// rows of more than LO and at most GROUP gathered entries: an entry per lane, ranked against the others of its group
template <int GROUP, int LO> __global__ __launch_bounds__(256) void contract_sort_group_kernel(int N, long long nnz, const long long *__restrict__ raw_ptr,
                                                                                               int *key_work, long long *border_work,
                                                                                               int *__restrict__ count) {
    static_assert(GROUP == 8 || GROUP == 32, "a group is a part of a wave");
    const int gl = threadIdx.x & (GROUP - 1);
    const int first = (threadIdx.x & 63) & ~(GROUP - 1);         // the group's first lane in its wave
    const long long groups = (long long)gridDim.x * (256 / GROUP);
    for (long long r = ((long long)blockIdx.x * 256 + threadIdx.x) / GROUP; r < N; r += groups) {
        long long lo, hi;
        stretch(raw_ptr, (int)r, nnz, lo, hi);
        const long long L = hi - lo;
        if (L <= LO || L > GROUP) continue;                      // the same in every lane of the group
        int key = DROP;
        long long b = 0;
        if (gl < L) { key = key_work[lo + gl]; b = border_work[lo + gl]; }
        long long sum = 0;
        bool earlier = false;
#pragma unroll
        for (int t = 0; t < GROUP; ++t) {
            const int kt = __shfl(key, t, GROUP);
            const long long bt = __shfl(b, t, GROUP);
            const bool same = kt == key;
            if (same) sum += bt;
            earlier = earlier || (same && t < gl);
        }
        const bool head = key != DROP && !earlier;
        int pos = 0;
#pragma unroll
        for (int t = 0; t < GROUP; ++t) {
            const int kt = __shfl(key, t, GROUP);
            const int ht = __shfl((int)head, t, GROUP);
            pos += (ht && kt < key) ? 1 : 0;
        }
        const unsigned long long heads = (__ballot(head) >> first) & ((1ull << GROUP) - 1ull);
        if (head) {                                              // every lane of the wave has loaded by now: the stores cannot overtake a load
            key_work[lo + pos] = key;
            border_work[lo + pos] = sum;
        }
        if (gl == 0) count[r] = __popcll(heads);
    }
}

// one compare-exchange step of the network over the pairs t = tid, tid + 256, ...: the smaller key goes to the lower index
__device__ __forceinline__ void exchange(int *keys, long long *bors, long long i, long long j, long long L) {
    if (j >= L) return;                                          // an entry past the row is DROP and stays
    const int ki = keys[i], kj = keys[j];
    if (kj < ki) {
        keys[i] = kj; keys[j] = ki;
        const long long bi = bors[i], bj = bors[j];
        bors[i] = bj; bors[j] = bi;
    }
}
// bitonic network with every comparator ascending (the first step of a merge mirrors, the others shift): sorts keys[0 .. L) for any L
__device__ void sort_row(int *keys, long long *bors, long long L, int tid) {
    long long P = 1;
    while (P < L) P <<= 1;
    const long long pairs = P >> 1;
    for (long long k = 2; k <= P; k <<= 1) {
        const long long half = k >> 1;
        for (long long t = tid; t < pairs; t += 256) {
            const long long block = t / half, off = t - block * half;
            exchange(keys, bors, block * k + off, block * k + k - 1 - off, L);
        }
        __syncthreads();
        for (long long s = half >> 1; s >= 1; s >>= 1) {
            for (long long t = tid; t < pairs; t += 256) {
                const long long i = 2 * s * (t / s) + t % s;
                exchange(keys, bors, i, i + s, L);
            }
            __syncthreads();
        }
    }
}

// rows of more than 32 gathered entries: a workgroup per row.  256 rows are looked at per trip, a lane each.
__global__ __launch_bounds__(256) void contract_sort_block_kernel(int N, long long nnz, const long long *__restrict__ raw_ptr, int *key_work,
                                                                  long long *border_work, int *__restrict__ count) {
    __shared__ int skey[CAP];
    __shared__ long long sbor[CAP];
    __shared__ int ck[256];
    __shared__ unsigned long long acc[257];
    __shared__ int wave_heads[4];
    __shared__ int is_long[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long r0 = (long long)blockIdx.x * 256; r0 < N; r0 += (long long)gridDim.x * 256) {
        int mine = 0;
        if (r0 + tid < N) {
            long long lo, hi;
            stretch(raw_ptr, (int)(r0 + tid), nnz, lo, hi);
            mine = hi - lo > 32;
        }
        is_long[tid] = mine;
        if (!__syncthreads_or(mine)) continue;
        for (int q = 0; q < 256; ++q) {
            if (!is_long[q]) continue;                           // the same in every lane
            const long long r = r0 + q;
            long long lo, hi;
            stretch(raw_ptr, (int)r, nnz, lo, hi);
            const long long L = hi - lo;
            int *gk = key_work + lo;
            long long *gb = border_work + lo;
            int *keys = gk;
            long long *bors = gb;
            if (L <= CAP) {
                for (long long t = tid; t < L; t += 256) { skey[t] = gk[t]; sbor[t] = gb[t]; }
                keys = skey;
                bors = sbor;
            }
            __syncthreads();
            sort_row(keys, bors, L, tid);
            // combine runs of equal keys, 256 entries at a time; the output never passes the input it has not read yet
            long long base = 0;
            int carry = DROP;
            for (long long c0 = 0; c0 < L; c0 += 256) {
                const long long i = c0 + tid;
                const bool valid = i < L;
                const int k = valid ? keys[i] : DROP;
                const long long b = valid ? bors[i] : 0;
                ck[tid] = k;
                acc[tid] = 0ull;
                if (tid == 0) acc[256] = 0ull;
                __syncthreads();
                const int prev = tid ? ck[tid - 1] : carry;
                const bool live = k != DROP;
                const bool head = live && (i == 0 || k != prev);
                const unsigned long long m = __ballot(head);
                if (lane == 0) wave_heads[wave] = __popcll(m);
                __syncthreads();
                int slot = __popcll(m & ((2ull << lane) - 1ull)), total = 0;
                for (int v = 0; v < 4; ++v) {
                    if (v < wave) slot += wave_heads[v];
                    total += wave_heads[v];
                }
                if (live) atomicAdd(&acc[slot], (unsigned long long)b);   // slot 0: the run goes on from the chunk before
                carry = ck[255];
                __syncthreads();
                if (head) {
                    gk[base + slot - 1] = k;
                    gb[base + slot - 1] = (long long)acc[slot];
                }
                if (tid == 0 && base > 0 && acc[0] != 0ull) gb[base - 1] += (long long)acc[0];
                base += total;
                __syncthreads();
            }
            if (tid == 0) count[r] = (int)base;
        }
        __syncthreads();
    }
}

// the write pass: a group of 8 lanes copies the combined row to where the prefix sum of the counts puts it
__global__ __launch_bounds__(256) void contract_write_kernel(int N, long long nnz, const long long *__restrict__ raw_ptr, const int *__restrict__ count,
                                                             const int *__restrict__ key_work, const long long *__restrict__ border_work,
                                                             const long long *__restrict__ indptr_out, long long nnz_out,
                                                             int *__restrict__ neighbor_out, long long *__restrict__ border_out) {
    const int gl = threadIdx.x & 7;
    const long long groups = (long long)gridDim.x * 32;
    for (long long r = ((long long)blockIdx.x * 256 + threadIdx.x) >> 3; r < N; r += groups) {
        long long lo, hi;
        stretch(raw_ptr, (int)r, nnz, lo, hi);
        long long c = count[r];
        if (c > hi - lo) c = hi - lo;
        const long long at = indptr_out[r];
        for (long long k = gl; k < c; k += 8) {
            const long long dst = at + k;
            if (dst >= 0 && dst < nnz_out) {
                neighbor_out[dst] = key_work[lo + k];
                border_out[dst] = border_work[lo + k];
            }
        }
    }
}

// the node tables of a call, read or written: every column whenever there is a row
Buffers &list_tables(Buffers &b, int32_t N, const int64_t *area, const double *mean, const double *m2, const int64_t *perimeter, const int32_t *box) {
    return b.in(area, N > 0).in(mean, N > 0).in(m2, N > 0).in(perimeter, N > 0).in(box, N > 0);
}
Buffers &list_tables_out(Buffers &b, int32_t N, int64_t *area, double *mean, double *m2, int64_t *perimeter, int32_t *box) {
    return b.out(area, N > 0).out(mean, N > 0).out(m2, N > 0).out(perimeter, N > 0).out(box, N > 0);
}
Tables tables_of(const int64_t *area, const double *mean, const double *m2, int F, const int64_t *perimeter, const int32_t *box) {
    return Tables{reinterpret_cast<const long long *>(area), mean, m2, F, reinterpret_cast<const long long *>(perimeter), box};
}

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_merge_cost_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t n_labels, int64_t nnz,
                        const int64_t *area, const double *mean, const double *m2, int F, const double *band_weights,
                        const int64_t *perimeter, const int32_t *box, double w_color, double w_compact, double *cost_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"merging", "cost"};
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.count("F", F, 1));
    OBIA_TRY(refuse.count("nnz", nnz, 0));
    OBIA_TRY(refuse.count("n_labels * F", (int64_t)n_labels * F, 0));
    Buffers b;
    list_csr(b, indptr, neighbor, border, n_labels, nnz);
    if (list_tables(b, n_labels, area, mean, m2, perimeter, box).in(band_weights).out(cost_out, nnz > 0).bad()) return refuse.buffers();
    if (nnz == 0 || n_labels == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(merge_cost_kernel, to_dim3(grids::flat(nnz)), dim3(256), 0, ctx->stream, csr_of(indptr, neighbor, border, n_labels, nnz),
                           tables_of(area, mean, m2, F, perimeter, box), band_weights, w_color, w_compact, cost_out);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_merge_pairs_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t n_labels, int64_t nnz,
                         const int32_t *partner, const int64_t *area, const double *mean, const double *m2, int F, const int64_t *perimeter,
                         const int32_t *box, int64_t *area_out, double *mean_out, double *m2_out, int64_t *perimeter_out, int32_t *box_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"merging", "pairs"};
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.count("F", F, 1));
    OBIA_TRY(refuse.count("nnz", nnz, 0));
    OBIA_TRY(refuse.count("n_labels * F", (int64_t)n_labels * F, 0));
    Buffers b;
    list_csr(b, indptr, neighbor, border, n_labels, nnz).in(partner, n_labels > 0);
    list_tables(b, n_labels, area, mean, m2, perimeter, box);
    if (list_tables_out(b, n_labels, area_out, mean_out, m2_out, perimeter_out, box_out).bad()) return refuse.buffers();
    if (n_labels == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(merge_pairs_kernel, to_dim3(grids::flat(n_labels)), dim3(256), 0, ctx->stream, csr_of(indptr, neighbor, border, n_labels, nnz),
                           partner, tables_of(area, mean, m2, F, perimeter, box),
                           TablesOut{reinterpret_cast<long long *>(area_out), mean_out, m2_out, reinterpret_cast<long long *>(perimeter_out), box_out});
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_merge_contract_rows_dev(obia_ctx *ctx, const int64_t *indptr, int32_t n_labels, int64_t nnz, const int32_t *root,
                                 int64_t *raw_count_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"merging", "contract rows"};
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.count("nnz", nnz, 0));
    const bool rows = n_labels > 0;
    if (Buffers().out(raw_count_out, rows).in(indptr, rows).in(root, rows).bad()) return refuse.buffers();
    if (n_labels == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        OBIA_TRY(fill_async(ctx, raw_count_out, 0, (size_t)n_labels * sizeof(int64_t)));
        hipLaunchKernelGGL(contract_rows_kernel, to_dim3(grids::flat(n_labels)), dim3(256), 0, ctx->stream, csr_of(indptr, nullptr, nullptr, n_labels, nnz),
                           root, reinterpret_cast<unsigned long long *>(raw_count_out));
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_merge_contract_count_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t n_labels,
                                  int64_t nnz, const int32_t *root, const int64_t *raw_ptr, int32_t *key_work, int64_t *border_work,
                                  int32_t *cursor_work, int32_t *count_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"merging", "contract count"};
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.count("nnz", nnz, 0));
    const bool rows = n_labels > 0;
    Buffers b;
    list_csr(b, indptr, neighbor, border, n_labels, nnz).in(root, rows).in(raw_ptr, rows);
    if (b.out(key_work, nnz > 0).out(border_work, nnz > 0).out(cursor_work, rows).out(count_out, rows).bad()) return refuse.buffers();
    if (n_labels == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        const long long *ptr = reinterpret_cast<const long long *>(raw_ptr);
        long long *bw = reinterpret_cast<long long *>(border_work);
        OBIA_TRY(fill_async(ctx, cursor_work, 0, (size_t)n_labels * sizeof(int32_t)));
        if (nnz > 0) {
            hipLaunchKernelGGL(contract_gather_kernel, to_dim3(grids::flat((long long)n_labels * 8)), dim3(256), 0, ctx->stream,
                               csr_of(indptr, neighbor, border, n_labels, nnz), root, ptr, cursor_work, key_work, bw);
            OBIA_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL((contract_sort_group_kernel<8, -1>), to_dim3(grids::flat((long long)n_labels * 8)), dim3(256), 0, ctx->stream, n_labels,
                           (long long)nnz, ptr, key_work, bw, count_out);
        OBIA_HIP_TRY(hipGetLastError());
        if (nnz > 8) {
            hipLaunchKernelGGL((contract_sort_group_kernel<32, 8>), to_dim3(grids::flat((long long)n_labels * 32)), dim3(256), 0, ctx->stream, n_labels,
                               (long long)nnz, ptr, key_work, bw, count_out);
            OBIA_HIP_TRY(hipGetLastError());
        }
        if (nnz > 32) {
            hipLaunchKernelGGL(contract_sort_block_kernel, to_dim3(grids::flat(n_labels)), dim3(256), 0, ctx->stream, n_labels, (long long)nnz, ptr,
                               key_work, bw, count_out);
            OBIA_HIP_TRY(hipGetLastError());
        }
        return OBIA_OK;
    });
}

int obia_merge_contract_write_dev(obia_ctx *ctx, int32_t n_labels, int64_t nnz, const int64_t *raw_ptr, const int32_t *count,
                                  const int32_t *key_work, const int64_t *border_work, const int64_t *indptr_out, int64_t nnz_out,
                                  int32_t *neighbor_out, int64_t *border_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"merging", "contract write"};
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.count("nnz", nnz, 0));
    OBIA_TRY(refuse.count("nnz_out", nnz_out, 0));
    const bool rows = n_labels > 0;
    Buffers b;
    b.in(raw_ptr, rows).in(count, rows).in(key_work, nnz > 0).in(border_work, nnz > 0).in(indptr_out, rows);
    if (b.out(neighbor_out, nnz_out > 0).out(border_out, nnz_out > 0).bad()) return refuse.buffers();
    if (n_labels == 0 || nnz_out == 0 || nnz == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(contract_write_kernel, to_dim3(grids::flat((long long)n_labels * 8)), dim3(256), 0, ctx->stream, n_labels, (long long)nnz,
                           reinterpret_cast<const long long *>(raw_ptr), count, key_work, reinterpret_cast<const long long *>(border_work),
                           reinterpret_cast<const long long *>(indptr_out), (long long)nnz_out, neighbor_out,
                           reinterpret_cast<long long *>(border_out));
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

}  // extern "C"
