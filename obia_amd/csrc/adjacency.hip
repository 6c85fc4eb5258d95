// adjacency.hip -- which segments of a label raster touch each other (include/obia_adjacency.h): the shared pixel edges of every pair
// of 4-adjacent segments, and the small kernels that work on the resulting table.  DESIGN.md 3.5v.
//
// The one all-pixel pass runs twice, as the pair table of boxes.hip does: a COUNT pass says how many records a tile has, the caller
// forms the prefix sum, a WRITE pass puts them where they belong.  A workgroup of 256 stages a tile of TH x TW labels with one halo
// column and one halo row in LDS, already mapped to 0 .. N - 1 (segment), N (background) or N + 1 (outside the raster), and every
// pixel adds the edges it owns -- right, lower, and the frame's -- to a hash table in LDS with integer atomics: the key is the
// UNDIRECTED pair (lower index first; a pseudo-neighbour is always the higher), the value the number of edges.  A slot that is taken
// for the first time is noted in a list, so a tile is emitted and its slots are cleared by walking the list, not the table: a tile in
// the interior of a segment costs its loads and three barriers.  The table holds every pair a tile can own (3 per pixel at the most:
// right, lower, frame), so nothing overflows and nothing is done in passes.  A workgroup keeps its table over the tiles it walks.
//
// The table kernels take a CSR the caller built (torch: sort, segment sum) and own one lane per output element, because the order of
// a floating-point sum is part of its definition: a lane per entry (d2, with the row found by bisection of indptr; the links of the
// components), a lane per (row, feature) (neighbour statistics), a lane per row (border to class, best neighbour).  The components
// are the lock-free union-find of seeds.hip -- roots are the smallest members -- with path halving, in the caller's root array.
//
// Nothing here takes memory from the context's workspace: every buffer is the caller's.  Every atomic is an integer atomic.
#include "csr.hpp"
#include "../../include/obia_adjacency.h"

#include <climits>

namespace obia {
namespace {

constexpr int TH = OBIA_ADJ_TILE_H, TW = OBIA_ADJ_TILE_W, CAP = OBIA_ADJ_TABLE;
constexpr int SW = TW + 1, STAGED = (TH + 1) * SW;              // the staged tile: a halo column and a halo row
constexpr int MAXREC = 3 * TH * TW;                             // undirected pairs a tile owns at the most
static_assert((CAP & (CAP - 1)) == 0 && CAP > MAXREC && CAP <= 65536, "the table holds every pair of a tile; a slot index fits 16 bits");
static_assert((TH * TW) % 256 == 0, "whole trips of the workgroup over a tile");
static_assert((size_t)CAP * 12 + (size_t)MAXREC * 2 + (size_t)STAGED * 4 + 16 <= 64 * 1024, "table, list and tile fit the LDS of a workgroup");

enum { W_BAD = 0 };                                             // work[W_BAD]: offset / total are not those of the count

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

struct TileArgs {
    const int *labels; int H, W, start, N;
    int *count_out;                                             // COUNT
    const long long *offset; long long total;                   // WRITE
    long long *key_out; int *edges_out; int *work;
};

template <bool WRITE> __global__ __launch_bounds__(256) void adj_tile_kernel(TileArgs T) {
    __shared__ unsigned long long keys[CAP];                     // (lo + 1) << 32 | hi; 0: free
    __shared__ int cnt[CAP];
    __shared__ unsigned short list[MAXREC];                      // the slots taken, in the order they were taken
    __shared__ int lab[STAGED];
    __shared__ int s_n, s_rec;
    const int tid = threadIdx.x, N = T.N;
    for (int i = tid; i < CAP; i += 256) { keys[i] = 0ull; cnt[i] = 0; }
    if (tid == 0) { s_n = 0; s_rec = 0; }
    __syncthreads();
    const int ntx = (T.W + TW - 1) / TW, nty = (T.H + TH - 1) / TH;

    // k edges between x and y, each in 0 .. N + 1
    auto add = [&](int x, int y, int k) {
        if (x == y) return;
        const int lo = x < y ? x : y, hi = x < y ? y : x;
        if (lo >= N) return;                                     // background against outside
        const unsigned long long key = ((unsigned long long)(unsigned)(lo + 1) << 32) | (unsigned long long)(unsigned)hi;
        unsigned slot = (((unsigned)lo * 2654435761u) ^ ((unsigned)hi * 2246822519u)) >> 16 & (CAP - 1);
        for (int probes = 0; probes < CAP; ++probes) {           // ends at a free slot: CAP > MAXREC
            const unsigned long long seen = atomicCAS(&keys[slot], 0ull, key);
            if (seen == 0ull) {
                const int at = atomicAdd(&s_n, 1);
                if (at < MAXREC) list[at] = (unsigned short)slot;   // always: a tile owns no more pairs
            }
            if (seen == 0ull || seen == key) { atomicAdd(&cnt[slot], k); return; }
            slot = (slot + 1) & (CAP - 1);
        }
    };

    for (int ty = blockIdx.y; ty < nty; ty += gridDim.y)
        for (int tx = blockIdx.x; tx < ntx; tx += gridDim.x) {
            const int r0 = ty * TH, c0 = tx * TW;
            for (int i = tid; i < STAGED; i += 256) {
                const int r = i / SW, c = i - r * SW;
                const int gr = r0 + r, gc = c0 + c;
                int v = N + 1;
                if (gr < T.H && gc < T.W) {
                    const long long d = (long long)T.labels[(long long)gr * T.W + gc] - (long long)T.start;
                    v = (d >= 0 && d < (long long)N) ? (int)d : N;
                }
                lab[i] = v;
            }
            __syncthreads();
            for (int p = tid; p < TH * TW; p += 256) {
                const int r = p / TW, c = p - r * TW;
                const int gr = r0 + r, gc = c0 + c;
                if (gr >= T.H || gc >= T.W) continue;
                const int a = lab[r * SW + c];
                add(a, lab[r * SW + c + 1], 1);                  // past the last column the staged value is N + 1: the frame's right edge
                add(a, lab[(r + 1) * SW + c], 1);
                const int frame = (gc == 0) + (gr == 0);
                if (frame) add(a, N + 1, frame);
            }
            __syncthreads();
            const long long t = (long long)ty * ntx + tx;
            const int n = s_n < MAXREC ? s_n : MAXREC;
            const long long off = WRITE ? T.offset[t] : 0;
            for (int e = tid; e < n; e += 256) {
                const int slot = list[e];
                const unsigned long long key = keys[slot];
                const int lo = (int)(unsigned)(key >> 32) - 1, hi = (int)(unsigned)(key & 0xffffffffull);
                const int rows = hi < N ? 2 : 1;                 // a real pair in both directions
                const int at = atomicAdd(&s_rec, rows);
                if (WRITE) {
                    if (off >= 0 && off <= T.total && (long long)(at + rows) <= T.total - off) {
                        const long long m = (long long)N + 2;
                        T.key_out[off + at] = (long long)lo * m + hi;
                        T.edges_out[off + at] = cnt[slot];
                        if (rows == 2) {
                            T.key_out[off + at + 1] = (long long)hi * m + lo;
                            T.edges_out[off + at + 1] = cnt[slot];
                        }
                    } else {
                        T.work[W_BAD] = 1;
                    }
                }
                keys[slot] = 0ull;                               // the lane that read an entry clears it: no full clear per tile
                cnt[slot] = 0;
            }
            __syncthreads();
            if (tid == 0) {
                if (WRITE) {
                    const long long end = t + 1 < (long long)ntx * nty ? T.offset[t + 1] : T.total;
                    if ((t == 0 && off != 0) || off < 0 || off > T.total || end - off != (long long)s_rec) T.work[W_BAD] = 1;
                } else {
                    T.count_out[t] = s_rec;
                }
                s_n = 0;
                s_rec = 0;
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(256) void adj_d2_kernel(Csr G, const double *__restrict__ values, int F, double *__restrict__ d2) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < G.nnz; e += (long long)gridDim.x * 256) {
        const int j = G.neighbor[e];
        double acc = quiet_nan();
        if (is_real(G, j)) {
            const double *a = values + (long long)row_of(G, e) * F, *b = values + (long long)j * F;
            acc = 0.0;
            for (int f = 0; f < F; ++f) {
                const double d = a[f] - b[f];
                const double t = d * d;
                acc = acc + t;
            }
            if (acc != acc) acc = quiet_nan();
        }
        d2[e] = acc;
    }
}

__global__ __launch_bounds__(256) void adj_stats_kernel(Csr G, const double *__restrict__ values, int F, double *__restrict__ mean,
                                                        double *__restrict__ mn_out, double *__restrict__ mx_out, int *__restrict__ used_out) {
    const long long total = (long long)G.N * F;
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long long)gridDim.x * 256) {
        const int i = (int)(k / F), f = (int)(k - (long long)i * F);
        long long lo, hi;
        row_range(G, i, lo, hi);
        double sw = 0.0, s = 0.0, mn = 0.0, mx = 0.0;
        int used = 0;
        for (long long e = lo; e < hi; ++e) {
            const int j = G.neighbor[e];
            if (!is_real(G, j)) continue;
            const double v = values[(long long)j * F + f];
            if (v != v) continue;
            const double w = (double)G.border[e];
            sw = sw + w;
            const double wv = w * v;
            s = s + wv;
            if (!used || v < mn) mn = v;
            if (!used || v > mx) mx = v;
            used += 1;
        }
        double m = s / sw;
        if (!used || m != m) m = quiet_nan();
        mean[k] = m;
        mn_out[k] = used ? mn : quiet_nan();
        mx_out[k] = used ? mx : quiet_nan();
        used_out[k] = used;
    }
}

__global__ __launch_bounds__(256) void adj_class_border_kernel(Csr G, const int *__restrict__ classes, int K, long long *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < G.N; i += (long long)gridDim.x * 256) {
        long long *mine = out + i * K;                           // this lane's row: no other lane touches it
        for (int k = 0; k < K; ++k) mine[k] = 0;
        long long lo, hi;
        row_range(G, (int)i, lo, hi);
        for (long long e = lo; e < hi; ++e) {
            const int j = G.neighbor[e];
            if (!is_real(G, j)) continue;
            const int k = classes[j];
            if (k >= 0 && k < K) mine[k] += G.border[e];
        }
    }
}

__global__ __launch_bounds__(256) void adj_best_kernel(Csr G, const double *__restrict__ d2, int *__restrict__ best, double *__restrict__ best_d2) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < G.N; i += (long long)gridDim.x * 256) {
        long long lo, hi;
        row_range(G, (int)i, lo, hi);
        int b = -1;
        double bd = quiet_nan();
        for (long long e = lo; e < hi; ++e) {
            const int j = G.neighbor[e];
            if (!is_real(G, j)) continue;
            const double d = d2[e];
            if (d != d) continue;
            if (b < 0 || d < bd) { b = j; bd = d; }
        }
        best[i] = b;
        best_d2[i] = bd;
    }
}

// ---- union-find (seeds.hip): parent[v] <= v always, roots are the smallest members; reads go to the coherent level.  Path halving:
// a member that is no root is hung under its grandparent with an integer minimum -- an ancestor either way, and never itself again,
// so the compare-and-swap that hangs a ROOT under a smaller one cannot meet it.  A path of 70 000 members stays shallow.
__device__ __forceinline__ int uf_load(int *parent, int v) { return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int uf_find(int *parent, int v) {
    for (;;) {
        const int p = uf_load(parent, v);
        if (p == v) return v;
        const int g = uf_load(parent, p);
        if (g == p) return p;
        atomicMin(&parent[v], g);
        v = g;
    }
}
__device__ __forceinline__ void uf_unite(int *parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        if (atomicCAS(&parent[a], a, b) == a) return;            // a was still a root: it now hangs under the smaller root
    }
}

__global__ __launch_bounds__(256) void adj_iota_kernel(int *__restrict__ parent, int n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) parent[i] = (int)i;
}
__global__ __launch_bounds__(256) void adj_link_kernel(Csr G, const unsigned char *__restrict__ link, int *parent) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < G.nnz; e += (long long)gridDim.x * 256) {
        if (!link[e]) continue;
        const int j = G.neighbor[e];
        if (is_real(G, j)) uf_unite(parent, row_of(G, e), j);
    }
}
// in place: what a lane stores is an ancestor of its member, so a walk that crosses it still ends at the root
__global__ __launch_bounds__(256) void adj_flatten_kernel(int *parent, int n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        int v = (int)i, p = uf_load(parent, v);
        while (p != v) { v = p; p = uf_load(parent, v); }
        __hip_atomic_store(parent + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void adj_relabel_kernel(const int *__restrict__ labels, long long n, int start, int N, const int *__restrict__ map,
                                                          int *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int l = labels[i];
        const long long d = (long long)l - (long long)start;
        out[i] = d < 0 ? l : d < (long long)N ? map[d] : (int)((long long)start - 1);
    }
}

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_adj_tile_count_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, int32_t start_label, int32_t n_labels, int32_t *count_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"adjacency", "tile count"};
    if (Buffers().out(count_out).in(labels).bad()) return refuse.buffers();
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.raster_below_2_31(H, W));
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        TileArgs T{};
        T.labels = labels; T.H = H; T.W = W; T.start = start_label; T.N = n_labels; T.count_out = count_out;
        hipLaunchKernelGGL(adj_tile_kernel<false>, to_dim3(grids::adj_tiles(H, W)), dim3(256), 0, ctx->stream, T);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_adj_tile_write_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, int32_t start_label, int32_t n_labels, const int64_t *offset,
                            int64_t total, int64_t *key_out, int32_t *edges_out, int32_t *work) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"adjacency", "tile write"};
    if (Buffers().out(key_out, total > 0).out(edges_out, total > 0).out(work).in(labels).in(offset).bad()) return refuse.buffers();
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.raster_below_2_31(H, W));
    OBIA_TRY(refuse.count("total", total, 0));
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        TileArgs T{};
        T.labels = labels; T.H = H; T.W = W; T.start = start_label; T.N = n_labels;
        T.offset = reinterpret_cast<const long long *>(offset); T.total = total;
        T.key_out = reinterpret_cast<long long *>(key_out); T.edges_out = edges_out; T.work = work;
        OBIA_TRY(fill_async(ctx, work, 0, OBIA_ADJ_WORK * sizeof(int32_t)));
        hipLaunchKernelGGL(adj_tile_kernel<true>, to_dim3(grids::adj_tiles(H, W)), dim3(256), 0, ctx->stream, T);
        OBIA_HIP_TRY(hipGetLastError());
        int32_t w[OBIA_ADJ_WORK];
        OBIA_TRY(read_back(ctx, w, work, sizeof w));
        if (w[W_BAD]) { set_error("adjacency: tile write: offset and total are not those of the count"); return OBIA_E_INVALID; }
        return OBIA_OK;
    });
}

int obia_adj_edge_d2_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, int32_t n_labels, int64_t nnz, const double *values,
                         int F, double *d2_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"adjacency", "edge d2"};
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.count("F", F, 1));
    OBIA_TRY(refuse.count("nnz", nnz, 0));
    OBIA_TRY(refuse.count("n_labels * F", (int64_t)n_labels * F, 0));
    Buffers b;
    if (list_csr(b, indptr, neighbor, n_labels, nnz).in(values, n_labels > 0).out(d2_out, nnz > 0).bad()) return refuse.buffers();
    if (nnz == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(adj_d2_kernel, to_dim3(grids::flat(nnz)), dim3(256), 0, ctx->stream, csr_of(indptr, neighbor, nullptr, n_labels, nnz),
                           values, F, d2_out);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_adj_neighbor_stats_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t n_labels,
                                int64_t nnz, const double *values, int F, double *mean_out, double *min_out, double *max_out,
                                int32_t *used_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"adjacency", "neighbor stats"};
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.count("F", F, 1));
    OBIA_TRY(refuse.count("nnz", nnz, 0));
    OBIA_TRY(refuse.count("n_labels * F", (int64_t)n_labels * F, 0));
    const bool rows = n_labels > 0;
    Buffers b;
    list_csr(b, indptr, neighbor, border, n_labels, nnz).in(values, rows);
    if (b.out(mean_out, rows).out(min_out, rows).out(max_out, rows).out(used_out, rows).bad()) return refuse.buffers();
    if (n_labels == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(adj_stats_kernel, to_dim3(grids::flat((long long)n_labels * F)), dim3(256), 0, ctx->stream,
                           csr_of(indptr, neighbor, border, n_labels, nnz), values, F, mean_out, min_out, max_out, used_out);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_adj_class_border_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, const int64_t *border, int32_t n_labels,
                              int64_t nnz, const int32_t *classes, int K, int64_t *out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"adjacency", "class border"};
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.count("K", K, 1));
    OBIA_TRY(refuse.count("nnz", nnz, 0));
    OBIA_TRY(refuse.count("n_labels * K", (int64_t)n_labels * K, 0));
    Buffers b;
    if (list_csr(b, indptr, neighbor, border, n_labels, nnz).in(classes, n_labels > 0).out(out, n_labels > 0).bad()) return refuse.buffers();
    if (n_labels == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(adj_class_border_kernel, to_dim3(grids::flat(n_labels)), dim3(256), 0, ctx->stream,
                           csr_of(indptr, neighbor, border, n_labels, nnz), classes, K, reinterpret_cast<long long *>(out));
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_adj_best_neighbor_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, int32_t n_labels, int64_t nnz,
                               const double *d2, int32_t *best_out, double *best_d2_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"adjacency", "best neighbor"};
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.count("nnz", nnz, 0));
    Buffers b;
    if (list_csr(b, indptr, neighbor, n_labels, nnz).in(d2, nnz > 0).out(best_out, n_labels > 0).out(best_d2_out, n_labels > 0).bad())
        return refuse.buffers();
    if (n_labels == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(adj_best_kernel, to_dim3(grids::flat(n_labels)), dim3(256), 0, ctx->stream, csr_of(indptr, neighbor, nullptr, n_labels, nnz),
                           d2, best_out, best_d2_out);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

int obia_adj_components_dev(obia_ctx *ctx, const int64_t *indptr, const int32_t *neighbor, int32_t n_labels, int64_t nnz,
                            const uint8_t *link, int32_t *root_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"adjacency", "components"};
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.count("nnz", nnz, 0));
    Buffers b;
    if (list_csr(b, indptr, neighbor, n_labels, nnz).in(link, nnz > 0).out(root_out, n_labels > 0).bad()) return refuse.buffers();
    if (n_labels == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(adj_iota_kernel, to_dim3(grids::flat(n_labels)), dim3(256), 0, ctx->stream, root_out, n_labels);
        OBIA_HIP_TRY(hipGetLastError());
        if (nnz > 0) {
            hipLaunchKernelGGL(adj_link_kernel, to_dim3(grids::flat(nnz)), dim3(256), 0, ctx->stream, csr_of(indptr, neighbor, nullptr, n_labels, nnz),
                               link, root_out);
            OBIA_HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(adj_flatten_kernel, to_dim3(grids::flat(n_labels)), dim3(256), 0, ctx->stream, root_out, n_labels);
            OBIA_HIP_TRY(hipGetLastError());
        }
        return OBIA_OK;
    });
}

int obia_adj_relabel_dev(obia_ctx *ctx, const int32_t *labels, int64_t npx, int32_t start_label, int32_t n_labels, const int32_t *map,
                         int32_t *out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"adjacency", "relabel"};
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.count("npx", npx, 1));
    if (Buffers().out(out).in(labels).in(map, n_labels > 0).bad()) return refuse.buffers();
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        hipLaunchKernelGGL(adj_relabel_kernel, to_dim3(grids::flat(npx)), dim3(256), 0, ctx->stream, labels, (long long)npx, start_label, n_labels, map,
                           out);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

}  // extern "C"
