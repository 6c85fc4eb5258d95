// classify.hip -- the prediction half of obia/classification/classify.py on gfx950: everything that touches the full segment table.
//   table_scale   : StandardScaler().fit(x).transform(x) (classify.py:126-129) + the forest's cast to float32
//   forest_predict: the per-row loop of classify.py:135-158 (predict_proba / predict, class filter, margin) for all rows at once
// Training stays scikit-learn on the host.  Exactness contract: DESIGN.md 3.5g.
#include "common.hpp"
#include "wave_ops.hpp"

#include <cmath>

namespace obia {

// ------------------------------------------------------------------------------------------------------------------ scaler
// Column sums of a row-major (N, F) float64 table without floating-point atomics: a workgroup of 64 columns x 4 row lanes takes
// SC_ROWS rows, every thread adds its rows in ascending order, the four row lanes are added in lane order, and the finalize
// kernels add the per-workgroup partials in a fixed order.  The layout depends on (N, F) alone, so two runs agree bit for bit.
constexpr int SC_ROWS = 256;

// PASS 0: s1 = sum x, cnt = number of non-NaN values.  PASS 1: s1 = sum (x - mean), s2 = sum (x - mean)^2.
template <int PASS>
__global__ __launch_bounds__(256) void scale_partial_kernel(const double *__restrict__ x, long long N, int F, const double *__restrict__ mean,
                                                            double *__restrict__ p1, double *__restrict__ p2, long long *__restrict__ pcnt) {
    __shared__ double s_a[4][64], s_b[4][64];
    __shared__ long long s_n[4][64];
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + cx;
    const long long r0 = (long long)blockIdx.x * SC_ROWS;
    const long long r1 = r0 + SC_ROWS < N ? r0 + SC_ROWS : N;
    double a = 0.0, b = 0.0;
    long long n = 0;
    if (c < F) {
        const double m = PASS ? mean[c] : 0.0;
        for (long long r = r0 + ry; r < r1; r += 4) {
            const double v = x[r * F + c];
            if (v != v) continue;
            if (PASS) {
                const double d = v - m;
                a += d;
                b += d * d;
            } else {
                a += v;
                ++n;
            }
        }
    }
    s_a[ry][cx] = a;
    s_b[ry][cx] = b;
    s_n[ry][cx] = n;
    __syncthreads();
    if (ry == 0 && c < F) {
        const long long o = (long long)blockIdx.x * F + c;
        p1[o] = ((s_a[0][cx] + s_a[1][cx]) + s_a[2][cx]) + s_a[3][cx];
        if (PASS) p2[o] = ((s_b[0][cx] + s_b[1][cx]) + s_b[2][cx]) + s_b[3][cx];
        else pcnt[o] = s_n[0][cx] + s_n[1][cx] + s_n[2][cx] + s_n[3][cx];
    }
}

__device__ __forceinline__ double wave_sum_fixed(double v) {   // butterfly: the same tree of additions in every run
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// one wave per column: lane l adds partials l, l + 64, ... in ascending order, then the butterfly
__global__ __launch_bounds__(64) void scale_mean_kernel(const double *__restrict__ p1, const long long *__restrict__ pcnt, int B, int F,
                                                        double *__restrict__ mean, long long *__restrict__ cnt) {
    const int c = blockIdx.x, l = threadIdx.x;
    double s = 0.0;
    long long n = 0;
    for (int b = l; b < B; b += 64) {
        s += p1[(long long)b * F + c];
        n += pcnt[(long long)b * F + c];
    }
    s = wave_sum_fixed(s);
    n = wave_sum(n);
    if (l == 0) {
        mean[c] = s / (double)n;          // 0 / 0 = NaN for an all-NaN column, as np.nansum(x) / 0 gives
        cnt[c] = n;
    }
}

// scikit-learn's _incremental_mean_and_var from an empty state, then StandardScaler.partial_fit's constant-feature rule
// (_is_constant_feature + _handle_zeros_in_scale with that mask): var <= n eps var + (n mean eps)^2 -> scale 1.
__global__ __launch_bounds__(64) void scale_var_kernel(const double *__restrict__ p1, const double *__restrict__ p2, int B, int F,
                                                       const double *__restrict__ mean, const long long *__restrict__ cnt,
                                                       double *__restrict__ scale) {
    const int c = blockIdx.x, l = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int b = l; b < B; b += 64) {
        s1 += p1[(long long)b * F + c];
        s2 += p2[(long long)b * F + c];
    }
    s1 = wave_sum_fixed(s1);
    s2 = wave_sum_fixed(s2);
    if (l == 0) {
        const double n = (double)cnt[c], m = mean[c];
        const double var = (s2 - s1 * s1 / n) / n;
        const double eps = 2.220446049250313e-16;
        const double t = n * m * eps;
        const double upper = n * eps * var + t * t;
        scale[c] = (var <= upper) ? 1.0 : sqrt(var);      // NaN compares false: an all-NaN column keeps sqrt(NaN) = NaN
    }
}

// OUT = float: the table the forest wants; OUT = double: what MLPClassifier is handed (no cast)
template <typename OUT>
__global__ __launch_bounds__(256) void scale_transform_kernel(const double *__restrict__ x, long long total, int F, const double *__restrict__ mean,
                                                              const double *__restrict__ scale, OUT *__restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % F);
        out[i] = (OUT)((x[i] - mean[c]) / scale[c]);
    }
}

// ------------------------------------------------------------------------------------------------------------------ forest
// What a walk reads per node: one 16-byte record and one word.  fm = feature | missing_go_to_left << 16; a leaf has left = -1.
struct alignas(16) NodeRec {
    double threshold;
    int32_t left, right;       // GLOBAL node indices (tree offset added); a leaf keeps left = -1
};

constexpr int FP_ROWS = 64;      // rows per workgroup = one wave of lanes
constexpr int FP_CHUNK = 32;     // trees per chunk: their leaf indices wait in LDS for the ordered sum
constexpr int FP_MAXK = 64;
constexpr int FP_X_LDS_BYTES = 40 * 1024;   // the rows' features are staged in LDS when 64 rows of them fit in this

// Packs the caller's flat arrays into walk records and checks them: a feature outside [0, F) or a child outside its own tree turns
// the node into a leaf and raises the flag, so that a walk can never leave the arrays whatever the caller passed.
__global__ __launch_bounds__(256) void forest_pack_kernel(const double *__restrict__ thr, const int32_t *__restrict__ feat,
                                                          const int32_t *__restrict__ left, const int32_t *__restrict__ right,
                                                          const uint8_t *__restrict__ mgl, const int64_t *__restrict__ tree_off, int T,
                                                          long long total, int F, NodeRec *__restrict__ rec, int32_t *__restrict__ fm,
                                                          int *__restrict__ bad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int lo = 0, hi = T - 1;                       // the tree of node i: the last t with tree_off[t] <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tree_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const long long base = tree_off[lo], end = (lo + 1 < T) ? tree_off[lo + 1] : total;
    const long long nn = end - base;
    NodeRec r;
    r.threshold = thr[i];
    int l = left[i], rt = right[i], f = feat[i];
    int word = 0;
    if (l < 0) {                                   // leaf (scikit-learn: children -1, feature -2)
        r.left = -1;
        r.right = -1;
    } else if (l >= nn || rt < 0 || rt >= nn || f < 0 || f >= F) {
        r.left = -1;
        r.right = -1;
        *bad = 1;
    } else {
        r.left = (int32_t)(base + l);
        r.right = (int32_t)(base + rt);
        word = f | ((mgl && mgl[i]) ? 1 << 16 : 0);
    }
    rec[i] = r;
    fm[i] = word;
}

// One step of a walk; a leaf stays where it is (its word reads feature 0, which every row has).
template <bool XLDS>
__device__ __forceinline__ int forest_step(const NodeRec *__restrict__ rec, const int32_t *__restrict__ fm, int node, const float *sx,
                                           const float *__restrict__ xrow, bool &leaf) {
    const NodeRec r = rec[node];
    const int w = fm[node];
    const float v = XLDS ? sx[w & 0xffff] : xrow[w & 0xffff];
    const bool go_left = (v != v) ? ((w >> 16) != 0) : ((double)v <= r.threshold);
    leaf = r.left < 0;
    return leaf ? node : (go_left ? r.left : r.right);
}

// A workgroup takes 64 rows.  Phase 1, per chunk of 32 trees: lane = row, a wave walks two trees of the chunk at a time (two
// independent chains of dependent loads per lane) and leaves the leaf's node index in LDS.  Phase 2: four lanes per row, lane q
// owns classes q, q + 4, ...; it adds the leaf rows of the chunk in tree order into float64 registers.  After the last chunk:
// divide by T, store, then first maximum and margin over the acceptable classes through two shuffles among the row's four lanes.
template <bool XLDS>
__global__ __launch_bounds__(256) void forest_predict_kernel(const float *__restrict__ X, long long N, int F, int xstride,
                                                             const NodeRec *__restrict__ rec, const int32_t *__restrict__ fm,
                                                             const int64_t *__restrict__ tree_off, int T, int max_steps,
                                                             const double *__restrict__ values, int K, const uint8_t *__restrict__ mask,
                                                             double *__restrict__ proba, int32_t *__restrict__ pred,
                                                             double *__restrict__ margin, int *__restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int32_t *s_leaf = reinterpret_cast<int32_t *>(smem);                    // [FP_CHUNK][FP_ROWS]
    float *s_x = reinterpret_cast<float *>(smem + FP_CHUNK * FP_ROWS * 4);  // [FP_ROWS][xstride] when XLDS
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * FP_ROWS;
    const int nrows = (int)((N - row0) < FP_ROWS ? (N - row0) : FP_ROWS);
    if (XLDS) {
        const float *src = X + row0 * F;
        for (int i = tid; i < nrows * F; i += 256) {
            const int r = i / F;
            s_x[r * xstride + (i - r * F)] = src[i];
        }
        __syncthreads();
    }
    // a lane past the last row walks row 0 of the block (reads stay in bounds) and stores nothing
    const int wrow = lane < nrows ? lane : 0;
    const float *sx = s_x + wrow * xstride;
    const float *xrow = X + (row0 + wrow) * F;

    const int prow = tid >> 2, q = tid & 3;
    double acc[FP_MAXK / 4];
#pragma unroll
    for (int j = 0; j < FP_MAXK / 4; ++j) acc[j] = 0.0;
    const int nj = (K - q + 3) >> 2;               // classes q, q + 4, ... below K

    for (int t0 = 0; t0 < T; t0 += FP_CHUNK) {
        const int tc = (T - t0) < FP_CHUNK ? (T - t0) : FP_CHUNK;
        for (int tt = wave; tt < tc; tt += 8) {
            const bool two = tt + 4 < tc;
            int n0 = (int)tree_off[t0 + tt], n1 = two ? (int)tree_off[t0 + tt + 4] : n0;
            bool l0 = false, l1 = !two;
            for (int step = 0; step < max_steps && !(l0 && l1); ++step) {
                bool a, b;
                const int m0 = forest_step<XLDS>(rec, fm, n0, sx, xrow, a);
                const int m1 = forest_step<XLDS>(rec, fm, n1, sx, xrow, b);
                n0 = m0;
                n1 = m1;
                l0 = a;
                l1 = b || !two;
            }
            if (!(l0 && l1)) *bad = 2;             // no leaf within the tree's node count: the children form a cycle
            s_leaf[tt * FP_ROWS + lane] = n0;
            if (two) s_leaf[(tt + 4) * FP_ROWS + lane] = n1;
        }
        __syncthreads();
        if (prow < nrows) {
            for (int tt = 0; tt < tc; ++tt) {
                const double *leaf_row = values + (long long)s_leaf[tt * FP_ROWS + prow] * K + q;
#pragma unroll
                for (int j = 0; j < FP_MAXK / 4; ++j)
                    if (j < nj) acc[j] += leaf_row[4 * j];
            }
        }
        __syncthreads();
    }

    // every lane of a row's group of four takes part in the shuffles; rows past the end carry neutral values
    const bool live = prow < nrows;
    const long long row = row0 + prow;
    const double tdiv = (double)T;
    double best = -INFINITY, second = -INFINITY;
    int besti = -1;
#pragma unroll
    for (int j = 0; j < FP_MAXK / 4; ++j) {
        const int k = q + 4 * j;
        if (j < nj && live) {
            const double p = acc[j] / tdiv;
            if (proba) proba[row * K + k] = p;
            if (!mask || mask[row * K + k]) {
                if (besti < 0 || p > best) {       // strictly greater: the first maximum of this lane's ascending classes stays
                    second = besti < 0 ? second : best;
                    best = p;
                    besti = k;
                } else if (p > second) {
                    second = p;
                }
            }
        }
    }
#pragma unroll
    for (int off = 1; off <= 2; off <<= 1) {
        const double ob = __shfl_xor(best, off), os = __shfl_xor(second, off);
        const int oi = __shfl_xor(besti, off);
        if (oi >= 0) {
            if (besti < 0) {
                best = ob; second = os; besti = oi;
            } else {
                const bool other_wins = ob > best || (ob == best && oi < besti);
                const double loser = other_wins ? best : ob;
                const double s2 = os > second ? os : second;
                second = loser > s2 ? loser : s2;
                if (other_wins) { best = ob; besti = oi; }
            }
        }
    }
    if (live && q == 0) {
        if (pred) pred[row] = besti;
        if (margin) margin[row] = best - second;
    }
}

}  // namespace obia

using namespace obia;

template <typename OUT>
static int table_scale(obia_ctx *ctx, const double *table, int64_t n_rows, int n_features, double *mean_out, double *scale_out,
                       OUT *scaled_out) {
    OBIA_TRY(enter(ctx));
    if (!table || !mean_out || !scale_out || !scaled_out || n_features <= 0) { set_error("bad arguments"); return OBIA_E_INVALID; }
    if (n_rows <= 0) { set_error("the table has no rows"); return OBIA_E_INVALID; }
    const long long B64 = (n_rows + SC_ROWS - 1) / SC_ROWS;
    if (B64 >= (1ll << 31) || n_features > 65535 * 64) { set_error("table too large"); return OBIA_E_UNSUPPORTED; }
    const int B = (int)B64, F = n_features;
    ctx->arena.reset();
    double *p1 = ctx->arena.get<double>((size_t)B * F);
    double *p2 = ctx->arena.get<double>((size_t)B * F);
    long long *pcnt = ctx->arena.get<long long>((size_t)B * F);
    long long *cnt = ctx->arena.get<long long>(F);
    if (!p1 || !p2 || !pcnt || !cnt) return OBIA_E_NOMEM;
    const dim3 grid(B, cdiv(F, 64));
    hipLaunchKernelGGL(scale_partial_kernel<0>, grid, dim3(256), 0, ctx->stream, table, (long long)n_rows, F, (const double *)nullptr, p1,
                       p2, pcnt);
    hipLaunchKernelGGL(scale_mean_kernel, dim3(F), dim3(64), 0, ctx->stream, p1, pcnt, B, F, mean_out, cnt);
    hipLaunchKernelGGL(scale_partial_kernel<1>, grid, dim3(256), 0, ctx->stream, table, (long long)n_rows, F, mean_out, p1, p2, pcnt);
    hipLaunchKernelGGL(scale_var_kernel, dim3(F), dim3(64), 0, ctx->stream, p1, p2, B, F, mean_out, cnt, scale_out);
    const long long total = (long long)n_rows * F;
    hipLaunchKernelGGL(scale_transform_kernel<OUT>, to_dim3(grids::scale_transform(n_rows, F)), dim3(256), 0, ctx->stream, table, total, F, mean_out, scale_out, scaled_out);
    OBIA_HIP_TRY(hipGetLastError());
    OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return OBIA_OK;
}

extern "C" {

int obia_table_scale_dev(obia_ctx *ctx, const double *table, int64_t n_rows, int n_features, double *mean_out, double *scale_out,
                         float *scaled_out) {
    return table_scale<float>(ctx, table, n_rows, n_features, mean_out, scale_out, scaled_out);
}

int obia_table_scale_f64_dev(obia_ctx *ctx, const double *table, int64_t n_rows, int n_features, double *mean_out, double *scale_out,
                             double *scaled_out) {
    return table_scale<double>(ctx, table, n_rows, n_features, mean_out, scale_out, scaled_out);
}

int obia_forest_predict_dev(obia_ctx *ctx, const float *x, int64_t n_rows, int n_features, const obia_forest *forest,
                            const uint8_t *acceptable, double *proba_out, int32_t *pred_out, double *margin_out) {
    OBIA_TRY(enter(ctx));
    if (!x || !forest || n_features <= 0 || n_rows < 0) { set_error("bad arguments"); return OBIA_E_INVALID; }
    const obia_forest &f = *forest;
    if (!f.threshold || !f.feature || !f.left || !f.right || !f.tree_offset || !f.tree_offset_host || !f.value || f.n_trees <= 0 ||
        f.n_classes <= 0 || f.n_nodes <= 0) {
        set_error("bad forest");
        return OBIA_E_INVALID;
    }
    if (f.n_classes > FP_MAXK || n_features > 4096 || f.n_trees > 65536 || f.n_nodes >= (1ll << 31) || n_rows >= (1ll << 31) * FP_ROWS) {
        set_error("forest_predict supports at most %d classes, 4096 features, 65536 trees and 2^31 - 1 nodes (got %d, %d, %d, %lld)",
                  FP_MAXK, f.n_classes, n_features, f.n_trees, (long long)f.n_nodes);
        return OBIA_E_UNSUPPORTED;
    }
    // the tree offsets decide where a walk starts: checked on the host copy before anything is launched
    long long max_nodes = 0;
    for (int t = 0; t < f.n_trees; ++t) {
        const long long lo = f.tree_offset_host[t], hi = (t + 1 < f.n_trees) ? f.tree_offset_host[t + 1] : f.n_nodes;
        if ((t == 0 && lo != 0) || hi <= lo || hi > f.n_nodes) { set_error("tree offsets must start at 0 and increase"); return OBIA_E_INVALID; }
        if (hi - lo > max_nodes) max_nodes = hi - lo;
    }
    if (n_rows == 0) return OBIA_OK;
    ctx->arena.reset();
    NodeRec *rec = ctx->arena.get<NodeRec>((size_t)f.n_nodes);
    int32_t *fm = ctx->arena.get<int32_t>((size_t)f.n_nodes);
    int *bad = ctx->arena.get<int>(1);
    if (!rec || !fm || !bad) return OBIA_E_NOMEM;
    OBIA_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(forest_pack_kernel, dim3(cdiv(f.n_nodes, 256)), dim3(256), 0, ctx->stream, f.threshold, f.feature, f.left, f.right,
                       f.missing_go_to_left, f.tree_offset, f.n_trees, (long long)f.n_nodes, n_features, rec, fm, bad);
    const int xstride = n_features | 1;            // odd: the 64 rows of a wave fall on different LDS banks for one feature
    const bool xlds = (size_t)FP_ROWS * xstride * 4 <= (size_t)FP_X_LDS_BYTES;
    const size_t lds = (size_t)FP_CHUNK * FP_ROWS * 4 + (xlds ? (size_t)FP_ROWS * xstride * 4 : 0);
    const dim3 grid((unsigned)((n_rows + FP_ROWS - 1) / FP_ROWS));
    const int max_steps = (int)max_nodes;          // a walk visits no node twice, so it ends within the tree's node count
    if (xlds)
        hipLaunchKernelGGL(forest_predict_kernel<true>, grid, dim3(256), lds, ctx->stream, x, (long long)n_rows, n_features, xstride, rec, fm,
                           f.tree_offset, f.n_trees, max_steps, f.value, f.n_classes, acceptable, proba_out, pred_out, margin_out, bad);
    else
        hipLaunchKernelGGL(forest_predict_kernel<false>, grid, dim3(256), lds, ctx->stream, x, (long long)n_rows, n_features, xstride, rec, fm,
                           f.tree_offset, f.n_trees, max_steps, f.value, f.n_classes, acceptable, proba_out, pred_out, margin_out, bad);
    OBIA_HIP_TRY(hipGetLastError());
    int h_bad = 0;
    OBIA_TRY(read_back(ctx, &h_bad, bad, sizeof(int)));
    if (h_bad) {
        set_error(h_bad == 1 ? "forest: a node's feature or child index is out of range" : "forest: a tree's children form a cycle");
        return OBIA_E_INVALID;
    }
    return OBIA_OK;
}

}  // extern "C"
