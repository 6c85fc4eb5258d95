// shap.hip -- SHAP values of a fitted tree ensemble on gfx950: path-dependent TreeSHAP (what shap.TreeExplainer(forest) computes
// without background data, classify.py:113-118 of the reference) in its per-path form, for every row of the segment table.
// Contract, operation order and the mapping: DESIGN.md 3.5k; the same arithmetic in NumPy / Fractions: tests/shap_restatement.py.
//
// A root-to-leaf path contributes to a row through one bit per DISTINCT feature on it ("the row follows the path at every split
// of this feature"), so the splits of one feature are merged into one element (zero fraction = the product of the splits'
// cover[child] / cover[node]; for a value that is not NaN the bit is an interval test, for a NaN one stored bit).
//   preparation : parent links + node checks, elements per leaf counted, two prefix sums, element and path records written
//   shap_base   : base[k] = sum over paths (zero fractions of the path multiplied) value[leaf][k] / T, one thread per class
//   shap_main   : lanes = path elements, a wave packs floor(64 / (m + 1)) rows of the SAME path side by side
// Everything is float64, there is no floating-point atomic, and the order of all additions is fixed by the forest alone.
#include "common.hpp"
#include "wave_ops.hpp"

#include <cmath>

namespace obia {

constexpr int SH_MAXM = 32;          // distinct features on one path (the unwinding amplifies rounding beyond that: DESIGN 3.5k)
constexpr int SH_MAXK = 64;
constexpr int SH_INV = SH_MAXM + 2;
constexpr int SH_WAVES = 4;          // waves per workgroup; every wave owns its own rows of the workgroup's block
constexpr int SH_MAX_ROWS = 64;      // rows per workgroup at most
constexpr int SH_MIN_LDS_ROWS = 4;   // the accumulators live in LDS when at least this many rows of them fit in 64 KB
constexpr int SH_GLOBAL_ROWS = 32;   // rows per workgroup when they live in the output itself
constexpr int SH_LDS_BYTES = 64 * 1024;

struct alignas(16) ShapElem {        // one distinct feature of one path
    double lo, hi;                   // a value v that is not NaN follows iff !(v <= lo) && v <= hi   (lo = NaN: no right turn)
    double zero;                     // product of cover[child] / cover[node] over the feature's splits, leaf upwards
    int32_t feature;
    int32_t nan_follows;             // a NaN follows: missing_go_to_left equals the turn taken at every split of the feature
};

struct alignas(8) ShapPath {
    long long off;                   // first element record
    int32_t leaf;                    // global node index: the row of `value`
    int32_t len;                     // number of elements m
    double zprod;                    // zero fractions of the elements multiplied in element order (1 for a tree that is one leaf)
};

// The integer ratios of EXTEND and UNWIND: rat(a, b) = (double)a * inv[b], inv[b] = 1.0 / (double)b (two roundings, no division
// in the recurrences).  Every denominator is the same for all lanes of a wave, so inv[] is read with wave-uniform loads.
struct ShapInv { double v[SH_INV]; };
constexpr ShapInv make_inv() {
    ShapInv t{};
    for (int b = 1; b < SH_INV; ++b) t.v[b] = 1.0 / (double)b;
    return t;
}
__device__ const ShapInv SHAP_INV = make_inv();

enum { SH_BAD_NODE = 1, SH_BAD_CYCLE = 2, SH_BAD_COVER = 3, SH_BAD_LONG = 4 };

__device__ __forceinline__ int tree_of(const int64_t *__restrict__ tree_off, int T, long long i) {
    int lo = 0, hi = T - 1;                       // the last t with tree_off[t] <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tree_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Per node: the checks of forest_pack_kernel, the cover check, and the parent link of its two children (global indices).  A node
// that two nodes name as their child, a node that names one child twice or a child that is its tree's root raise the flag: after
// this kernel every node has at most one parent, so a walk upwards can only end or go round a cycle (which the step bound ends).
__global__ __launch_bounds__(256) void shap_parent_kernel(const int32_t *__restrict__ feat, const int32_t *__restrict__ left,
                                                          const int32_t *__restrict__ right, const double *__restrict__ cover,
                                                          const int64_t *__restrict__ tree_off, int T, long long total, int F,
                                                          int32_t *__restrict__ parent, int *__restrict__ bad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const double c = cover[i];
    if (!(c > 0.0) || c == INFINITY) atomicMax(bad, SH_BAD_COVER);
    const int l = left[i];
    if (l < 0) return;
    const int t = tree_of(tree_off, T, i);
    const long long base = tree_off[t], end = (t + 1 < T) ? tree_off[t + 1] : total;
    const long long nn = end - base;
    const int r = right[i], f = feat[i];
    if (l >= nn || r < 0 || r >= nn || f < 0 || f >= F || l == r || l == 0 || r == 0) {
        atomicMax(bad, SH_BAD_NODE);
        return;
    }
    if (atomicCAS(&parent[base + l], -1, (int32_t)i) != -1) atomicMax(bad, SH_BAD_NODE);
    if (atomicCAS(&parent[base + r], -1, (int32_t)i) != -1) atomicMax(bad, SH_BAD_NODE);
}

// One thread per leaf walks to its root.  FILL = false: counts the distinct features (nelem[i], 0 for an inner node) and marks the
// leaf (isleaf[i]).  FILL = true: writes the path record and the element records at the offsets the prefix sums gave.  The walk is
// bounded by the tree's node count; it is only started when shap_parent_kernel raised no flag (FILL) or touches nothing but
// checked indices (a child link is followed only through `parent`, which holds checked indices alone).
template <bool FILL>
__global__ __launch_bounds__(64) void shap_path_kernel(const double *__restrict__ thr, const int32_t *__restrict__ feat,
                                                       const int32_t *__restrict__ left, const uint8_t *__restrict__ mgl,
                                                       const double *__restrict__ cover, const int64_t *__restrict__ tree_off, int T,
                                                       long long total, int F, const int32_t *__restrict__ parent,
                                                       int32_t *__restrict__ nelem, int32_t *__restrict__ isleaf,
                                                       const long long *__restrict__ path_idx, const long long *__restrict__ elem_off,
                                                       ShapPath *__restrict__ paths, ShapElem *__restrict__ elems, int *__restrict__ bad) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= total) return;
    if (left[i] >= 0) {
        if (!FILL) { nelem[i] = 0; isleaf[i] = 0; }
        return;
    }
    const int t = tree_of(tree_off, T, i);
    const long long base = tree_off[t], end = (t + 1 < T) ? tree_off[t + 1] : total;
    const long long nn = end - base;
    int32_t seen[SH_MAXM];
    int m = 0;
    ShapElem *mine = FILL ? elems + elem_off[i] : nullptr;
    const int want = FILL ? nelem[i] : 0;
    long long node = i;
    long long steps = 0;
    bool ok = true;
    while (node != base) {
        const int32_t p = parent[node];
        if (p < 0 || ++steps > nn) {               // an unreachable node, or a cycle
            atomicMax(bad, p < 0 ? SH_BAD_NODE : SH_BAD_CYCLE);
            ok = false;
            break;
        }
        const int f = feat[p];
        if (f < 0 || f >= F) { atomicMax(bad, SH_BAD_NODE); ok = false; break; }
        int e = 0;
        while (e < m && seen[e] != f) ++e;
        if (e == m) {
            if (m == SH_MAXM) { atomicMax(bad, SH_BAD_LONG); ok = false; break; }
            seen[m++] = f;
            if (FILL && e < want) {
                ShapElem n;
                n.lo = NAN;
                n.hi = INFINITY;
                n.zero = 1.0;
                n.feature = f;
                n.nan_follows = 1;
                mine[e] = n;
            }
        }
        if (FILL && e < want) {
            const bool is_left = base + left[p] == node;
            const double th = thr[p];
            ShapElem n = mine[e];
            if (is_left) {
                if (n.hi == n.hi && (th != th || th < n.hi)) n.hi = th;      // a NaN threshold is never followed to the left
            } else if (th == th && !(th <= n.lo)) {
                n.lo = th;
            }
            n.zero = n.zero * (cover[node] / cover[p]);
            if (((mgl && mgl[p]) != 0) != is_left) n.nan_follows = 0;
            mine[e] = n;
        }
        node = p;
    }
    if (!FILL) {
        nelem[i] = ok ? m : 0;
        isleaf[i] = 1;
        return;
    }
    ShapPath P;
    P.off = elem_off[i];
    P.leaf = (int32_t)i;
    P.len = want;
    double z = 1.0;
    for (int e = 0; e < want; ++e) z = z * mine[e].zero;
    P.zprod = z;
    paths[path_idx[i]] = P;
}

// Exclusive prefix sum of n int32 counts into int64 (one workgroup: thread t owns a contiguous chunk) and their total.
__global__ __launch_bounds__(256) void shap_scan_kernel(const int32_t *__restrict__ in, long long n, long long *__restrict__ out,
                                                        long long *__restrict__ total_out) {
    workgroup_exclusive_scan<256>(in, out, n, total_out);
}

// base[k]: thread k adds the paths in their order (trees ascending, leaves in ascending node index).
__global__ __launch_bounds__(64) void shap_base_kernel(const ShapPath *__restrict__ paths, long long n_paths,
                                                       const double *__restrict__ value, int K, int T, double *__restrict__ base_out) {
    const int k = threadIdx.x;
    if (k >= K) return;
    const double tn = (double)T;
    double acc = 0.0;
    for (long long p = 0; p < n_paths; ++p) acc = acc + (paths[p].zprod * value[(long long)paths[p].leaf * K + k]) / tn;
    base_out[k] = acc;
}

// A workgroup takes R rows and walks ALL paths in their order; wave w owns rows [w per, (w + 1) per) of the block.  For a path of
// m elements a wave lays floor(64 / (m + 1)) of its rows side by side: lane e of a row's segment holds weight w[e] of the EXTEND
// recurrence (e = 0 is the empty set's slot, e = 1 .. m the elements).  EXTEND is m steps, each one shuffle from the lane below
// and two broadcasts (the new element's zero fraction and the row's bit for it); then every lane unwinds its own element in m
// steps of broadcast reads and adds its contribution to phi[row][its feature][:].  Within a path every lane of a segment owns a
// different feature and every segment a different row, and one wave handles a row's paths in program order: the accumulators
// see plain read-modify-writes, in LDS (LDS = true, copied out at the end) or in the output itself.
template <bool LDS>
__global__ __launch_bounds__(256) void shap_main_kernel(const float *__restrict__ X, long long N, int F, int K, int R,
                                                        const ShapPath *__restrict__ paths, long long n_paths,
                                                        const ShapElem *__restrict__ elems, const double *__restrict__ value, int T,
                                                        double *__restrict__ phi) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * R;
    const int nrows = (int)((N - row0) < R ? (N - row0) : R);
    const int FK = F * K;
    double *acc = LDS ? reinterpret_cast<double *>(smem) : phi + row0 * FK;
    float *s_x = reinterpret_cast<float *>(smem + (size_t)R * FK * sizeof(double));
    const float *xs = LDS ? s_x : X + row0 * F;
    for (int i = tid; i < nrows * FK; i += 256) acc[i] = 0.0;
    if (LDS)
        for (int i = tid; i < nrows * F; i += 256) s_x[i] = X[row0 * F + i];
    __syncthreads();

    const int per = (nrows + SH_WAVES - 1) / SH_WAVES;
    const int wr0 = wave * per, wr1 = (wr0 + per) < nrows ? (wr0 + per) : nrows;
    const double tn = (double)T;
    const double *inv = SHAP_INV.v;
    for (long long p = 0; p < n_paths; ++p) {
        const ShapPath P = paths[p];
        const int m = P.len;
        if (m <= 0 || m > SH_MAXM) continue;       // a tree that is one leaf explains nothing
        const int L = m + 1, g = 64 / L;
        const int seg = lane / L, e = lane - seg * L, segbase = seg * L;
        const bool in_seg = seg < g;
        ShapElem el;
        el.lo = NAN; el.hi = INFINITY; el.zero = 1.0; el.feature = 0; el.nan_follows = 1;
        if (in_seg && e > 0) el = elems[P.off + e - 1];
        const double *leaf_row = value + (long long)P.leaf * K;
        for (int rb = wr0; rb < wr1; rb += g) {
            const int r = rb + seg;
            const bool live = in_seg && r < wr1;
            const int rr = live ? r : wr0;         // lanes without a row compute on the wave's first row and store nothing
            const float v = xs[rr * F + el.feature];
            const double vd = (double)v;
            const bool fol = (v != v) ? (el.nan_follows != 0) : (!(vd <= el.lo) && vd <= el.hi);
            const double one = (e == 0 || fol) ? 1.0 : 0.0;
            double w = e == 0 ? 1.0 : 0.0;
            for (int s = 1; s <= m; ++s) {
                const double pz = __shfl(el.zero, segbase + s), po = __shfl(one, segbase + s);
                const double below = __shfl_up(w, 1);
                const double is = inv[s + 1];
                if (e <= s) {
                    const double a = (pz * w) * ((double)(s - e) * is);
                    const double b = e > 0 ? (po * below) * ((double)e * is) : 0.0;
                    w = a + b;
                }
            }
            double nop = __shfl(w, segbase + m), tot = 0.0;
            const double m1 = (double)(m + 1), im1 = inv[m + 1];
            for (int j = m - 1; j >= 0; --j) {
                const double wj = __shfl(w, segbase + j);
                if (one != 0.0) {
                    const double t = nop * (m1 * inv[j + 1]);
                    tot = tot + t;
                    nop = wj - (t * el.zero) * ((double)(m - j) * im1);
                } else {
                    tot = tot + wj * (m1 * inv[m - j]);
                }
            }
            if (one == 0.0) tot = tot / el.zero;
            const double scale = (tot * (one - el.zero)) / tn;
            if (live && e > 0) {
                double *a = acc + ((long long)rr * F + el.feature) * K;
                for (int k = 0; k < K; ++k) a[k] = a[k] + scale * leaf_row[k];
            }
            __threadfence_block();                 // the next path's owner of this accumulator is another lane of this wave
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = tid; i < nrows * FK; i += 256) phi[row0 * FK + i] = acc[i];
    }
}

}  // namespace obia

using namespace obia;

extern "C" {

int obia_forest_shap_dev(obia_ctx *ctx, const float *x, int64_t n_rows, int n_features, const obia_forest *forest, const double *cover,
                         double *phi_out, double *base_out) {
    OBIA_TRY(enter(ctx));
    if (!x || !forest || !cover || !phi_out || !base_out || n_features <= 0 || n_rows < 0) { set_error("bad arguments"); return OBIA_E_INVALID; }
    const obia_forest &f = *forest;
    if (!f.threshold || !f.feature || !f.left || !f.right || !f.tree_offset || !f.tree_offset_host || !f.value || f.n_trees <= 0 ||
        f.n_classes <= 0 || f.n_nodes <= 0) {
        set_error("bad forest");
        return OBIA_E_INVALID;
    }
    if (f.n_classes > SH_MAXK || n_features > 4096 || f.n_trees > 65536 || f.n_nodes >= (1ll << 31) || n_rows >= (1ll << 31) * SH_MIN_LDS_ROWS) {
        set_error("forest_shap supports at most %d classes, 4096 features, 65536 trees and 2^31 - 1 nodes (got %d, %d, %d, %lld)",
                  SH_MAXK, f.n_classes, n_features, f.n_trees, (long long)f.n_nodes);
        return OBIA_E_UNSUPPORTED;
    }
    for (int t = 0; t < f.n_trees; ++t) {
        const long long lo = f.tree_offset_host[t], hi = (t + 1 < f.n_trees) ? f.tree_offset_host[t + 1] : f.n_nodes;
        if ((t == 0 && lo != 0) || hi <= lo || hi > f.n_nodes) { set_error("tree offsets must start at 0 and increase"); return OBIA_E_INVALID; }
    }
    const long long n = f.n_nodes;
    const int F = n_features, K = f.n_classes, T = f.n_trees;
    ctx->arena.reset();
    int32_t *parent = ctx->arena.get<int32_t>((size_t)n);
    int32_t *nelem = ctx->arena.get<int32_t>((size_t)n);
    int32_t *isleaf = ctx->arena.get<int32_t>((size_t)n);
    long long *path_idx = ctx->arena.get<long long>((size_t)n);
    long long *elem_off = ctx->arena.get<long long>((size_t)n);
    long long *totals = ctx->arena.get<long long>(2);
    int *bad = ctx->arena.get<int>(1);
    if (!parent || !nelem || !isleaf || !path_idx || !elem_off || !totals || !bad) return OBIA_E_NOMEM;
    OBIA_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    OBIA_HIP_TRY(hipMemsetAsync(parent, 0xff, (size_t)n * sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(shap_parent_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, f.feature, f.left, f.right, cover, f.tree_offset,
                       T, n, F, parent, bad);
    hipLaunchKernelGGL(shap_path_kernel<false>, dim3(cdiv(n, 64)), dim3(64), 0, ctx->stream, f.threshold, f.feature, f.left,
                       f.missing_go_to_left, cover, f.tree_offset, T, n, F, parent, nelem, isleaf, (const long long *)nullptr,
                       (const long long *)nullptr, (ShapPath *)nullptr, (ShapElem *)nullptr, bad);
    hipLaunchKernelGGL(shap_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, isleaf, n, path_idx, totals);
    hipLaunchKernelGGL(shap_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, nelem, n, elem_off, totals + 1);
    OBIA_HIP_TRY(hipGetLastError());
    int h_bad = 0;
    OBIA_TRY(read_back(ctx, &h_bad, bad, sizeof(int)));
    if (h_bad == SH_BAD_LONG) {
        set_error("forest_shap: a root-to-leaf path tests more than %d distinct features", SH_MAXM);
        return OBIA_E_UNSUPPORTED;
    }
    if (h_bad) {
        set_error(h_bad == SH_BAD_COVER ? "forest_shap: a node's cover is not finite and positive"
                  : h_bad == SH_BAD_CYCLE ? "forest: a tree's children form a cycle"
                                          : "forest: a node's feature or child index is out of range, or a node is not reached from its root exactly once");
        return OBIA_E_INVALID;
    }
    long long h_tot[2] = {0, 0};
    OBIA_TRY(read_back(ctx, h_tot, totals, sizeof(h_tot)));
    const long long n_paths = h_tot[0], n_elems = h_tot[1];
    if (n_paths <= 0 || n_paths > n || n_elems < 0 || n_elems > n_paths * SH_MAXM) { set_error("forest_shap: inconsistent path count"); return OBIA_E_INVALID; }
    ShapPath *paths = ctx->arena.get<ShapPath>((size_t)n_paths);
    ShapElem *elems = ctx->arena.get<ShapElem>((size_t)n_elems + 1);
    if (!paths || !elems) return OBIA_E_NOMEM;
    hipLaunchKernelGGL(shap_path_kernel<true>, dim3(cdiv(n, 64)), dim3(64), 0, ctx->stream, f.threshold, f.feature, f.left,
                       f.missing_go_to_left, cover, f.tree_offset, T, n, F, parent, nelem, isleaf, (const long long *)path_idx,
                       (const long long *)elem_off, paths, elems, bad);
    hipLaunchKernelGGL(shap_base_kernel, dim3(1), dim3(64), 0, ctx->stream, paths, n_paths, f.value, K, T, base_out);
    if (n_rows > 0) {
        const size_t per_row = (size_t)F * K * sizeof(double) + (size_t)F * sizeof(float);
        const int fit = (int)(SH_LDS_BYTES / per_row);
        if (fit >= SH_MIN_LDS_ROWS) {
            const int R = fit < SH_MAX_ROWS ? fit : SH_MAX_ROWS;
            hipLaunchKernelGGL(shap_main_kernel<true>, dim3((unsigned)((n_rows + R - 1) / R)), dim3(256), (size_t)R * per_row, ctx->stream, x,
                               (long long)n_rows, F, K, R, paths, n_paths, elems, f.value, T, phi_out);
        } else {
            const int R = SH_GLOBAL_ROWS;
            hipLaunchKernelGGL(shap_main_kernel<false>, dim3((unsigned)((n_rows + R - 1) / R)), dim3(256), 0, ctx->stream, x, (long long)n_rows,
                               F, K, R, paths, n_paths, elems, f.value, T, phi_out);
        }
    }
    OBIA_HIP_TRY(hipGetLastError());
    OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return OBIA_OK;
}

}  // extern "C"
