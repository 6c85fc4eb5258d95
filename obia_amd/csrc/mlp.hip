// mlp.hip -- MLPClassifier's forward pass (scikit-learn's _forward_pass_fast) for the whole segment table at once, fused through to
// class, margin and class filter.  The arithmetic is an order of our own that tests/mlp_restatement.py reproduces bit for bit
// (DESIGN.md 3.5j): float64 throughout, every product and every sum rounded on its own (the build has -ffp-contract=off; no fma, no
// MFMA), a unit's inputs added in ascending order starting from 0.0, the bias last.
#include "mlp.hpp"

namespace obia {

// A 256-thread workgroup takes R rows (64 where the layers are narrow enough, down to 4 at width 512) through the layers
// (mlp_layers in mlp.hpp: the mapping and the LDS layout).  The input layer comes from x, read coalesced.
// After the last layer one thread per row turns the logits into proba, class and margin (forest_predict_kernel's rule).
__global__ __launch_bounds__(256) void mlp_predict_kernel(const double *__restrict__ X, long long N, const double *__restrict__ Wt,
                                                          const double *__restrict__ Bs, const MlpPlan p, const uint8_t *__restrict__ mask,
                                                          double *__restrict__ proba, int32_t *__restrict__ pred, double *__restrict__ margin,
                                                          double *__restrict__ logits, int *__restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int R = 1 << p.rshift;
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * R;
    const int nrows = (int)((N - row0) < R ? (N - row0) : R);
    const int F = p.sizes[0];
    const double *src = mlp_layers(p, Wt, Bs, smem, [&](int rr, int f) {
        double v = 0.0;                                     // rows past the end of the table compute on zeros and store nothing
        if (rr < nrows) {
            v = X[(row0 + rr) * F + f];
            if (!(fabs(v) <= DBL_MAX)) *bad = 1;
        }
        return v;
    });

    if (tid >= nrows) return;                               // tid < R here: thread = row
    const long long row = row0 + tid;
    const int K = p.n_classes, n_out = p.sizes[p.n_layers];
    const double *z = src + tid;                            // z[k * R]
    if (logits)
        for (int k = 0; k < n_out; ++k) logits[row * n_out + k] = z[k * R];
    double best = -INFINITY, second = -INFINITY, s = 0.0, m = z[0], p1 = 0.0;
    int besti = -1;
    if (p.out_act == 0) {
        for (int k = 1; k < K; ++k) m = z[k * R] > m ? z[k * R] : m;
        for (int k = 0; k < K; ++k) s = s + exp(z[k * R] - m);
    } else {
        p1 = 1.0 / (1.0 + exp(-z[0]));
    }
    for (int k = 0; k < K; ++k) {
        const double pk = p.out_act == 0 ? exp(z[k * R] - m) / s : (k == 0 ? 1.0 - p1 : p1);
        if (proba) proba[row * K + k] = pk;
        if (!mask || mask[row * K + k]) {
            if (besti < 0 || pk > best) {                   // strictly greater: the first maximum stays
                second = besti < 0 ? second : best;
                best = pk;
                besti = k;
            } else if (pk > second) {
                second = pk;
            }
        }
    }
    if (pred) pred[row] = besti;
    if (margin) margin[row] = best - second;
}

}  // namespace obia

using namespace obia;

extern "C" {

int obia_mlp_predict_dev(obia_ctx *ctx, const double *x, int64_t n_rows, int n_features, const obia_mlp *mlp, const uint8_t *acceptable,
                         double *proba_out, int32_t *pred_out, double *margin_out, double *logits_out) {
    OBIA_TRY(enter(ctx));
    if (!x || !mlp || n_features <= 0 || n_rows < 0) { set_error("bad arguments"); return OBIA_E_INVALID; }
    MlpPlan p;
    OBIA_TRY(mlp_make_plan(mlp, n_features, "mlp_predict", p));
    const obia_mlp &m = *mlp;
    const int R = 1 << p.rshift;
    const long long blocks = (n_rows + R - 1) / R;
    if (blocks >= (1ll << 31)) { set_error("table too large"); return OBIA_E_UNSUPPORTED; }
    if (n_rows == 0) return OBIA_OK;
    ctx->arena.reset();
    int *bad = ctx->arena.get<int>(1);
    if (!bad) return OBIA_E_NOMEM;
    OBIA_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(mlp_predict_kernel, dim3((unsigned)blocks), dim3(256), mlp_lds_bytes(p), ctx->stream, x, (long long)n_rows, m.weights, m.biases, p,
                       acceptable, proba_out, pred_out, margin_out, logits_out, bad);
    OBIA_HIP_TRY(hipGetLastError());
    int h_bad = 0;
    OBIA_TRY(read_back(ctx, &h_bad, bad, sizeof(int)));
    if (h_bad) { set_error("Input X contains NaN or infinity"); return OBIA_E_INVALID; }
    return OBIA_OK;
}

}  // extern "C"
