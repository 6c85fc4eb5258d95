// mlp_shap.hip -- exact interventional Shapley values of a fitted MLP against a background table (what shap.KernelExplainer
// computes when its budget lets it enumerate every coalition; classify.py:108-115 of the reference).  Contract: DESIGN.md 3.5l.
//   mlp_coalition_kernel   : v(row, coalition) = the mean over the background rows of proba(hybrid row), the hot kernel
//   shapley_combine_kernel : phi[row, f, :] from the 2^F coalition values of a row by the subset formula
// The forward pass is mlp_layers of mlp.hpp -- the loop mlp_predict_kernel runs -- and the softmax is the same expressions, so a
// hybrid row gets the bits mlp_predict gives it.  Float64 throughout, no fma, no MFMA, no floating-point atomics.
#include "mlp.hpp"

namespace obia {

constexpr int SHAPLEY_MAX_FEATURES = 16;     // 2^F coalitions are enumerated

struct ShapleyWeights { double w[SHAPLEY_MAX_FEATURES]; };

// flag[which] = 1 if a[0 .. n) holds a NaN or an infinity.
__global__ __launch_bounds__(256) void mlp_finite_kernel(const double *__restrict__ a, long long n, int *__restrict__ flag, int which) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && !(fabs(a[i]) <= DBL_MAX)) flag[which] = 1;
}

// One workgroup owns one (row n, coalition m) pair and walks the background in pieces of R rows (R = mlp_predict_kernel's rows per
// workgroup for these layer sizes, the same 64 KB LDS plan).  Per piece: the R hybrid rows -- x[n, f] where the coalition holds f,
// background[b, f] elsewhere -- are built while the input layer is staged; mlp_layers leaves the logits in LDS, [k][R]; all
// (row, class) pairs take their exp side by side and divide by the row's sum (the sum in ascending k, as mlp_predict_kernel adds
// it); then thread k adds the piece's probabilities of class k to its running sum in ascending b.  The sum of a (row, coalition,
// class) lives in one register from 0.0 to the division by B: the order is b = 0, 1, ..., B - 1 whatever R is.
// masks: (M, F) bytes, non-zero = the feature comes from x; NULL = coalition m holds feature f iff bit f of m is set.
__global__ __launch_bounds__(256) void mlp_coalition_kernel(const double *__restrict__ X, int M, const double *__restrict__ Wt,
                                                            const double *__restrict__ Bs, const MlpPlan p,
                                                            const double *__restrict__ bg, int nB, const uint8_t *__restrict__ masks,
                                                            double *__restrict__ values) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int R = 1 << p.rshift;
    const int tid = threadIdx.x;
    const int F = p.sizes[0], K = p.n_classes;
    const long long pair = blockIdx.x;
    const long long n = pair / M;
    const int m = (int)(pair - n * M);
    const double *x = X + n * F;
    const uint8_t *mk = masks ? masks + (long long)m * F : nullptr;
    double *buf0 = reinterpret_cast<double *>(smem), *buf1 = buf0 + p.wmax * R;
    double *z = ((p.n_layers - 1) & 1) ? buf1 : buf0;      // where mlp_layers leaves the logits
    double *e = ((p.n_layers - 1) & 1) ? buf0 : buf1;      // the other buffer: wmax >= n_out rows of R doubles

    double acc = 0.0;                                       // thread k < K: the running sum of class k
    for (int b0 = 0; b0 < nB; b0 += R) {
        const int nrows = (nB - b0) < R ? (nB - b0) : R;
        mlp_layers(p, Wt, Bs, smem, [&](int rr, int f) {
            if (rr >= nrows) return 0.0;                    // rows past the end of the background compute on zeros and are not added
            const bool from_x = mk ? mk[f] != 0 : ((m >> f) & 1) != 0;
            return from_x ? x[f] : bg[(long long)(b0 + rr) * F + f];
        });
        if (p.out_act == 0) {
            for (int i = tid; i < K * R; i += 256) {
                const int r = i & (R - 1), k = i >> p.rshift;
                double mx = z[r];
                for (int kk = 1; kk < K; ++kk) mx = z[kk * R + r] > mx ? z[kk * R + r] : mx;
                e[k * R + r] = exp(z[k * R + r] - mx);
            }
            __syncthreads();
            for (int i = tid; i < K * R; i += 256) {
                const int r = i & (R - 1), k = i >> p.rshift;
                double s = 0.0;
                for (int kk = 0; kk < K; ++kk) s = s + e[kk * R + r];
                z[k * R + r] = e[k * R + r] / s;            // the logits have all been read before the barrier above
            }
            __syncthreads();
            if (tid < K)
                for (int r = 0; r < nrows; ++r) acc = acc + z[tid * R + r];
        } else {
            if (tid < R) z[tid] = 1.0 / (1.0 + exp(-z[tid]));
            __syncthreads();
            if (tid < 2)
                for (int r = 0; r < nrows; ++r) acc = acc + (tid == 0 ? 1.0 - z[r] : z[r]);
        }
        __syncthreads();                                    // the next piece overwrites what was just added
    }
    if (tid < K) values[pair * K + tid] = acc / (double)nB;
}

// One thread per (row, feature, class): the coalitions without the feature in ascending binary order, from 0.0:
// acc = acc + w[popcount(m)] * (v[m | 1 << f] - v[m]), every difference, product and sum rounded on its own.
__global__ __launch_bounds__(256) void shapley_combine_kernel(const double *__restrict__ values, long long total, int F, int K,
                                                              const ShapleyWeights sw, double *__restrict__ phi) {
    __shared__ double s_w[SHAPLEY_MAX_FEATURES];
    if (threadIdx.x < SHAPLEY_MAX_FEATURES) s_w[threadIdx.x] = sw.w[threadIdx.x];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % K), f = (int)((i / K) % F);
    const long long n = i / ((long long)K * F);
    const int M = 1 << F, half = M >> 1, bit = 1 << f, low = bit - 1;
    const double *v = values + n * M * K + k;
    double acc = 0.0;
    for (int j = 0; j < half; ++j) {
        const int m = ((j & ~low) << 1) | (j & low);
        const double d = v[(long long)(m | bit) * K] - v[(long long)m * K];
        acc = acc + s_w[__popc(m)] * d;
    }
    phi[i] = acc;
}

}  // namespace obia

using namespace obia;

extern "C" {

int obia_mlp_coalition_dev(obia_ctx *ctx, const double *x, int64_t n_rows, int n_features, const obia_mlp *mlp, const double *background,
                           int64_t n_background, const uint8_t *masks, int64_t n_masks, double *values_out) {
    OBIA_TRY(enter(ctx));
    if (!x || !mlp || !background || !values_out || n_features <= 0 || n_rows < 0) { set_error("bad arguments"); return OBIA_E_INVALID; }
    if (n_background < 1 || n_masks < 1) { set_error("mlp_coalition_values needs at least one background row and one coalition"); return OBIA_E_INVALID; }
    MlpPlan p;
    OBIA_TRY(mlp_make_plan(mlp, n_features, "mlp_coalition_values", p));
    if (!masks && n_features > SHAPLEY_MAX_FEATURES) {
        set_error("all 2^F coalitions are enumerated for at most %d features (got %d); pass explicit masks", SHAPLEY_MAX_FEATURES, n_features);
        return OBIA_E_UNSUPPORTED;
    }
    if (!masks && n_masks != (1ll << n_features)) { set_error("without masks there are 2^F = %lld coalitions, not %lld", 1ll << n_features, (long long)n_masks); return OBIA_E_INVALID; }
    if (n_background >= (1ll << 31) || n_masks >= (1ll << 31) || (n_rows > 0 && n_masks > ((1ll << 31) - 1) / n_rows)) {
        set_error("mlp_coalition_values supports fewer than 2^31 background rows and 2^31 (row, coalition) pairs per call");
        return OBIA_E_UNSUPPORTED;
    }
    if (n_rows == 0) return OBIA_OK;
    ctx->arena.reset();
    int *bad = ctx->arena.get<int>(2);
    if (!bad) return OBIA_E_NOMEM;
    OBIA_HIP_TRY(hipMemsetAsync(bad, 0, 2 * sizeof(int), ctx->stream));
    const long long nx = (long long)n_rows * n_features, nb = (long long)n_background * n_features;
    hipLaunchKernelGGL(mlp_finite_kernel, dim3(cdiv(nx, 256)), dim3(256), 0, ctx->stream, x, nx, bad, 0);
    hipLaunchKernelGGL(mlp_finite_kernel, dim3(cdiv(nb, 256)), dim3(256), 0, ctx->stream, background, nb, bad, 1);
    hipLaunchKernelGGL(mlp_coalition_kernel, dim3((unsigned)(n_rows * n_masks)), dim3(256), mlp_lds_bytes(p), ctx->stream, x, (int)n_masks,
                       mlp->weights, mlp->biases, p, background, (int)n_background, masks, values_out);
    OBIA_HIP_TRY(hipGetLastError());
    int h_bad[2] = {0, 0};
    OBIA_TRY(read_back(ctx, h_bad, bad, sizeof(h_bad)));
    if (h_bad[0]) { set_error("Input X contains NaN or infinity"); return OBIA_E_INVALID; }
    if (h_bad[1]) { set_error("Input background contains NaN or infinity"); return OBIA_E_INVALID; }
    return OBIA_OK;
}

int obia_shapley_combine_dev(obia_ctx *ctx, const double *values, int64_t n_rows, int n_features, int n_classes, const double *size_weights,
                             double *phi_out) {
    OBIA_TRY(enter(ctx));
    if (!values || !size_weights || !phi_out || n_features <= 0 || n_classes <= 0 || n_rows < 0) { set_error("bad arguments"); return OBIA_E_INVALID; }
    if (n_features > SHAPLEY_MAX_FEATURES || n_classes > MLP_MAX_CLASSES) {
        set_error("shapley_combine supports at most %d features and %d classes (got %d, %d)", SHAPLEY_MAX_FEATURES, MLP_MAX_CLASSES, n_features,
                  n_classes);
        return OBIA_E_UNSUPPORTED;
    }
    const long long total = (long long)n_rows * n_features * n_classes;
    if (n_rows >= (1ll << 31) || total >= (1ll << 31) * 256) { set_error("table too large"); return OBIA_E_UNSUPPORTED; }
    if (n_rows == 0) return OBIA_OK;
    ShapleyWeights sw = {};
    for (int s = 0; s < n_features; ++s) sw.w[s] = size_weights[s];
    hipLaunchKernelGGL(shapley_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, values, total, n_features,
                       n_classes, sw, phi_out);
    OBIA_HIP_TRY(hipGetLastError());
    OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return OBIA_OK;
}

}  // extern "C"
