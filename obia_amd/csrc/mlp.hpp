// mlp.hpp -- what mlp.hip (prediction) and mlp_shap.hip (coalition values) share: the limits, the launch plan and the layer loop of
// the forward pass.  One copy of the loop is what makes the two kernels give the same bits for the same row.
#pragma once
#include "common.hpp"

#include <cfloat>
#include <cmath>

namespace obia {

constexpr int MLP_MAX_LAYERS = 8;        // weight matrices
constexpr int MLP_MAX_FEATURES = 4096;
constexpr int MLP_MAX_CLASSES = 64;
constexpr int MLP_MAX_WIDTH = 512;       // hidden units per layer
constexpr int MLP_LDS_DOUBLES = 8192;    // 64 KB of dynamic LDS: what a launch gets without asking for more
constexpr int MLP_MIN_CHUNK = 8;         // features the input staging buffer holds at least
constexpr int MLP_U = 8;                 // output units a thread carries in registers per pass

struct MlpPlan {
    int32_t sizes[MLP_MAX_LAYERS + 1];   // n_features, hidden widths ..., n_out
    int64_t woff[MLP_MAX_LAYERS];        // first weight of every matrix
    int32_t boff[MLP_MAX_LAYERS];        // first bias of every layer
    int32_t n_layers, hidden_act, out_act, n_classes;
    int32_t rshift;                      // a workgroup takes R = 1 << rshift rows
    int32_t wmax;                        // widest layer output: each of the two activation buffers is wmax * R doubles
    int32_t chunk;                       // features of the input layer staged at a time
};

// Checks the network against the limits and the table's width and fills the plan (`who` names the caller in the messages).
// OBIA_OK, OBIA_E_INVALID or OBIA_E_UNSUPPORTED with the error text set.
inline int mlp_make_plan(const obia_mlp *mlp, int n_features, const char *who, MlpPlan &p) {
    if (!mlp) { set_error("bad arguments"); return OBIA_E_INVALID; }
    const obia_mlp &m = *mlp;
    if (!m.weights || !m.biases || !m.layer_sizes || m.n_layers <= 0 || m.n_classes <= 0) { set_error("bad mlp"); return OBIA_E_INVALID; }
    if (m.n_layers > MLP_MAX_LAYERS || n_features > MLP_MAX_FEATURES || m.n_classes > MLP_MAX_CLASSES) {
        set_error("%s supports at most %d weight matrices, %d features and %d classes (got %d, %d, %d)", who, MLP_MAX_LAYERS,
                  MLP_MAX_FEATURES, MLP_MAX_CLASSES, m.n_layers, n_features, m.n_classes);
        return OBIA_E_UNSUPPORTED;
    }
    p = MlpPlan{};
    long long woff = 0;
    int boff = 0, wmax = 0;
    for (int l = 0; l <= m.n_layers; ++l) {
        const int w = m.layer_sizes[l];
        if (w <= 0) { set_error("mlp: layer %d has no units", l); return OBIA_E_INVALID; }
        if (l > 0 && l < m.n_layers && w > MLP_MAX_WIDTH) {
            set_error("%s supports hidden layers of at most %d units (layer %d has %d)", who, MLP_MAX_WIDTH, l, w);
            return OBIA_E_UNSUPPORTED;
        }
        p.sizes[l] = w;
        if (l > 0) {
            p.woff[l - 1] = woff;
            p.boff[l - 1] = boff;
            woff += (long long)m.layer_sizes[l - 1] * w;
            boff += w;
            if (w > wmax) wmax = w;
        }
    }
    const int n_out = m.layer_sizes[m.n_layers];
    if (m.layer_sizes[0] != n_features) {
        set_error("mlp: the network takes %d features, the table has %d columns", m.layer_sizes[0], n_features);
        return OBIA_E_INVALID;
    }
    if (m.hidden_activation < 0 || m.hidden_activation > 3 || m.out_activation < 0 || m.out_activation > 1 ||
        (m.out_activation == 0 && n_out != m.n_classes) || (m.out_activation == 1 && (n_out != 1 || m.n_classes != 2))) {
        set_error("mlp: activations or output width do not fit the classes (softmax: n_out = n_classes; logistic: n_out = 1, 2 classes)");
        return OBIA_E_INVALID;
    }
    // rows per workgroup: the most for which two activation buffers and a staging buffer of MLP_MIN_CHUNK features fit
    int rshift = 6;
    while (2 * wmax * (1 << rshift) + MLP_MIN_CHUNK * ((1 << rshift) + 1) > MLP_LDS_DOUBLES) --rshift;   // ends at 4 rows for 512 units
    const int R = 1 << rshift;
    const int room = (MLP_LDS_DOUBLES - 2 * wmax * R) / (R + 1);
    p.n_layers = m.n_layers;
    p.hidden_act = m.hidden_activation;
    p.out_act = m.out_activation;
    p.n_classes = m.n_classes;
    p.rshift = rshift;
    p.wmax = wmax;
    p.chunk = n_features < room ? n_features : room;
    return OBIA_OK;
}

inline size_t mlp_lds_bytes(const MlpPlan &p) {
    const size_t R = (size_t)1 << p.rshift;
    return (2 * (size_t)p.wmax * R + (size_t)p.chunk * (R + 1)) * sizeof(double);
}

#if defined(__HIPCC__)
__device__ __forceinline__ double mlp_hidden(double z, int act) {
    switch (act) {
        case 1: return z > 0 ? z : 0.0;
        case 2: return tanh(z);
        case 3: return 1.0 / (1.0 + exp(-z));
        default: return z;
    }
}

// The layers of the forward pass for the R rows of a 256-thread workgroup.  Thread t works on row r = t % R for unit group
// g = t / R; a group carries MLP_U units of a layer in registers per pass and the 256 / R groups walk the layer's units together.
// Activations sit in LDS unit-major, [unit][R]: the lanes of a wave read consecutive doubles (or the same ones, broadcast), and a
// thread reads one activation per MLP_U multiply-adds.  Two such buffers alternate per layer.  The input layer comes from
// `load(row of the workgroup, feature)` in chunks of `chunk` features, staged transposed with row stride R + 1; between chunks a
// unit's running sum waits in the destination buffer -- a store and a load of a double, which changes no bit of the ordered sum.
// smem: [wmax][R], [wmax][R], [chunk][R + 1] doubles (mlp_lds_bytes).  Returns the buffer that holds the logits, [n_out][R]; all
// threads of the workgroup have passed a barrier after the last store into it.
template <class Load>
__device__ __forceinline__ const double *mlp_layers(const MlpPlan &p, const double *__restrict__ Wt, const double *__restrict__ Bs,
                                                    unsigned char *smem, Load load) {
    const int R = 1 << p.rshift, G = 256 >> p.rshift;
    double *buf0 = reinterpret_cast<double *>(smem);       // [wmax][R]
    double *buf1 = buf0 + p.wmax * R;                       // [wmax][R]
    double *s_x = buf1 + p.wmax * R;                        // [chunk][R + 1]
    const int tid = threadIdx.x, r = tid & (R - 1), g = tid >> p.rshift;

    const double *src = nullptr;
    for (int l = 0; l < p.n_layers; ++l) {
        const int n_in = p.sizes[l], n_out = p.sizes[l + 1];
        double *dst = (l & 1) ? buf1 : buf0;
        const double *W = Wt + p.woff[l], *B = Bs + p.boff[l];
        const int step = l == 0 ? p.chunk : n_in;
        for (int f0 = 0; f0 < n_in; f0 += step) {
            const int fc = (n_in - f0) < step ? (n_in - f0) : step;
            const double *a;
            int astride;
            if (l == 0) {
                if (f0) __syncthreads();                    // the chunk before has been read by everyone
                for (int i = tid; i < R * fc; i += 256) {
                    const int rr = i / fc, f = i - rr * fc;
                    s_x[f * (R + 1) + rr] = load(rr, f0 + f);
                }
                __syncthreads();
                a = s_x + r;
                astride = R + 1;
            } else {
                a = src + r;
                astride = R;
            }
            const bool first = f0 == 0, last = f0 + fc == n_in;
            for (int j0 = g * MLP_U; j0 < n_out; j0 += G * MLP_U) {
                const int nu = (n_out - j0) < MLP_U ? (n_out - j0) : MLP_U;
                double *d = dst + j0 * R + r;
                const double *w = W + (long long)f0 * n_out + j0;
                double acc[MLP_U];
#pragma unroll
                for (int u = 0; u < MLP_U; ++u) acc[u] = (first || u >= nu) ? 0.0 : d[u * R];
                if (nu == MLP_U) {
                    for (int f = 0; f < fc; ++f) {
                        const double av = a[f * astride];
#pragma unroll
                        for (int u = 0; u < MLP_U; ++u) acc[u] = acc[u] + av * w[u];
                        w += n_out;
                    }
                } else {
                    for (int f = 0; f < fc; ++f) {
                        const double av = a[f * astride];
#pragma unroll
                        for (int u = 0; u < MLP_U; ++u)
                            if (u < nu) acc[u] = acc[u] + av * w[u];
                        w += n_out;
                    }
                }
#pragma unroll
                for (int u = 0; u < MLP_U; ++u) {
                    if (u < nu) {
                        double z = acc[u];
                        if (last) {
                            z = z + B[j0 + u];
                            if (l + 1 < p.n_layers) z = mlp_hidden(z, p.hidden_act);
                        }
                        d[u * R] = z;
                    }
                }
            }
        }
        __syncthreads();
        src = dst;
    }
    return src;
}
#endif

}  // namespace obia
