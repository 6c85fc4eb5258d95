"""NumPy float64 restatement of the arithmetic contract of ``mlp_predict`` (test infrastructure: the CPU tests
hold it against scikit-learn's stored answers, the GPU tests against the kernel bit for bit where the activations are exact).

Per layer: ``acc = 0.0``; for every input index f in ascending order ``acc += a[:, f:f+1] * W[f:f+1, :]`` (each product and each
sum rounded on its own); then ``acc + b``.  Hidden activations: identity, ``np.where(z > 0, z, 0.0)``, ``np.tanh``,
``1 / (1 + np.exp(-z))``.  Output: softmax as ``exp(z - max z)`` divided by its sum taken in ascending class order; binary
logistic ``p = 1 / (1 + exp(-z_0))``, ``proba = [1 - p, p]``.  ``mlp`` is anything with the flat arrays of ``obia_amd.classify.MLP``
as attributes or keys.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp")
CASES = ["a", "b", "c", "d", "e", "f"]            # tests/golden/mlp/<case>.npz (gen_goldens_mlp.py)
ARRAYS = ("weights", "biases", "layer_sizes")


def load_case(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def pooled_e_ref():
    """E of the tolerance tests: the largest ``e_ref`` = max|scikit-learn's proba - the longdouble forward pass| over ALL fixtures."""
    return max(float(load_case(n)["e_ref"]) for n in CASES)


def mlp_of(case):
    """The obia_amd.classify.MLP of a fixture (or of a random_mlp dict)."""
    from obia_amd.classify import MLP
    return MLP(classes_=case["classes_"], hidden_activation=str(case["hidden_activation"]), out_activation=str(case["out_activation"]),
               **{k: case[k] for k in ARRAYS})


def _get(mlp, name):
    return mlp[name] if isinstance(mlp, dict) or hasattr(mlp, "files") else getattr(mlp, name)


def layers(mlp):
    ls = np.asarray(_get(mlp, "layer_sizes")).tolist()
    w, b = np.asarray(_get(mlp, "weights"), np.float64), np.asarray(_get(mlp, "biases"), np.float64)
    out, wo, bo = [], 0, 0
    for n_in, n_out in zip(ls[:-1], ls[1:]):
        out.append((w[wo:wo + n_in * n_out].reshape(n_in, n_out), b[bo:bo + n_out]))
        wo, bo = wo + n_in * n_out, bo + n_out
    return out


def logits(mlp, X):
    """(N, n_out) float64: the last layer before its activation."""
    a = np.asarray(X, np.float64)
    hidden = str(_get(mlp, "hidden_activation"))
    ly = layers(mlp)
    for i, (W, b) in enumerate(ly):
        acc = np.zeros((a.shape[0], W.shape[1]), np.float64)
        for f in range(W.shape[0]):
            acc += a[:, f:f + 1] * W[f:f + 1, :]
        z = acc + b
        if i + 1 < len(ly):
            if hidden == "relu":
                z = np.where(z > 0, z, 0.0)
            elif hidden == "tanh":
                z = np.tanh(z)
            elif hidden == "logistic":
                z = 1.0 / (1.0 + np.exp(-z))
            elif hidden != "identity":
                raise ValueError(hidden)
        a = z
    return a


def proba_of_logits(z, out_activation):
    if str(out_activation) == "logistic":
        p = 1.0 / (1.0 + np.exp(-z[:, 0]))
        return np.stack([1.0 - p, p], axis=1)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    s = np.zeros(z.shape[0], np.float64)
    for k in range(z.shape[1]):
        s += e[:, k]
    return e / s[:, None]


def predict_proba(mlp, X):
    return proba_of_logits(logits(mlp, X), _get(mlp, "out_activation"))


def random_mlp(rs, layer_sizes, hidden_activation="relu", out_activation="softmax"):
    """A synthetic network as a dict of flat arrays (no training): weights ~ N(0, 1 / n_in), biases ~ N(0, 0.1)."""
    ls = [int(v) for v in layer_sizes]
    w = np.concatenate([rs.normal(0, 1.0 / np.sqrt(a), a * b) for a, b in zip(ls[:-1], ls[1:])])
    b = rs.normal(0, 0.1, sum(ls[1:]))
    K = 2 if out_activation == "logistic" else ls[-1]
    return {"weights": w, "biases": b, "layer_sizes": np.asarray(ls, np.int32), "hidden_activation": hidden_activation,
            "out_activation": out_activation, "classes_": np.arange(K)}
