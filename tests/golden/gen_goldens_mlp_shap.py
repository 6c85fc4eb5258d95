#!/usr/bin/env python3
"""Fixtures of the mlp_shap tests (run with scikit-learn 1.7.2; needs no GPU).

    python tests/golden/gen_goldens_mlp_shap.py

Each mlp_shap/<case>.npz holds the flat network (the arrays of obia_amd.classify.MLP), ``X`` (N, F) -- the rows to explain --,
``background`` (B, F), ``values_ld`` (N, 2^F, K) -- the value of every coalition in binary order, evaluated in np.longdouble
(forward pass, ordered sum over the background, one division by B) and rounded to float64 once --, ``phi_exact`` (N, F, K) and
``base_exact`` (K,) -- the Shapley values of ``values_ld`` in Fractions, rounded, and the empty coalition's value -- and
``e_comb = max(2^-52, |float64 restatement of the subset formula - phi_exact|)`` on ``values_ld``.

``author`` is the reference author's configuration (9 feature columns, 6 classes, hidden layers (100, 50, 30), lbfgs) fitted by
scikit-learn; its weights are rounded to float32 after the fit -- everything above is computed from the rounded network -- so that
the file stays small.  The rest are ``mlp_restatement.random_mlp``.  Table values are quantised so that the files compress.
"""
import os
import sys
import warnings
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import mlp_restatement as mr  # noqa: E402
from tests import mlp_shap_restatement as S  # noqa: E402


def finish(name, net, X, background):
    F = X.shape[1]
    values_ld = S.coalition_values(net, X, background, S.all_masks(F), num=np.longdouble)
    phi_exact = S.to_float(S.shapley(values_ld, num=Fraction))
    e_comb = max(2.0 ** -52, float(np.abs(S.shapley(values_ld, num=float) - phi_exact).max()))
    out = dict(net, X=X, background=background, values_ld=values_ld, phi_exact=phi_exact, base_exact=values_ld[0, 0].copy(),
               e_comb=np.float64(e_comb))
    out["hidden_activation"], out["out_activation"] = np.str_(net["hidden_activation"]), np.str_(net["out_activation"])
    os.makedirs(os.path.join(HERE, "mlp_shap"), exist_ok=True)
    path = os.path.join(HERE, "mlp_shap", f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: layers {np.asarray(net['layer_sizes']).tolist()}, {net['hidden_activation']} / {net['out_activation']}, {X.shape[0]} rows, "
          f"{background.shape[0]} background rows, e_comb {e_comb:.3g}, max|phi| {np.abs(phi_exact).max():.3g}, {os.path.getsize(path)} bytes")


def author():
    import sklearn
    from sklearn.neural_network import MLPClassifier
    from sklearn.preprocessing import StandardScaler
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    warnings.filterwarnings("ignore")
    rs = np.random.RandomState(7)
    F, K, n = 9, 6, 240
    y = np.concatenate([np.arange(K), rs.randint(0, K, n - K)])
    centre = rs.normal(0, 1.5, (K, F))
    table = np.round((centre[y] + rs.normal(0, 1.0, (n, F)) + np.linspace(-8, 8, F)[None, :]) * 64) / 64
    x_train = StandardScaler().fit_transform(table)
    clf = MLPClassifier(hidden_layer_sizes=(100, 50, 30), solver="lbfgs", random_state=7).fit(x_train, y)
    net = {"weights": np.concatenate([np.asarray(w, np.float32).ravel() for w in clf.coefs_]).astype(np.float64),
           "biases": np.concatenate([np.asarray(b, np.float32).ravel() for b in clf.intercepts_]).astype(np.float64),
           "layer_sizes": np.asarray([F] + [w.shape[1] for w in clf.coefs_], np.int32),
           "hidden_activation": clf.activation, "out_activation": clf.out_activation_, "classes_": np.asarray(clf.classes_)}
    quant = np.round(x_train * 256) / 256
    finish("author", net, quant[:1].copy(), quant[20:44].copy())


def synthetic(name, seed, layer_sizes, hidden, out, n, b, tie_column=None):
    rs = np.random.RandomState(seed)
    net = mr.random_mlp(rs, layer_sizes, hidden, out)
    F = layer_sizes[0]
    X = np.round(rs.normal(0, 1.5, (n, F)) * 64) / 64
    background = np.round(rs.normal(0, 1.5, (b, F)) * 64) / 64
    if tie_column is not None:                    # a null feature: row 0 equals every background row there
        background[:, tie_column] = X[0, tie_column]
    finish(name, net, X, background)


def main():
    author()
    synthetic("r1", 11, [5, 16, 3], "tanh", "softmax", 4, 7, tie_column=2)
    synthetic("r2", 12, [3, 8, 1], "relu", "logistic", 5, 33)
    synthetic("r3", 13, [7, 12, 10, 4], "logistic", "softmax", 3, 5)


if __name__ == "__main__":
    main()
