#!/usr/bin/env python3
"""Fixtures of the MLP prediction tests: scikit-learn's own answers (run with scikit-learn 1.7.2; needs no GPU).

    python tests/golden/gen_goldens_mlp.py

Each mlp/<case>.npz (a directory of its own: other suites take every .npz next to this script for a SLIC case) holds the flat
network (weights, biases, layer_sizes, hidden_activation, out_activation, classes_: the arrays of obia_amd.classify.MLP), a
float64 ``table``, StandardScaler's ``mean_`` / ``scale_`` / ``transformed`` float64 table for it, ``proba`` / ``predict`` of
MLPClassifier on the whole transformed table in one call, ``proba_ld`` -- the same forward pass evaluated in np.longdouble and
rounded to float64 -- and ``e_ref = max|proba - proba_ld|``: how far scikit-learn's own float64 result is from the better one.
The flow is the one of obia ``classify``: a scaler of its own for the training rows, another one for the table to predict.
Every row's top-two margin in ``proba`` is at least 1e-6 (asserted), so a class test needs to leave no row out.  Table values
are quantised so that the files compress (the arithmetic does not care).
"""
import os
import warnings

import numpy as np
import sklearn
from sklearn.neural_network import MLPClassifier
from sklearn.preprocessing import StandardScaler

HERE = os.path.dirname(os.path.abspath(__file__))
MIN_MARGIN = 1e-6


def table(rs, n, F, K, y, sep, grid):
    """Class-dependent columns (class centres ``sep`` standard deviations apart) around different offsets; values on a grid of
    1 / ``grid``."""
    centre = rs.normal(0, sep, (K, F))
    x = centre[y] + rs.normal(0, 1.0, (n, F)) + np.linspace(-8, 8, F)[None, :]
    return np.round(x * grid) / grid


def flat(clf):
    return {"weights": np.concatenate([np.asarray(w, np.float64).ravel() for w in clf.coefs_]),
            "biases": np.concatenate([np.asarray(b, np.float64).ravel() for b in clf.intercepts_]),
            "layer_sizes": np.asarray([clf.coefs_[0].shape[0]] + [w.shape[1] for w in clf.coefs_], np.int32),
            "hidden_activation": np.str_(clf.activation), "out_activation": np.str_(clf.out_activation_),
            "classes_": np.asarray(clf.classes_)}


def forward_longdouble(clf, X):
    """MLPClassifier.predict_proba in np.longdouble, rounded to float64 at the very end."""
    L = np.longdouble
    a = X.astype(L)
    act = {"identity": lambda z: z, "relu": lambda z: np.maximum(z, L(0)), "tanh": np.tanh,
           "logistic": lambda z: L(1) / (L(1) + np.exp(-z))}[clf.activation]
    n = len(clf.coefs_)
    for i, (W, b) in enumerate(zip(clf.coefs_, clf.intercepts_)):
        a = a @ W.astype(L) + b.astype(L)
        if i + 1 < n:
            a = act(a)
    if clf.out_activation_ == "logistic":
        p = L(1) / (L(1) + np.exp(-a[:, 0]))
        out = np.stack([L(1) - p, p], axis=1)
    else:
        e = np.exp(a - a.max(axis=1, keepdims=True))
        out = e / e.sum(axis=1, keepdims=True)
    return out.astype(np.float64)


def case(name, seed, n_train, n_pred, F, K, mlp_kwargs, classes=None, sep=1.5, grid=64, write=True):
    rs = np.random.RandomState(seed)
    classes = np.arange(K) if classes is None else np.asarray(classes)
    y = np.concatenate([np.arange(K), rs.randint(0, K, n_train - K)])      # every class is present
    rs2 = np.random.RandomState(seed + 1000)
    both = table(rs2, n_train + n_pred, F, K, np.concatenate([y, rs.randint(0, K, n_pred)]), sep, grid)
    xt, xp = both[:n_train].copy(), both[n_train:].copy()
    clf = MLPClassifier(random_state=seed, **mlp_kwargs)
    clf.fit(StandardScaler().fit_transform(xt), classes[y])
    sc = StandardScaler().fit(xp)
    tr = sc.transform(xp)
    assert tr.dtype == np.float64
    proba = clf.predict_proba(tr)
    proba_ld = forward_longdouble(clf, tr)
    out = flat(clf)
    out.update(table=xp, mean_=sc.mean_, scale_=sc.scale_, transformed=tr, proba=proba, predict=clf.predict(tr), proba_ld=proba_ld,
               e_ref=np.float64(np.abs(proba - proba_ld).max()))
    top = np.sort(proba, 1)
    margin = float((top[:, -1] - top[:, -2]).min())
    assert margin >= MIN_MARGIN, (name, margin)
    assert np.array_equal(classes[np.argmax(proba, 1)], out["predict"])
    if not write:
        return clf, out
    os.makedirs(os.path.join(HERE, "mlp"), exist_ok=True)
    path = os.path.join(HERE, "mlp", f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: layers {out['layer_sizes'].tolist()}, {clf.activation} / {clf.out_activation_}, {n_pred} rows, smallest top-two "
          f"margin {margin:.3g}, e_ref {float(out['e_ref']):.3g}, {os.path.getsize(path)} bytes")
    return margin


CASES = {
    # (a) scikit-learn's default network
    "a": lambda write: case("a", 1, 400, 1000, 20, 5, dict(), write=write),
    # (b) two classes: one logistic output unit; more than one wave of rows, not a multiple of 64
    "b": lambda write: case("b", 2, 120, 70, 12, 2, dict(), write=write),
    # (c) two hidden layers, tanh, the width of the author's table without its five all-NaN point-cloud columns
    "c": lambda write: case("c", 3, 400, 1000, 96, 7, dict(hidden_layer_sizes=(64, 32), activation="tanh"), grid=4, write=write),
    # (d) logistic hidden units
    "d": lambda write: case("d", 4, 300, 200, 30, 4, dict(hidden_layer_sizes=(50,), activation="logistic"), write=write),
    # (e) a narrow identity layer, class values that are not 0 .. K-1, one row more than 64
    "e": lambda write: case("e", 5, 300, 65, 3, 9, dict(hidden_layer_sizes=(7,), activation="identity"),
                            classes=[3, 5, 8, 13, 21, 34, 55, 89, 144], write=write),
    # (f) no hidden layer: a single weight matrix
    "f": lambda write: case("f", 6, 200, 200, 6, 3, dict(hidden_layer_sizes=()), write=write),
}


def main(only=None, write=True):
    """Writes every fixture; ``main(only="c", write=False)`` returns (fitted classifier, arrays) of one case instead."""
    warnings.filterwarnings("ignore")                                # ConvergenceWarning: the default 200 iterations are what the reference runs
    if only is not None:
        return CASES[only](write)
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    for name in sorted(CASES):
        CASES[name](True)


if __name__ == "__main__":
    main()
