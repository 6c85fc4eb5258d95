#!/usr/bin/env python3
"""Fixtures of the classification tests: scikit-learn's own answers (run with scikit-learn 1.7.2; needs no GPU).

    python tests/golden/gen_goldens_forest.py

Each forest/<case>.npz (a directory of its own: other suites take every .npz next to this script for a SLIC case) holds the flat forest arrays (threshold, feature, left, right, missing_go_to_left, tree_offset, value,
classes_, n_features), a float64 ``table``, StandardScaler's ``mean_`` / ``scale_`` / ``transformed`` table for it, and
``proba`` / ``predict`` of RandomForestClassifier (n_jobs=None) on the transformed table.  The flow is the one of obia
``classify``: a scaler of its own for the training rows, another one for the table to predict.  The GPU tests read only these
files, so they need no scikit-learn.  Table values are quantised so that the files compress (the arithmetic does not care).
"""
import os
import warnings

import numpy as np
import sklearn
from sklearn.ensemble import RandomForestClassifier
from sklearn.preprocessing import StandardScaler

HERE = os.path.dirname(os.path.abspath(__file__))


def table(rs, n, F, K, y, sep, grid):
    """Class-dependent columns (class centres ``sep`` standard deviations apart) around different offsets; values on a grid of
    1 / ``grid``."""
    centre = rs.normal(0, sep, (K, F))
    x = centre[y] + rs.normal(0, 1.0, (n, F)) + np.linspace(-8, 8, F)[None, :]
    return np.round(x * grid) / grid


def flat(rf):
    parts = {k: [] for k in ("threshold", "feature", "left", "right", "missing_go_to_left", "value")}
    off, total = [], 0
    for est in rf.estimators_:
        t = est.tree_
        off.append(total)
        parts["threshold"].append(t.threshold.astype(np.float64))
        parts["feature"].append(t.feature.astype(np.int32))
        parts["left"].append(t.children_left.astype(np.int32))
        parts["right"].append(t.children_right.astype(np.int32))
        parts["missing_go_to_left"].append(np.asarray(t.missing_go_to_left, np.uint8))
        parts["value"].append(t.value[:, 0, :].astype(np.float64))          # 1.7.2: class fractions, returned as they are
        total += t.node_count
    out = {k: np.concatenate(v) for k, v in parts.items()}
    out["tree_offset"] = np.asarray(off, np.int64)
    out["classes_"] = np.asarray(rf.classes_)
    out["n_features"] = np.int64(rf.n_features_in_)
    return out


def case(name, seed, n_train, n_pred, F, K, rf_kwargs, nan_cols=(), const_col=None, train_nan=None, pred_nan=None, classes=None,
         sep=1.5, grid=64, write=True):
    rs = np.random.RandomState(seed)
    classes = np.arange(K) if classes is None else np.asarray(classes)
    y = np.concatenate([np.arange(K), rs.randint(0, K, n_train - K)])      # every class is present
    rs2 = np.random.RandomState(seed + 1000)
    both = table(rs2, n_train + n_pred, F, K, np.concatenate([y, rs.randint(0, K, n_pred)]), sep, grid)
    xt, xp = both[:n_train].copy(), both[n_train:].copy()
    for c in nan_cols:                       # the reference's five point-cloud columns: always NaN
        xt[:, c] = np.nan
        xp[:, c] = np.nan
    if const_col is not None:
        xt[:, const_col] = 3.25
        xp[:, const_col] = 3.25
    for c, frac in (train_nan or {}).items():
        xt[rs.rand(n_train) < frac, c] = np.nan
    for c, frac in (pred_nan or {}).items():
        xp[rs.rand(n_pred) < frac, c] = np.nan
    rf = RandomForestClassifier(random_state=seed, **rf_kwargs)
    rf.fit(StandardScaler().fit_transform(xt), classes[y])
    sc = StandardScaler().fit(xp)
    tr = sc.transform(xp)
    proba = rf.predict_proba(tr)
    out = flat(rf)
    out.update(table=xp, mean_=sc.mean_, scale_=sc.scale_, transformed=tr, proba=proba, predict=rf.predict(tr))
    if not write:
        return rf, out
    path = os.path.join(HERE, "forest", f"{name}.npz")
    np.savez_compressed(path, **out)
    top = np.sort(proba, 1)
    ties = int((top[:, -1] == top[:, -2]).sum())
    depth = max(e.tree_.max_depth for e in rf.estimators_)
    not_next = int(sum(((e.tree_.children_left >= 0) & (e.tree_.children_left != np.arange(e.tree_.node_count) + 1)).sum()
                       for e in rf.estimators_))
    print(f"{name}: {len(out['threshold'])} nodes, depth {depth}, {ties} of {n_pred} rows tie at the top, "
          f"{not_next} left children that are not node + 1, {os.path.getsize(path)} bytes")
    return ties, not_next


def main(only=None, write=True):
    """Writes every fixture; ``main(only="c", write=False)`` returns (fitted forest, arrays) of one case instead."""
    warnings.filterwarnings("ignore", category=RuntimeWarning)       # the all-NaN columns divide 0 by 0 inside StandardScaler
    if only is not None:
        return CASES[only](write)
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    for name in sorted(CASES):
        CASES[name](True)


def _a(write):
    # (a) NaN handling of every kind + ties at the top: column 3 all NaN, column 5 constant, column 7 with NaNs in training and
    #     in prediction, column 9 with NaNs in prediction only
    r = case("a", 1, 400, 3000, 12, 4, dict(n_estimators=25), nan_cols=(3,), const_col=5, train_nan={7: 0.10},
             pred_nan={7: 0.20, 9: 0.05}, sep=0.3, write=write)
    assert not write or r[0] > 0
    return r


def _c(write):
    # (c) best-first trees: the left child is not node + 1
    r = case("c", 3, 300, 200, 6, 9, dict(n_estimators=3, max_leaf_nodes=17), classes=[3, 5, 8, 13, 21, 34, 55, 89, 144], write=write)
    assert not write or r[1] > 0
    return r


CASES = {
    "a": _a,
    # (b) one shallow tree, more than one wave of rows, not a multiple of 64
    "b": lambda write: case("b", 2, 60, 70, 3, 2, dict(n_estimators=1, max_depth=2), write=write),
    "c": _c,
    # (d) far more trees than rows
    "d": lambda write: case("d", 4, 120, 7, 5, 3, dict(n_estimators=200), write=write),
    # (e) the width of the author's table: 96 statistics + the five all-NaN point-cloud columns
    "e": lambda write: case("e", 5, 300, 1000, 101, 5, dict(n_estimators=10), nan_cols=(96, 97, 98, 99, 100), grid=4, write=write),
}


if __name__ == "__main__":
    main()
