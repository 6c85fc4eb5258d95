"""NumPy restatement of scikit-learn's random-forest prediction and of the class filter of obia ``classify`` (test
infrastructure: the CPU tests pin it on scikit-learn's own output bit for bit, the GPU tests use it where a fixture stores no
answer -- the masked prediction, the synthetic edge forests).

The loop, per tree t = 0 .. T-1 in that order: cast the table to float32; at a node compare ``float64(x) <= threshold``
(threshold float64); a NaN feature goes left iff ``missing_go_to_left``; a node with left child -1 is a leaf; add the leaf's
row of ``value`` to a float64 accumulator.  Divide by T.  ``forest`` is anything with the flat arrays of
``obia_amd.classify.Forest`` as attributes or keys.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["a", "b", "c", "d", "e"]                 # tests/golden/forest/<case>.npz (gen_goldens_forest.py)
ARRAYS = ("threshold", "feature", "left", "right", "missing_go_to_left", "tree_offset", "value")


def load_case(name):
    with np.load(os.path.join(GOLDEN, "forest", f"{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def forest_of(case):
    """The obia_amd.classify.Forest of a fixture (or of a random_forest dict)."""
    from obia_amd.classify import Forest
    return Forest(classes_=case["classes_"], n_features=int(case["n_features"]), **{k: case[k] for k in ARRAYS})


def _get(forest, name):
    return np.asarray(forest[name] if isinstance(forest, dict) or hasattr(forest, "files") else getattr(forest, name))


def leaves(forest, X):
    """(T, N) global node index of the leaf every row ends in, per tree."""
    thr, feat = _get(forest, "threshold"), _get(forest, "feature")
    left, right = _get(forest, "left").astype(np.int64), _get(forest, "right").astype(np.int64)
    mgl, off = _get(forest, "missing_go_to_left"), _get(forest, "tree_offset").astype(np.int64)
    X32 = np.asarray(X).astype(np.float32)
    N = X32.shape[0]
    rows = np.arange(N)
    out = np.empty((len(off), N), np.int64)
    for t, base in enumerate(off):
        node = np.full(N, base, np.int64)
        while True:
            inner = left[node] >= 0
            if not inner.any():
                break
            v = X32[rows, np.where(inner, feat[node], 0)]
            with np.errstate(invalid="ignore"):
                go_left = np.where(np.isnan(v), mgl[node] != 0, v.astype(np.float64) <= thr[node])
            node = np.where(inner, base + np.where(go_left, left[node], right[node]), node)
        out[t] = node
    return out


def predict_proba(forest, X):
    value = _get(forest, "value")
    lv = leaves(forest, X)
    acc = np.zeros((lv.shape[1], value.shape[1]), np.float64)
    for t in range(lv.shape[0]):
        acc += value[lv[t]]
    acc /= lv.shape[0]
    return acc


def choose(proba, acceptable=None):
    """(pred, margin) of classify.py:145-158 per row: the first maximum of ``proba`` over the acceptable classes (``idxmax`` on
    the filtered columns / ``np.argmax``) and the largest minus the second largest of those values (``np.partition(..., -2)``).
    A row with fewer than two candidates raises ValueError, as the reference's ``np.partition`` / ``idxmax`` do."""
    proba = np.asarray(proba)
    N, K = proba.shape
    acc = np.ones((N, K), bool) if acceptable is None else np.asarray(acceptable) != 0
    if acc.shape != (N, K):
        raise ValueError("acceptable must be (rows, classes)")
    pred, margin = np.empty(N, np.int32), np.empty(N, np.float64)
    for i in range(N):
        idx = np.flatnonzero(acc[i])
        if len(idx) < 2:
            raise ValueError(f"row {i} has fewer than two acceptable classes")
        p = proba[i, idx]
        pred[i] = idx[np.argmax(p)]
        top2 = np.partition(p, -2)[-2:]
        margin[i] = top2[1] - top2[0]
    return pred, margin


def random_forest(rs, n_trees, n_features, n_classes, max_depth, leaf_only=False):
    """A synthetic forest as a dict of flat arrays (no training): random splits, children allocated breadth-first so that the
    left child is NOT node + 1, random ``missing_go_to_left``, leaf rows = random fractions.  ``leaf_only``: every tree is one
    leaf."""
    thr, feat, left, right, mgl, val, off = [], [], [], [], [], [], []
    total = 0
    for _ in range(n_trees):
        off.append(total)
        nodes = [0]                       # depth of every node, in allocation order
        t_left, t_right = [], []
        i = 0
        while i < len(nodes):
            d = nodes[i]
            if not leaf_only and d < max_depth and (d == 0 or rs.rand() < 0.7):
                t_left.append(len(nodes))
                t_right.append(len(nodes) + 1)
                nodes += [d + 1, d + 1]
            else:
                t_left.append(-1)
                t_right.append(-1)
            i += 1
        n = len(nodes)
        is_leaf = np.asarray(t_left) < 0
        thr.append(np.where(is_leaf, -2.0, rs.normal(0, 1, n)))
        feat.append(np.where(is_leaf, -2, rs.randint(0, n_features, n)).astype(np.int32))
        left.append(np.asarray(t_left, np.int32))
        right.append(np.asarray(t_right, np.int32))
        mgl.append(rs.randint(0, 2, n).astype(np.uint8))
        v = rs.randint(0, 5, (n, n_classes)).astype(np.float64) + (rs.rand(n, 1) < 0.5)
        val.append(v / v.sum(1, keepdims=True).clip(1))
        total += n
    return {"threshold": np.concatenate(thr), "feature": np.concatenate(feat), "left": np.concatenate(left),
            "right": np.concatenate(right), "missing_go_to_left": np.concatenate(mgl), "tree_offset": np.asarray(off, np.int64),
            "value": np.concatenate(val), "classes_": np.arange(n_classes), "n_features": n_features}
