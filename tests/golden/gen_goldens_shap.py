#!/usr/bin/env python3
"""Fixtures of the SHAP tests: exact answers in rational arithmetic (needs scikit-learn 1.7.2 for the fitted forests; no GPU).

    python tests/golden/gen_goldens_shap.py [case ...]

Each shap/<case>.npz holds the flat forest arrays plus ``cover``, ``classes_`` and ``n_features``; ``X32``, the float32 rows the
tests use (``rows``: their indices in the forest fixture's table, empty for the synthetic cases); ``phi_exact`` / ``base_exact``,
the result of tests/shap_restatement.py in ``fractions.Fraction`` rounded to float64; and ``e_ref``, the largest distance from
these of the float64 restatement over the natural element order and 8 seeded random orders, floored at 2^-52.  The fitted
forests are those of gen_goldens_forest.py (refitted here, checked against the stored arrays), so tests/golden/forest/<case>.npz
holds scikit-learn's ``proba`` for the same rows.
"""
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import shap_restatement as S  # noqa: E402

N_ORDERS = 8


def forest_case(name):
    import gen_goldens_forest as G
    rf, out = G.main(only=name, write=False)
    with np.load(os.path.join(HERE, "forest", f"{name}.npz"), allow_pickle=False) as z:
        for k in S.ARRAYS:
            assert np.array_equal(out[k], z[k], equal_nan=True), (name, k)
        assert np.array_equal(out["transformed"], z["transformed"], equal_nan=True)
    arrays = {k: out[k] for k in S.ARRAYS + ("classes_", "n_features")}
    arrays["cover"] = np.concatenate([np.asarray(e.tree_.weighted_n_node_samples, np.float64) for e in rf.estimators_])
    return arrays, out["transformed"].astype(np.float32)


def rows_of(name, X32):
    n = X32.shape[0]
    if name == "b":
        return np.arange(n)
    if name == "c":
        return np.arange(40)
    if name == "a":               # NaNs in columns 7 and 9 (column 3 is all NaN, column 5 constant), and rows without
        nan7, nan9 = np.flatnonzero(np.isnan(X32[:, 7])), np.flatnonzero(np.isnan(X32[:, 9]))
        both = np.intersect1d(nan7, nan9)
        clean = np.flatnonzero(~np.isnan(X32[:, 7]) & ~np.isnan(X32[:, 9]))
        rows = np.unique(np.concatenate([nan7[:12], nan9[:12], both[:4]]))
        return np.sort(np.concatenate([rows, np.setdiff1d(clean, rows)[:48 - len(rows)]]))
    if name == "d":
        return np.arange(7)
    if name == "e":
        return np.arange(32)
    raise KeyError(name)


def comb_case(n_chain):
    arrays = S.comb_forest(n_chain)
    F = int(arrays["n_features"])
    rs = np.random.RandomState(100 + n_chain)
    X = rs.normal(0, 1, (16, F))
    X[:8] += 4.0                                   # above every threshold of the chain: these rows reach its deepest leaves
    X[2, F - 1] = -6.0                             # ... one of them turns off at the last split, one at the first
    X[3, 0] = -6.0
    X[4, 1] = np.nan
    return arrays, (np.round(X * 16) / 16).astype(np.float32)


def build(name):
    if name.startswith("comb"):
        arrays, X32 = comb_case(int(name[4:]))
        rows = np.zeros(0, np.int64)
    else:
        arrays, table = forest_case(name)
        rows = rows_of(name, table)
        X32 = table[rows]
    phi_q, base_q = S.shap_values(arrays, X32, num=Fraction)
    phi_exact, base_exact = S.to_float(phi_q), S.to_float(base_q)
    e_ref = 2.0 ** -52
    for order in [None] + list(range(N_ORDERS)):
        phi_f, base_f = S.shap_values(arrays, X32, num=float, order=order)
        e_ref = max(e_ref, float(np.abs(phi_f - phi_exact).max()), float(np.abs(base_f - base_exact).max()))
    path = os.path.join(HERE, "shap", f"{name}.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, X32=X32, rows=rows, phi_exact=phi_exact, base_exact=base_exact, e_ref=np.float64(e_ref), **arrays)
    longest = max(len(p["elems"]) for p in S.paths(arrays))
    print(f"{name}: {X32.shape[0]} rows, {len(arrays['tree_offset'])} trees, {len(arrays['threshold'])} nodes, longest path "
          f"{longest} distinct features, e_ref {e_ref:.3e}, {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    for case in (sys.argv[1:] or S.CASES):
        build(case)
