"""Timing of the classification step (obia_amd.classify) on one GPU: standard_scale and forest_predict on a table of the
author's size (489 480 segments) with 96 feature columns, against a forest of 100 trees grown here on synthetic data
(scikit-learn, host).  Device events on the stream the library's context runs on.  Prints one JSON line: milliseconds (median of
--reps), rows / s, and node visits / s -- the visits counted by the NumPy restatement on a sample of the rows and scaled.

    python tools/classify_time.py [--rows 489480] [--features 96] [--trees 100] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def mean_path_length(forest, X):
    """Mean number of nodes a row visits per tree (leaf included), from the restatement's leaves."""
    from tests import forest_restatement as R
    lv = R.leaves(forest, X)
    size = np.diff(np.r_[forest.tree_offset, forest.n_nodes])
    base = np.repeat(forest.tree_offset, size)
    depth = np.zeros(forest.n_nodes, np.int64)          # children follow their parent in scikit-learn's node order
    for i in np.flatnonzero(forest.left >= 0):
        depth[base[i] + forest.left[i]] = depth[base[i] + forest.right[i]] = depth[i] + 1
    return float(depth[lv].mean() + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=489480)
    ap.add_argument("--features", type=int, default=96)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--train-rows", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "classify_time.py needs a GPU"
    from sklearn.ensemble import RandomForestClassifier
    from obia_amd import _lib
    from obia_amd.classify import Forest, forest_predict, standard_scale

    rs = np.random.RandomState(0)
    centre = rs.normal(0, 0.5, (a.classes, a.features))
    y = rs.randint(0, a.classes, a.train_rows)
    rf = RandomForestClassifier(n_estimators=a.trees, random_state=0).fit(centre[y] + rs.normal(0, 1, (a.train_rows, a.features)), y)
    forest = Forest.from_sklearn(rf)
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn((a.rows, a.features), generator=g, device="cuda", dtype=torch.float64) * 1.1 + 0.3
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)     # kernels on torch's stream: events bracket them

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), r

    t_scale, t_pred = [], []
    for i in range(a.warmup + a.reps):
        ms_s, (X32, _, _) = timed(lambda: standard_scale(table, ctx=ctx))
        ms_p, _ = timed(lambda: forest_predict(forest, X32, ctx=ctx))
        if i >= a.warmup:
            t_scale.append(ms_s)
            t_pred.append(ms_p)
    sample = X32[:: max(1, a.rows // 2000)].cpu().numpy()
    path = mean_path_length(forest, sample)
    ms_s, ms_p = statistics.median(t_scale), statistics.median(t_pred)
    print(json.dumps({
        "workload": f"standard_scale + forest_predict, {a.rows} x {a.features}, {a.trees} trees, {forest.n_nodes} nodes, {a.classes} classes",
        "scale_ms": round(ms_s, 3), "predict_ms": round(ms_p, 3), "scale_all_ms": [round(v, 3) for v in t_scale],
        "predict_all_ms": [round(v, 3) for v in t_pred],
        "rows_per_s": round(a.rows / ((ms_s + ms_p) * 1e-3)),
        "mean_nodes_per_walk": round(path, 2),
        "node_visits_per_s": round(a.rows * a.trees * path / (ms_p * 1e-3)),
        "scale_bytes": a.rows * a.features * (8 * 3 + 4),          # three reads of the float64 table, one float32 write
        "gpu": torch.cuda.get_device_name(0),
    }))


if __name__ == "__main__":
    main()
