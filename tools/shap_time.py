"""Timing of forest_shap (obia_amd.classify, csrc/shap.hip) on one GPU: a table of the author's size (489 480 segments)
with 96 feature columns against a forest of 100 trees grown here on synthetic data (scikit-learn, host) -- the forest and the
table of tools/classify_time.py, and forest_predict timed on them for comparison.  Device events on the stream the library's
context runs on.  Prints one JSON line: milliseconds (median of --reps), rows / s and (row, root-to-leaf path) pairs / s.

The output is rows x features x classes x 8 bytes; --chunk rows are explained per call (the default keeps it at 0.5 GB) and the
times of the chunks are added.

    python tools/shap_time.py [--rows 489480] [--features 96] [--trees 100] [--reps 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=489480)
    ap.add_argument("--features", type=int, default=96)
    ap.add_argument("--classes", type=int, default=6)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--train-rows", type=int, default=600)
    ap.add_argument("--chunk", type=int, default=122370)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "shap_time.py needs a GPU"
    from sklearn.ensemble import RandomForestClassifier
    from obia_amd import _lib
    from obia_amd.classify import Forest, forest_predict, forest_shap, standard_scale

    rs = np.random.RandomState(0)
    centre = rs.normal(0, 0.5, (a.classes, a.features))
    y = rs.randint(0, a.classes, a.train_rows)
    rf = RandomForestClassifier(n_estimators=a.trees, random_state=0).fit(centre[y] + rs.normal(0, 1, (a.train_rows, a.features)), y)
    forest = Forest.from_sklearn(rf)
    n_paths = int((forest.left < 0).sum())
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn((a.rows, a.features), generator=g, device="cuda", dtype=torch.float64) * 1.1 + 0.3
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)     # kernels on torch's stream: events bracket them
    X32, _, _ = standard_scale(table, ctx=ctx)
    del table

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), r

    t_shap, t_pred = [], []
    worst = 0.0
    for i in range(a.warmup + a.reps):
        ms_p, (_, _, proba) = timed(lambda: forest_predict(forest, X32, ctx=ctx))
        ms = 0.0
        for r0 in range(0, a.rows, a.chunk):
            part, (phi, base) = timed(lambda: forest_shap(forest, X32[r0:r0 + a.chunk], ctx=ctx))
            ms += part
            if i == 0:                              # additivity of what was timed, on the device
                worst = max(worst, float((phi.sum(1) + base[None, :] - proba[r0:r0 + a.chunk]).abs().max()))
            del phi
        if i >= a.warmup:
            t_shap.append(ms)
            t_pred.append(ms_p)
    ms_s, ms_p = statistics.median(t_shap), statistics.median(t_pred)
    print(json.dumps({
        "workload": f"forest_shap, {a.rows} x {a.features}, {a.trees} trees, {forest.n_nodes} nodes, {n_paths} paths, {a.classes} classes, "
                    f"{a.chunk} rows per call",
        "shap_ms": round(ms_s, 1), "shap_all_ms": [round(v, 1) for v in t_shap],
        "predict_ms": round(ms_p, 3),
        "rows_per_s": round(a.rows / (ms_s * 1e-3)),
        "row_path_pairs_per_s": round(a.rows * n_paths / (ms_s * 1e-3)),
        "max_abs_sum_phi_plus_base_minus_proba": worst,
        "output_bytes": a.rows * a.features * a.classes * 8,
        "gpu": torch.cuda.get_device_name(0),
    }))


if __name__ == "__main__":
    main()
