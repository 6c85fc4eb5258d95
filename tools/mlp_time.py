"""Timing of MLP prediction (obia_amd.classify.mlp_predict) on one GPU: standard_scale(dtype=float64) and mlp_predict on a table
of the author's size (489 480 segments) with 96 feature columns, against a network with one hidden layer of 100 units
and 5 classes whose weights are drawn here (no training: the time does not depend on the values).  Device events on the stream the
library's context runs on.  Prints one JSON line: milliseconds (median of --reps), rows / s and float64 GFLOP / s counting one
multiply and one add per weight and row.

    python tools/mlp_time.py [--rows 489480] [--features 96] [--hidden 100] [--classes 5] [--reps 5]
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
    ap.add_argument("--hidden", type=int, nargs="*", default=[100])
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--activation", default="relu")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mlp_time.py needs a GPU"
    from obia_amd import _lib
    from obia_amd.classify import MLP, _mlp_plan, mlp_predict, standard_scale

    rs = np.random.RandomState(0)
    ls = [a.features] + list(a.hidden) + [a.classes]
    mlp = MLP(np.concatenate([rs.normal(0, 1 / np.sqrt(i), i * o) for i, o in zip(ls[:-1], ls[1:])]), rs.normal(0, 0.1, sum(ls[1:])), ls,
              a.activation, "softmax", np.arange(a.classes))
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
        ms_s, (X64, _, _) = timed(lambda: standard_scale(table, ctx=ctx, dtype=np.float64))
        ms_p, _ = timed(lambda: mlp_predict(mlp, X64, ctx=ctx))
        if i >= a.warmup:
            t_scale.append(ms_s)
            t_pred.append(ms_p)
    ms_s, ms_p = statistics.median(t_scale), statistics.median(t_pred)
    flop = 2 * a.rows * sum(i * o for i, o in zip(ls[:-1], ls[1:]))
    rows_per_wg, chunk = _mlp_plan(ls)
    print(json.dumps({
        "workload": f"standard_scale(float64) + mlp_predict, {a.rows} x {a.features}, hidden {list(a.hidden)} {a.activation}, {a.classes} classes",
        "scale_ms": round(ms_s, 3), "predict_ms": round(ms_p, 3), "scale_all_ms": [round(v, 3) for v in t_scale],
        "predict_all_ms": [round(v, 3) for v in t_pred],
        "rows_per_s": round(a.rows / ((ms_s + ms_p) * 1e-3)),
        "predict_gflop_per_s": round(flop / (ms_p * 1e-3) / 1e9, 1),
        "rows_per_workgroup": rows_per_wg, "features_staged_at_a_time": chunk,
        "predict_bytes": a.rows * (a.features * 8 + a.classes * 8 + 4 + 8),      # the table once, proba, pred, margin
        "gpu": torch.cuda.get_device_name(0),
    }))


if __name__ == "__main__":
    main()
