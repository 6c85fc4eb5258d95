"""Timing of mlp_shap (obia_amd.classify, csrc/mlp_shap.hip) on one GPU at the shape of the reference author's notebook cell: 2010
rows of 9 features explained against the same 2010 rows as background, a network of layers (9, 100, 50, 30, 6) with synthetic
weights (tests/mlp_restatement.random_mlp) -- 2010 x 512 x 2010 forward passes.  mlp_predict is timed beside it on 2010 x 512 rows,
the same number of forward passes divided by 2010.  Device events on the stream the library's context runs on.  Prints one JSON
line: seconds (median of --reps), forward passes / s and float64 multiply-adds / s of both.

    python tools/mlp_shap_time.py [--rows 2010] [--background 2010] [--reps 5]
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
    ap.add_argument("--rows", type=int, default=2010)
    ap.add_argument("--background", type=int, default=2010)
    ap.add_argument("--layers", type=int, nargs="+", default=[9, 100, 50, 30, 6])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mlp_shap_time.py needs a GPU"
    from obia_amd import _lib
    from obia_amd.classify import mlp_predict, mlp_shap
    from tests import mlp_restatement as mr

    rs = np.random.RandomState(0)
    mlp = mr.mlp_of(mr.random_mlp(rs, a.layers))
    F, K = a.layers[0], a.layers[-1]
    M = 1 << F
    table = torch.as_tensor(rs.normal(0, 1, (max(a.rows, a.background), F)), device="cuda")
    X, bg = table[:a.rows].contiguous(), table[:a.background].contiguous()
    flat = torch.as_tensor(rs.normal(0, 1, (a.rows * M, F)), device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)     # kernels on torch's stream: events bracket them

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, r

    t_shap, t_pred = [], []
    gap = 0.0
    for i in range(a.warmup + a.reps):
        s_p, _ = timed(lambda: mlp_predict(mlp, flat, ctx=ctx))
        s_s, (phi, base) = timed(lambda: mlp_shap(mlp, X, bg, ctx=ctx))
        if i == 0:                                  # additivity of what was timed, on the device
            _, _, proba = mlp_predict(mlp, X, ctx=ctx)
            gap = float((phi.sum(1) + base[None, :] - proba).abs().max())
        if i >= a.warmup:
            t_shap.append(s_s)
            t_pred.append(s_p)
    s_s, s_p = statistics.median(t_shap), statistics.median(t_pred)
    macs = sum(u * v for u, v in zip(a.layers[:-1], a.layers[1:]))
    passes = a.rows * M * a.background
    print(json.dumps({
        "workload": f"mlp_shap, {a.rows} rows x {F} features against {a.background} background rows, layers {a.layers}, {M} coalitions, "
                    f"{K} classes",
        "shap_s": round(s_s, 3), "shap_all_s": [round(v, 3) for v in t_shap],
        "forward_passes": passes, "forward_passes_per_s": round(passes / s_s), "multiply_adds_per_s": round(passes * macs / s_s),
        "predict_rows": a.rows * M, "predict_s": round(s_p, 6), "predict_forward_passes_per_s": round(a.rows * M / s_p),
        "predict_multiply_adds_per_s": round(a.rows * M * macs / s_p),
        "max_abs_sum_phi_plus_base_minus_proba": gap,
        "gpu": torch.cuda.get_device_name(0),
    }))


if __name__ == "__main__":
    main()
