"""Timing of the cost surface (obia_amd.cost) on one GPU: make_cost_surface end to end and every stage, with device events
on the stream the library's context runs on.  A seeded 16384^2 x 8 WorldView-3-shaped raster (the bench raster's shape), a
CHM with NaN patches and a label raster are built on the device.  Prints one JSON line: milliseconds (median of --reps),
the bytes each stage must move (from shapes), the fraction of 6.3 TB/s (measured achievable HBM bandwidth) and of 8 TB/s
(spec) those bytes imply, and the CPU restatement's time at 2048^2 for scale.

    python tools/cost_time.py [--size 16384] [--reps 5] [--cpu-size 2048]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.3e12, 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-size", type=int, default=2048)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cost_time.py needs a GPU"
    from obia_amd import _lib, cost

    H = W = a.size
    P = H * W
    g = torch.Generator(device="cuda").manual_seed(0)
    wv3 = torch.rand((H, W, 8), generator=g, device="cuda") * 1000
    chm = torch.rand((H, W), generator=g, device="cuda") * 30
    chm[torch.rand((H, W), generator=g, device="cuda") < 1e-3] = float("nan")
    for k in range(16):
        y, x = (k * 977) % (H - 64), (k * 1553) % (W - 64)
        chm[y:y + 64, x:x + 64] = float("nan")
    ys = torch.arange(H, device="cuda", dtype=torch.int32)[:, None] // 40
    xs = torch.arange(W, device="cuda", dtype=torch.int32)[None, :] // 40
    lab = (ys * 4096 + xs).contiguous()
    torch.cuda.synchronize()

    stream = torch.cuda.current_stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)     # kernels on torch's stream: events bracket them
    lib = _lib.load()
    w = (0.4, 0.3, 0.2, 0.1)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), r

    img = wv3.contiguous()
    pan = torch.empty((H, W), dtype=torch.float32, device="cuda")
    gap = torch.empty_like(pan)

    def stages():
        t = {}
        t["bands"], _ = timed(lambda: _lib.check(lib.obia_cost_bands_f32_dev(ctx.handle, img.data_ptr(), P, pan.data_ptr(), gap.data_ptr())))
        t["sobel"], grad = timed(lambda: cost._sobel_dev(lib, ctx, chm))
        t["select_pan"], lc = timed(lambda: cost._select(lib, ctx, pan))
        t["entropy"], tex = timed(lambda: cost._entropy_dev(lib, ctx, pan, lc[0], lc[1]))
        t["select_grad"], lg = timed(lambda: cost._select(lib, ctx, grad))
        t["select_gap"], lp = timed(lambda: cost._select(lib, ctx, gap))
        t["select_tex"], lt = timed(lambda: cost._select(lib, ctx, tex))
        t["edge_count"], le = timed(lambda: cost._edge_lohi(lib, ctx, lab, H, W))
        out = torch.empty((H, W), dtype=torch.float32, device="cuda")
        import ctypes
        d4 = ctypes.c_double * 4
        lohi = [lg[:2], lp[:2], lt[:2], le]
        t["combine"], _ = timed(lambda: _lib.check(lib.obia_cost_combine_dev(
            ctx.handle, grad.data_ptr(), gap.data_ptr(), tex.data_ptr(), lab.data_ptr(), H, W, d4(*[p[0] for p in lohi]),
            d4(*[p[1] for p in lohi]), d4(*w), out.data_ptr())))
        return t

    for _ in range(a.warmup):
        cost.make_cost_surface(wv3, chm, slic=lab, weights=w, ctx=ctx)
        stages()
    e2e, per = [], {}
    for _ in range(a.reps):
        ms, _ = timed(lambda: cost.make_cost_surface(wv3, chm, slic=lab, weights=w, ctx=ctx))
        e2e.append(ms)
        for k, v in stages().items():
            per.setdefault(k, []).append(v)
    # compulsory bytes per stage: one read of every input and one write of every output; a select pass reads its plane
    # once, and the selects are charged the most passes they can run (float32 3, float64 6: fewer when a digit group is
    # constant)
    by = {"bands": 40 * P, "sobel": 8 * P, "select_pan": 3 * 4 * P, "entropy": 12 * P, "select_grad": 3 * 4 * P,
          "select_gap": 3 * 4 * P, "select_tex": 6 * 8 * P, "edge_count": 4 * P, "combine": 24 * P}
    stage_ms = {k: statistics.median(v) for k, v in per.items()}
    total_bytes = sum(by.values())
    e2e_ms = statistics.median(e2e)
    res = {
        "workload": f"make_cost_surface {H}x{W}x8 + CHM + labels",
        "end_to_end_ms": round(e2e_ms, 3),
        "end_to_end_all_ms": [round(v, 3) for v in e2e],
        "stage_ms": {k: round(v, 3) for k, v in stage_ms.items()},
        "stage_bytes": by,
        "stage_frac_of_6.3TBs": {k: round(by[k] / (stage_ms[k] * 1e-3) / HBM_MEASURED, 3) for k in by},
        "stage_frac_of_8TBs": {k: round(by[k] / (stage_ms[k] * 1e-3) / HBM_SPEC, 3) for k in by},
        "bytes_total": total_bytes,
        "bytes_per_px": total_bytes / P,
        "end_to_end_frac_of_6.3TBs": round(total_bytes / (e2e_ms * 1e-3) / HBM_MEASURED, 3),
        "end_to_end_frac_of_8TBs": round(total_bytes / (e2e_ms * 1e-3) / HBM_SPEC, 3),
        "gpu": torch.cuda.get_device_name(0),
    }
    if a.cpu_size > 0:
        from tests import cost_restatement as R
        n = a.cpu_size
        rs = np.random.RandomState(0)
        wv = rs.uniform(0, 1000, (n, n, 8)).astype(np.float32)
        ch = rs.uniform(0, 30, (n, n)).astype(np.float32)
        lb = ((np.arange(n)[:, None] // 40) * 4096 + np.arange(n)[None] // 40).astype(np.int32)
        t0 = time.perf_counter()
        R.make_cost_surface(wv, ch, lb, w)
        res["cpu_restatement_s_at"] = {"size": n, "s": round(time.perf_counter() - t0, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
