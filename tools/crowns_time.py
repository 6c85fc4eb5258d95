"""Timing of cost allocation (obia_crowns_allocate_dev, include/obia_crowns.h) on one GPU: a device-resident 2048 x 2048 float32 cost
raster, smooth and in [0, 1]; seeds on a jittered 18-pixel grid (about 12.9 k, the density of the benchmark's tiles), one id each;
8-connected, weight 0.5, pixel size 1.  Once unbounded and once with max_dist = 27 pixels.  Device events on the stream the library's
context runs on; the call reads a flag back after every round, so the events bracket the host's round trips too -- that is the time
a caller waits.  Warm-up first, then the median of --reps runs.  Prints one JSON line: milliseconds, the rounds of the distance and
of the label pass, the tiles every round relaxes (all of them) and how many of them changed per round on average.

    python tools/crowns_time.py [--size 2048] [--grid 18] [--reps 7] [--warmup 2]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--grid", type=int, default=18)
    ap.add_argument("--max-dist", type=float, default=27.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "crowns_time.py needs a GPU"
    from obia_amd import _lib

    H = W = a.size
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32),
                            indexing="ij")
    cost = (0.5 + 0.25 * torch.sin(xx / 7.0) * torch.cos(yy / 9.0) + 0.25 * torch.sin((xx + yy) / 23.0)).clamp(0, 1).contiguous()
    del yy, xx
    rs = np.random.RandomState(0)
    gy, gx = np.mgrid[a.grid // 2:H:a.grid, a.grid // 2:W:a.grid]
    rows = np.clip(gy + rs.randint(-a.grid // 3, a.grid // 3 + 1, gy.shape), 0, H - 1).reshape(-1)
    cols = np.clip(gx + rs.randint(-a.grid // 3, a.grid // 3 + 1, gx.shape), 0, W - 1).reshape(-1)
    n = len(rows)
    rc = torch.as_tensor(np.stack([rows, cols], 1).astype(np.int32)).cuda()
    ids = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    dist = torch.empty((H, W), dtype=torch.float64, device="cuda")
    labels = torch.empty((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)          # kernels on torch's stream: events bracket them
    lib = _lib.load()
    tile = _lib.CROWNS_TILE
    tiles = -(-H // tile) * -(-W // tile)

    def run(max_dist):
        _lib.check(lib.obia_crowns_allocate_dev(ctx.handle, cost.data_ptr(), None, H, W, rc.data_ptr(), ids.data_ptr(), n, 0.5, 1.0, 1.0,
                                                math.sqrt(2.0), 8, max_dist, dist.data_ptr(), labels.data_ptr(), None))

    out = {"size": a.size, "seeds": n, "tile": tile, "tiles": tiles, "reps": a.reps, "runs": {}}
    for name, max_dist in (("unbounded", -1.0), (f"max_dist_{a.max_dist:g}", a.max_dist)):
        ts = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run(max_dist)
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        w = (ctypes.c_int64 * 4)()
        _lib.check(lib.obia_crowns_last_work(ctx.handle, w))
        out["runs"][name] = {"ms": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3),
                             "distance_rounds": w[0], "label_rounds": w[1], "tiles_relaxed_per_round": tiles,
                             "distance_tiles_changed_per_round": round(w[2] / w[0], 1), "label_tiles_changed_per_round": round(w[3] / w[1], 1),
                             "labelled_px": int((labels > 0).sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
