"""Timing of height above ground (obia_amd.pointcloud.GroundIndex; include/obia_ground.h) on one GPU, on device-resident inputs:

  * --ground ground points uniform over the extent of a --size x --size raster of 0.5 m pixels (16384: 8192 m a side; 2 * 10^7
    points: 0.3 per square metre) on a smooth terrain, and --points queries uniform over the same extent;
  * the index build (``GroundIndex(ground)``: cells, a stable sort, the gathers, the start table) timed apart from the queries;
  * the queries once in GROUND order -- sorted by the cell of the index, so that neighbours in the array are neighbours on the
    ground and the lanes of a wave read the same runs -- once in STRIPE order -- sorted by row band of 32 m, shuffled inside a band,
    roughly what a flight line delivers -- and once fully SHUFFLED (as generated);
  * per order ``GroundIndex.height_above_ground`` with ``count`` 1 and 3: queries per second, GB/s on the compulsory 28 bytes per
    query (x, y, z read, hag written; the call also writes the 8-byte ground height) and that rate as a fraction of --hbm-gbps.

Wall-clock milliseconds around each call with the device idle before and after.  The first run is reported on its own, then the
median of --reps.  There is no earlier implementation to compare with.  Prints one JSON line.

    python tools/ground_time.py [--size 16384] [--ground 20000000] [--points 200000000] [--reps 5] [--hbm-gbps 8000]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

BYTES_PER_QUERY = 28


def timed(fn, reps):
    ts = []
    for _ in range(1 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"first_ms": round(ts[0], 3), "ms": round(statistics.median(ts[1:]), 3), "ms_min": round(min(ts[1:]), 3),
            "ms_max": round(max(ts[1:]), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--ground", type=int, default=20_000_000)
    ap.add_argument("--points", type=int, default=200_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-gbps", type=float, default=8000.0)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ground_time.py needs a GPU"
    from obia_amd.pointcloud import GroundIndex

    extent, ng, n = 0.5 * a.size, a.ground, a.points
    g = torch.Generator(device="cuda").manual_seed(11)

    def terrain(x, y):
        return 300.0 + 40.0 * torch.sin(x / 700.0) * torch.cos(y / 900.0) + 0.01 * x

    gx = 1000.0 + torch.rand(ng, generator=g, device="cuda", dtype=torch.float64) * extent
    gy = 2000.0 + torch.rand(ng, generator=g, device="cuda", dtype=torch.float64) * extent
    ground = {"X": gx, "Y": gy, "Z": terrain(gx, gy)}
    out = {"size": a.size, "extent_m": extent, "ground": ng, "points": n, "reps": a.reps, "bytes_per_query": BYTES_PER_QUERY,
           "hbm_gbps": a.hbm_gbps}
    made = []
    out["index_build"] = timed(lambda: made.__setitem__(slice(None), [GroundIndex(ground)]), a.reps)
    idx = made[0]
    out["index"] = {"side": idx.side, "shape": list(idx.shape), "cells": idx.shape[0] * idx.shape[1], "n_ground": idx.n_ground}

    x = 1000.0 + torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * extent
    y = 2000.0 + torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * extent
    z = terrain(x, y) + torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 30.0
    cell = torch.floor(y / idx.side) * (idx.shape[1] + 2.0) + torch.floor(x / idx.side)
    orders = (("ground", torch.sort(cell).indices),
              ("stripe", torch.sort(torch.floor(y / 32.0) + torch.rand(n, generator=g, device="cuda", dtype=torch.float64)).indices),
              ("shuffled", None))
    del cell
    for name, order in orders:
        cloud = {"X": x, "Y": y, "Z": z} if order is None else {"X": x[order], "Y": y[order], "Z": z[order]}
        r = {}
        for count in (1, 3):
            t = timed(lambda: idx.height_above_ground(cloud, count=count), a.reps)
            t["Mqueries_per_s"] = round(n / (t["ms"] * 1e-3) / 1e6, 1)
            t["GBps"] = round(BYTES_PER_QUERY * n / (t["ms"] * 1e-3) / 1e9, 1)
            t["fraction_of_hbm_peak"] = round(t["GBps"] / a.hbm_gbps, 4)
            r[f"count_{count}"] = t
        out[name] = r
        del cloud
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
