"""Timing of the maskSLIC seeding (obia_amd.segmentation.mask_centroids -> obia_mask_centroids_dev) on one GPU, on the shape it exists
for: one 2048 x 2048 tile of the reference's tiler at n_segments = 13 351 (a 2048^2 tile at 0.5 m pixels and crown radius 5: one
segment per 314 pixels), which is 1.3 M k-means points x 13 351 centroids x 5 iterations.  Two masks: all ones, and a blob that
keeps 70 % of the tile.  The timed region is the public call with a device-resident mask (the NumPy picks on the host, the upload of
the picks, the kernels, the read-back of the seeds), host clock, median of --reps after --warmup calls; the picks alone are timed
beside it.  Prints one JSON line.

The reference's routine (scikit-image's `_get_mask_centroids`: kmeans2 + a K x K pdist) takes 220 s per such tile on a CPU (SURVEY
section 6); `--cpu-kmeans K` re-times its k-means step with the local SciPy at a smaller K on this host (it scales as K^2), without a GPU.

Status of the numbers: NOT MEASURED YET on an MI355X.

    python tools/mask_seeds_time.py [--size 2048] [--n 13351] [--reps 3] [--warmup 1] [--cpu-kmeans 0]
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


def masks(size):
    yy, xx = np.mgrid[0:size, 0:size]
    # an ellipse-like blob cut by a straight edge: ~70 % of the tile
    blob = ((yy - 0.5 * size) ** 2 / (0.5 * size) ** 2 + (xx - 0.45 * size) ** 2 / (0.445 * size) ** 2 < 1.0) & (xx + yy > 0.25 * size)
    return {"all_ones": np.ones((size, size), bool), "blob_70pct": blob}


def cpu_kmeans_seconds(mask, K):
    from scipy.cluster.vq import kmeans2
    from obia_amd.segmentation import _mask_seed_picks
    yy, xx = np.nonzero(mask)
    coord = np.stack([np.zeros(len(yy)), yy, xx], 1).astype(np.float64)
    idx, dense = _mask_seed_picks(len(coord), K)
    t0 = time.perf_counter()
    kmeans2(coord if dense is None else coord[dense], coord[idx], iter=5)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--n", type=int, default=13351)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-kmeans", type=int, default=0, help="K for a SciPy kmeans2 timing on this host (0: skip)")
    a = ap.parse_args()
    res = {"size": a.size, "n_segments": a.n, "reference_cpu_s_per_2048_tile": 220.0}
    if a.cpu_kmeans > 0:
        res["scipy_kmeans2_s"] = {"K": a.cpu_kmeans, "seconds": round(cpu_kmeans_seconds(masks(a.size)["all_ones"], a.cpu_kmeans), 2)}
        print(json.dumps(res))
        return
    import torch
    assert torch.cuda.is_available(), "mask_seeds_time.py needs a GPU (or --cpu-kmeans K)"
    from obia_amd.segmentation import _mask_seed_picks, mask_centroids
    res["gpu"] = torch.cuda.get_device_name(0)
    for name, m in masks(a.size).items():
        dm = torch.as_tensor(m).cuda()
        n_valid = int(m.sum())
        t0 = time.perf_counter()
        idx, dense = _mask_seed_picks(n_valid, a.n)
        picks_ms = (time.perf_counter() - t0) * 1e3
        for _ in range(a.warmup):
            mask_centroids(dm, a.n)
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cent, steps = mask_centroids(dm, a.n)
            ms.append((time.perf_counter() - t0) * 1e3)
        pts = n_valid if dense is None else len(dense)
        med = statistics.median(ms)
        res[name] = {"n_valid": n_valid, "valid_fraction": round(n_valid / m.size, 3), "K": len(idx), "points": pts,
                     "call_ms": round(med, 2), "call_all_ms": [round(v, 2) for v in ms], "host_picks_ms": round(picks_ms, 2),
                     "distances_per_s": round(5.0 * pts * len(idx) / ((med - picks_ms) * 1e-3), 0) if med > picks_ms else None,
                     "steps": [float(v) for v in steps]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
