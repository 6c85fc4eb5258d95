"""Timing of the seed-table options (obia_amd.seeds: sample_heights, stage1_clusters, reduce_stage1, split_clusters_by_height,
trim_clusters, nms_per_crown; include/obia_seed_table.h) on one GPU, on device-resident tables of n = 10^4, 10^5 and 10^6 seeds: a
grid of 4-unit spacing jittered by +-1.2 units (about the density of tree tops at 0.5 m pixels), heights 2 .. 25, clusters of the seeds
of 3 x 3 grid blocks.  Wall-clock milliseconds around each public function with the device idle before and after: what a caller waits,
the sorts, the gathers and the read-backs of the rounds included.  Warm-up first, then the median of --reps runs.  At n = 10^4 the
restatement of the test suite (tests/seed_table_restatement.py: NumPy on one CPU core) runs stage 1 and the NMS once, for scale; there
is no earlier implementation to compare with.  Prints one JSON line.

    python tools/seed_table_time.py [--sizes 10000,100000,1000000] [--reps 5] [--warmup 2]
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


def make_table(n, rs):
    side = int(np.ceil(np.sqrt(n)))
    gy, gx = np.divmod(np.arange(n), side)
    xs = 431000.0 + 4.0 * gx + rs.uniform(-1.2, 1.2, n)
    ys = 5012000.0 + 4.0 * gy + rs.uniform(-1.2, 1.2, n)
    hs = rs.uniform(2.0, 25.0, n).astype(np.float32)
    cl = ((gy // 3) * (side // 3 + 1) + gx // 3).astype(np.int32)
    order = rs.permutation(n)                                                # table order is not grid order
    return xs[order], ys[order], hs[order], cl[order], side


def timed(fn, reps, warmup):
    ts = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(1e3 * (time.perf_counter() - t0))
    return {"ms": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-at", type=int, default=10000, help="size at which the CPU restatement runs once (0: never)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "seed_table_time.py needs a GPU"
    from obia_amd import seeds as S

    out = {"reps": a.reps, "sizes": {}}
    for n in [int(v) for v in a.sizes.split(",")]:
        rs = np.random.RandomState(n % 9973)
        xs, ys, hs, cl, side = make_table(n, rs)
        chm = torch.as_tensor(rs.uniform(2, 25, (2 * side + 8, 2 * side + 8)).astype(np.float32)).cuda()
        affine = [2.0, 0.0, 0.0, 2.0, 431000.0 - 4.0, 5012000.0 - 4.0]
        dx, dy, dh, dc = (torch.as_tensor(v).cuda() for v in (xs, ys, hs, cl))
        r = {}
        r["stage1_clusters"] = timed(lambda: S.stage1_clusters(dx, dy, dh), a.reps, a.warmup)
        r["stage1_clusters"]["rounds"] = S.stage1_rounds()[0]
        cl1 = S.stage1_clusters(dx, dy, dh)
        r["stage1_clusters"]["pre_clusters"] = int(cl1.max()) + 1
        r["reduce_stage1"] = timed(lambda: S.reduce_stage1(cl1, dh, 1), a.reps, a.warmup)
        r["split_clusters_by_height"] = timed(lambda: S.split_clusters_by_height(dc, dh, 8.0), a.reps, a.warmup)
        r["trim_clusters"] = timed(lambda: S.trim_clusters(dc, dh, 4), a.reps, a.warmup)
        r["nms_per_crown"] = timed(lambda: S.nms_per_crown(dx, dy, dh, dc, 3.0, 0.1), a.reps, a.warmup)
        r["nms_per_crown"]["kept"] = int(S.nms_per_crown(dx, dy, dh, dc, 3.0, 0.1).numel())
        r["sample_heights"] = timed(lambda: S.sample_heights(dx, dy, chm, affine), a.reps, a.warmup)
        if n == a.cpu_at:
            from tests import seed_table_restatement as T
            t0 = time.perf_counter()
            want = T.stage1(xs, ys, hs)
            r["cpu_restatement_stage1_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            t0 = time.perf_counter()
            keep = T.nms(xs, ys, hs, cl, 3.0, 0.1)
            r["cpu_restatement_nms_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            r["equal_to_restatement"] = bool(np.array_equal(cl1.cpu().numpy(), want)
                                             and np.array_equal(S.nms_per_crown(dx, dy, dh, dc, 3.0, 0.1).cpu().numpy(), keep))
        out["sizes"][str(n)] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
