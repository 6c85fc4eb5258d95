"""Timing of the box leg (obia_amd.boxes; include/obia_boxes.h) on one GPU, on device-resident inputs:

  * ``assign_boxes`` for a --size x --size label raster of square segments of --segment pixels a side (16384 and 16: 1 048 576
    segments) and --boxes boxes with sides uniform in 10 .. 40 pixels at random fractional positions;
  * the ABI call behind it alone (``obia_boxes_assign_dev``, ``n_labels`` given), and from it the overlap kernel's rate against the
    bytes of its footprints: the call walks every footprint twice (the maximum, then the lowest box that reaches it), 4 bytes per
    footprint pixel, so  rate >= 2 x 4 B x footprint pixels / call time  -- a lower bound, the call also checks the boxes, fills two
    tables and reads three flags back;
  * ``box_overlaps`` (count, prefix sum, write, sort) on the same input;
  * ``box_nms`` for --nms boxes: a quarter as many trees, each seen four times with a jitter of up to a pixel, as the overlapping
    tiles of ``tile_and_process`` deliver them, scores random.

Wall-clock milliseconds around each call with the device idle before and after.  The first run is reported on its own (it pays the
arena's allocations), then the median of --reps.  There is no earlier implementation to compare with.  Prints one JSON line.

    python tools/boxes_time.py [--size 16384] [--segment 16] [--boxes 100000] [--nms 400000] [--reps 5]
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
    ap.add_argument("--segment", type=int, default=16)
    ap.add_argument("--boxes", type=int, default=100000)
    ap.add_argument("--nms", type=int, default=400000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "boxes_time.py needs a GPU"
    from obia_amd import _lib, boxes as B

    S, seg = a.size, a.segment
    per_row = -(-S // seg)
    idx = torch.arange(S, device="cuda", dtype=torch.int32) // seg
    labels = (idx[:, None] * per_row + idx[None, :] + 1).contiguous()
    n_labels = per_row * per_row
    rs = np.random.RandomState(5)
    xy = rs.uniform(0, S - 40, (a.boxes, 2))
    px = torch.as_tensor(np.concatenate([xy, xy + rs.uniform(10, 40, (a.boxes, 2))], 1)).cuda()
    foot = ((torch.floor(px[:, 2]) - torch.ceil(px[:, 0]) + 2) * (torch.floor(px[:, 3]) - torch.ceil(px[:, 1]) + 2)).sum().item()
    out = {"size": S, "segments": n_labels, "boxes": a.boxes, "footprint_pixels": int(foot), "reps": a.reps}

    out["assign_boxes"] = timed(lambda: B.assign_boxes(labels, None, px, n_labels, pixel=True), a.reps)
    lib, ctx = _lib.load(), _lib.default_context(0)
    assigned = torch.empty(n_labels + 1, dtype=torch.int32, device="cuda")
    area = torch.empty(n_labels + 1, dtype=torch.float64, device="cuda")
    out["assign_call"] = timed(lambda: _lib.check(lib.obia_boxes_assign_dev(ctx.handle, labels.data_ptr(), S, S, px.data_ptr(), a.boxes, n_labels,
                                                                            assigned.data_ptr(), area.data_ptr())), a.reps)
    out["assign_call"]["footprint_GBps_lower_bound"] = round(2 * 4 * foot / (out["assign_call"]["ms"] * 1e-3) / 1e9, 1)
    out["assigned_segments"] = int((assigned >= 0).sum())
    out["box_overlaps"] = timed(lambda: B.box_overlaps(labels, px, n_labels), a.reps)
    out["box_overlaps"]["pairs"] = int(B.box_overlaps(labels, px, n_labels)["box"].numel())
    out["dissolve_by_box"] = timed(lambda: B.dissolve_by_box(labels, assigned), a.reps)

    trees = max(1, a.nms // 4)
    txy = rs.uniform(0, S - 40, (trees, 2))
    tb = np.concatenate([txy, txy + rs.uniform(10, 40, (trees, 2))], 1)
    nb = np.repeat(tb, 4, 0)[:a.nms] + rs.uniform(-1, 1, (min(a.nms, 4 * trees), 4))
    nb[:, 2:] = np.maximum(nb[:, 2:], nb[:, :2])
    dnb, dsc = torch.as_tensor(nb).cuda(), torch.as_tensor(rs.uniform(0, 1, len(nb))).cuda()
    out["box_nms"] = timed(lambda: B.box_nms(dnb, dsc, 0.15), a.reps)
    out["box_nms"].update(n=len(nb), kept=int(B.box_nms(dnb, dsc, 0.15)[1].numel()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
