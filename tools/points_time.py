"""Timing of the point-cloud leg (obia_amd.pointcloud; include/obia_points.h) on one GPU, on device-resident inputs:

  * a --size x --size label raster of square segments of --segment pixels a side (16384 and 16: 1 048 576 segments) and --points
    points with uint16 intensities, uniform over the raster, gamma heights, dz = 1, 41 height bins;
  * the cloud once in STRIPE order -- sorted by row band of 64 pixels, shuffled inside a band, roughly what a flight line delivers --
    once fully SHUFFLED, and once in SCAN order -- the same bands swept along their length (sorted by band, then by column), so that
    neighbours in the array are neighbours on the ground, which is what the LDS tables of the join are for;
  * per order: ``PointRasters.add``, ``SegmentPoints.add`` (points per second, and GB/s on the compulsory 26 bytes per point: 22 read
    plus the 4-byte label gather; the rasters pass reads 20) and ``SegmentPoints.columns``;
  * beside it what a user could compose before: ``obia_sample_labels_i32_dev`` plus ``torch.bincount`` for the profile alone (no top,
    no intensity sums, no counters), and its ratio to ``SegmentPoints.add``.

Wall-clock milliseconds around each call with the device idle before and after.  The first run is reported on its own, then the
median of --reps.  There is no earlier implementation to compare with.  Prints one JSON line.

    python tools/points_time.py [--size 16384] [--segment 16] [--points 200000000] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DZ, ZMAX = 1.0, 40.0


def timed(fn, reps, fresh=None):
    """``fresh``: makes the argument of every call outside its timing -- an accumulator with empty state, so that no call profits from
    the maxima the call before left behind (a maximum that stands costs a load, one that rises an atomic)"""
    ts = []
    for _ in range(1 + reps):
        arg = () if fresh is None else (fresh(),)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(*arg)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"first_ms": round(ts[0], 3), "ms": round(statistics.median(ts[1:]), 3), "ms_min": round(min(ts[1:]), 3),
            "ms_max": round(max(ts[1:]), 3)}


def rate(t, n, bytes_per_point):
    t["Mpoints_per_s"] = round(n / (t["ms"] * 1e-3) / 1e6, 1)
    t["GBps"] = round(bytes_per_point * n / (t["ms"] * 1e-3) / 1e9, 1)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--segment", type=int, default=16)
    ap.add_argument("--points", type=int, default=200_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "points_time.py needs a GPU"
    from obia_amd import _lib
    from obia_amd.consumers import invert_affine
    from obia_amd.pointcloud import PointRasters, SegmentPoints

    S, seg, n = a.size, a.segment, a.points
    per_row = -(-S // seg)
    idx = torch.arange(S, device="cuda", dtype=torch.int32) // seg
    labels = (idx[:, None] * per_row + idx[None, :] + 1).contiguous()
    n_labels = per_row * per_row
    affine = [0.5, 0.0, 0.0, -0.5, 1000.0, 2000.0 + 0.5 * S]
    g = torch.Generator(device="cuda").manual_seed(7)
    col = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * S
    row = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * S
    z = (torch.rand(n, generator=g, device="cuda") * torch.rand(n, generator=g, device="cuda") * 45.0).to(torch.float32)      # a few above z_max
    inten = torch.randint(-32768, 32768, (n,), generator=g, device="cuda", dtype=torch.int16)          # the bits of uint16 intensities
    stripe = torch.sort(torch.floor(row / 64.0) + torch.rand(n, generator=g, device="cuda", dtype=torch.float64)).indices
    scan = torch.sort(torch.floor(row / 64.0) * S + col).indices
    x, y = affine[0] * col + affine[4], affine[3] * row + affine[5]
    del col, row
    out = {"size": S, "segments": n_labels, "points": n, "nz": int(ZMAX // DZ) + 1, "reps": a.reps}
    lib, ctx = _lib.load(), _lib.default_context(0)
    inv = (ctypes.c_double * 6)(*invert_affine(affine))

    for name, order in (("stripe", stripe), ("shuffled", None), ("scan", scan)):
        if order is None:
            cloud = {"X": x, "Y": y, "HeightAboveGround": z, "Intensity": inten.view(torch.uint16)}    # generated in random order
        else:
            cloud = {"X": x[order], "Y": y[order], "HeightAboveGround": z[order], "Intensity": inten[order].view(torch.uint16)}
        r = {}
        made = []

        def fresh_rasters():
            made[:] = [PointRasters((S, S), affine).add({k: v[:0] for k, v in cloud.items()})]         # the planes allocated and zeroed
            return made[0]

        def fresh_segments():
            made[:] = [SegmentPoints(labels, affine, DZ, ZMAX, n_labels=n_labels)]
            return made[0]

        r["rasters_add"] = rate(timed(lambda acc: acc.add(cloud), a.reps, fresh_rasters), n, 20)
        pr = made[0]
        r["rasters_result"] = timed(lambda: pr.result(), a.reps)
        del pr
        r["segments_add"] = rate(timed(lambda acc: acc.add(cloud), a.reps, fresh_segments), n, 26)
        sp = made[0]
        del made[:]
        r["counters"] = sp.counters()
        r["columns"] = timed(lambda: sp.columns(), a.reps)
        nz = sp.nz

        xy = torch.stack([cloud["X"], cloud["Y"]], 1).contiguous()
        zz = cloud["HeightAboveGround"]

        def composed():
            lab = torch.empty(n, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            _lib.check(lib.obia_sample_labels_i32_dev(ctx.handle, labels.data_ptr(), S, S, inv, xy.data_ptr(), n, 0, lab.data_ptr()))
            j = torch.floor(zz.to(torch.float64) / DZ)
            ok = (lab >= 1) & torch.isfinite(zz) & (zz >= 0) & (j < nz)
            key = (lab[ok].to(torch.int64) - 1) * nz + j[ok].to(torch.int64)
            return torch.bincount(key, minlength=n_labels * nz)

        assert torch.equal(composed().view(n_labels, nz), sp.profile()), "the composition and the kernel disagree"
        del sp
        r["torch_composition_profile_only"] = rate(timed(composed, a.reps), n, 26)
        r["segments_add_speedup_over_composition"] = round(r["torch_composition_profile_only"]["ms"] / r["segments_add"]["ms"], 2)
        del xy, zz, cloud
        torch.cuda.empty_cache()
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
