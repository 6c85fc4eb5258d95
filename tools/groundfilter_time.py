"""Timing of the ground filter (obia_amd.pointcloud; include/obia_groundfilter.h) on one GPU, on device-resident inputs:

  * FILTERS: a grey opening (4 line passes through obia_morph_filter_dev, buffers allocated outside the timing) of a --size x --size
    float32 plane with a fifth of its cells empty at radii 1, 4, 16, 64: milliseconds and GB/s against the compulsory 8 bytes per
    cell and line pass;
  * THRESHOLD: obia_gf_threshold_dev with the default schedule (radii 1, 2, 4, 8, 16: 20 line passes) on the same plane;
  * CELL MINIMUM and CLASSIFICATION of --points points over that grid, once in SCAN order -- bands of 64 rows swept along their
    length, so that neighbours in the array are neighbours on the ground -- and once fully SHUFFLED (the two orders of
    tools/points_time.py): points per second and GB/s on the compulsory 24 bytes per point (x, y, z) of the minimum and 29 of the
    classification (plus the threshold gather and the flag);
  * beside each what a user can compose from torch today: ``-max_pool2d(-x, 2r + 1, stride=1, padding=r)`` followed by ``max_pool2d``
    on the same plane with infinities for the empties (checked equal to the kernels' opening), and the pixel arithmetic plus
    ``scatter_reduce_(..., "amin")`` for the cell minimum (checked equal), with the ratios.

Wall-clock milliseconds around each call with the device idle before and after.  The first run is reported on its own, then the
median of --reps (the torch compositions at radius 16 and 64 run --slow-reps times: their cost grows with the window's area).  There
is no earlier implementation to compare with.  Prints one JSON line.

    python tools/groundfilter_time.py [--size 8192] [--points 200000000] [--reps 5]
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


def timed(fn, reps, fresh=None):
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


def same(a, b):
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--points", type=int, default=200_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow-reps", type=int, default=2)
    ap.add_argument("--radii", type=int, nargs="*", default=[1, 4, 16, 64])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "groundfilter_time.py needs a GPU"
    import torch.nn.functional as F
    from obia_amd import _lib
    from obia_amd.consumers import invert_affine
    from obia_amd.pointcloud import pmf_schedule

    S, n = a.size, a.points
    cells = S * S
    lib, ctx = _lib.load(), _lib.default_context(0)
    h = ctx.handle
    g = torch.Generator(device="cuda").manual_seed(7)
    plane = torch.rand((S, S), generator=g, device="cuda") * 30.0 + 100.0
    plane[torch.rand((S, S), generator=g, device="cuda") < 0.2] = float("nan")
    tmp, mid, dst = (torch.empty_like(plane) for _ in range(3))
    out = {"size": S, "cells": cells, "points": n, "reps": a.reps, "slow_reps": a.slow_reps, "filters": {}}

    def opening(r):
        _lib.check(lib.obia_morph_filter_dev(h, plane.data_ptr(), S, S, r, 0, tmp.data_ptr(), mid.data_ptr()))
        _lib.check(lib.obia_morph_filter_dev(h, mid.data_ptr(), S, S, r, 1, tmp.data_ptr(), dst.data_ptr()))

    def composed(r):
        inf = float("inf")
        x = torch.where(torch.isnan(plane), inf, plane)[None, None]
        e = -F.max_pool2d(-x, 2 * r + 1, stride=1, padding=r)
        d = F.max_pool2d(torch.where(e == inf, -inf, e), 2 * r + 1, stride=1, padding=r)
        return torch.where(d == -inf, float("nan"), d)[0, 0]

    for r in a.radii:
        t = timed(lambda: opening(r), a.reps)
        t["GBps_of_8B_per_cell_and_pass"] = round(4 * 8 * cells / (t["ms"] * 1e-3) / 1e9, 1)
        assert same(composed(r), dst), f"the composition and the kernels disagree at radius {r}"
        c = timed(lambda: composed(r), a.reps if r < 16 else a.slow_reps)
        out["filters"][f"r{r}"] = {"opening": t, "torch_composition": c, "speedup_over_composition": round(c["ms"] / t["ms"], 2)}
        torch.cuda.empty_cache()

    radii, dh = pmf_schedule()
    K = len(radii)
    surface, thresh = torch.empty_like(plane), torch.empty_like(plane)
    R, D = (ctypes.c_int32 * K)(*radii), (ctypes.c_double * K)(*dh)
    t = timed(lambda: _lib.check(lib.obia_gf_threshold_dev(h, plane.data_ptr(), S, S, R, D, K, tmp.data_ptr(), mid.data_ptr(), surface.data_ptr(),
                                                           thresh.data_ptr())), a.reps)
    t["line_passes"] = 4 * K
    t["GBps_of_8B_per_cell_and_pass"] = round(4 * K * 8 * cells / (t["ms"] * 1e-3) / 1e9, 1)
    out["threshold_default_schedule"] = t
    del tmp, mid, dst, surface
    torch.cuda.empty_cache()

    # the cloud over the grid: cells of 1 m, north-up
    affine = [1.0, 0.0, 0.0, -1.0, 1000.0, 2000.0 + S]
    inv6 = invert_affine(affine)
    inv = (ctypes.c_double * 6)(*inv6)
    col = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * S
    row = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * S
    z = (torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 30.0 + 100.0)
    scan = torch.sort(torch.floor(row / 64.0) * S + col).indices
    x, y = affine[0] * col + affine[4], affine[3] * row + affine[5]
    del col, row
    for name, order in (("scan", scan), ("shuffled", None)):
        X, Y, Z = (x, y, z) if order is None else (x[order], y[order], z[order])
        r = {}
        keys = torch.zeros((S, S), dtype=torch.int32, device="cuda")

        def fresh():
            keys.zero_()
            return keys

        def cell_min(k):
            _lib.check(lib.obia_gf_cell_min_dev(h, X.data_ptr(), Y.data_ptr(), Z.data_ptr(), n, inv, S, S, k.data_ptr()))

        t = timed(cell_min, a.reps, fresh)
        t["Mpoints_per_s"], t["GBps_of_24B_per_point"] = round(n / (t["ms"] * 1e-3) / 1e6, 1), round(24 * n / (t["ms"] * 1e-3) / 1e9, 1)
        r["cell_min"] = t
        zmin = torch.empty((S, S), dtype=torch.float32, device="cuda")
        r["cell_min_finish"] = timed(lambda: _lib.check(lib.obia_gf_cell_min_finish_dev(h, keys.data_ptr(), S, S, zmin.data_ptr())), a.reps)

        def composed_min():
            c = torch.floor(inv6[0] * X + inv6[1] * Y + inv6[4])
            w = torch.floor(inv6[2] * X + inv6[3] * Y + inv6[5])
            ok = (c >= 0) & (c < S) & (w >= 0) & (w < S) & torch.isfinite(Z)
            px = (w[ok].to(torch.int64) * S + c[ok].to(torch.int64))
            m = torch.full((cells,), float("inf"), dtype=torch.float32, device="cuda")
            m.scatter_reduce_(0, px, Z[ok].to(torch.float32), "amin", include_self=True)
            return torch.where(m == float("inf"), float("nan"), m).view(S, S)

        assert same(composed_min(), zmin), "the composition and the kernel disagree on the cell minimum"
        c = timed(composed_min, a.reps)
        r["torch_composition_cell_min"] = c
        r["cell_min_speedup_over_composition"] = round(c["ms"] / (t["ms"] + r["cell_min_finish"]["ms"]), 2)
        torch.cuda.empty_cache()
        flags = torch.empty(n, dtype=torch.uint8, device="cuda")
        counters = torch.zeros(4, dtype=torch.int64, device="cuda")
        t = timed(lambda: _lib.check(lib.obia_gf_classify_dev(h, X.data_ptr(), Y.data_ptr(), Z.data_ptr(), n, inv, thresh.data_ptr(), S, S,
                                                              flags.data_ptr(), counters.data_ptr())), a.reps)
        t["Mpoints_per_s"], t["GBps_of_29B_per_point"] = round(n / (t["ms"] * 1e-3) / 1e6, 1), round(29 * n / (t["ms"] * 1e-3) / 1e9, 1)
        r["classify"] = t
        r["ground_share"] = round(float(flags.to(torch.float32).mean()), 4)
        out[name] = r
        del X, Y, Z, keys, zmin, flags
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
