"""Timing of polygons -> label raster (obia_amd.polygons.rasterize) on one GPU, on the workload it exists for: the bench raster
(BASELINE configs[2]: 16384^2 x 8, tile 2048, overlap 64) goes through the tiler, its label raster through ``polygonize``, and the
rings come back through the rasteriser.  The rings are device-resident and already in pixel coordinates; the timed region is
the library call alone (obia_rasterize_polygons_dev, which ends in a stream synchronisation), host clock, median of --reps after
--warmup calls on a device that the tiler and the polygoniser have already warmed.  Prints one JSON line: milliseconds of the
rasterisation, shape / ring / vertex counts, how many shapes took which regime, GB/s on the bytes the pass must move (4 B per
pixel written + 16 B per vertex read), the time of ``polygonize`` on the same label raster (device passes alone, and with the
host grouping) and whether the round trip gave the label raster back.  A second leg times the large-shape regime alone: a few
stars of --big-vertices vertices each with bounding boxes of ~10^6 pixels.

    python tools/rasterize_time.py [--size 16384] [--reps 7] [--warmup 2] [--big-vertices 20000]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big-vertices", type=int, default=20000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rasterize_time.py needs a GPU"
    import bench
    from obia_amd import _lib
    from obia_amd.polygons import polygonize, rasterize, rasterize_info
    from obia_amd.tiling import create_tiled_segments
    lib = _lib.load()
    c = _lib.default_context(0)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), [round(v, 3) for v in ms]

    def raster_call(xy, off, owner, vals, H, W, out):
        def call():
            _lib.check(lib.obia_rasterize_polygons_dev(c.handle, xy.data_ptr(), off.data_ptr(), owner.numel(), owner.data_ptr(),
                                                       vals.data_ptr(), vals.numel(), H, W, 0, out.data_ptr()))
        return call

    res = {"gpu": torch.cuda.get_device_name(0), "limits": {k: v for k, v in rasterize_info().items() if k.startswith("max")}}
    H = W = a.size
    img = bench.synth_raster(H, W, 8, seed=0, device=torch.device("cuda", 0), row0=0)
    mask = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    lab, n = create_tiled_segments(img, input_mask=mask, tile_size=2048, buffer=64, crown_radius=5, pixel_size=(0.5, 0.5),
                                   compactness=10.0)
    del img, mask

    # polygonize: the device passes alone (count + rings into buffers of the right size), then the public call with its host grouping
    nr, nv = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.obia_polygon_count_i32_dev(c.handle, lab.data_ptr(), H, W, 1, ctypes.byref(nr), ctypes.byref(nv)))
    R_, V_ = int(nr.value), int(nv.value)
    bufs = (torch.empty(R_, dtype=torch.int32, device="cuda"), torch.empty(R_, dtype=torch.uint8, device="cuda"),
            torch.zeros(R_ + 1, dtype=torch.int64, device="cuda"), torch.empty((V_, 2), dtype=torch.int32, device="cuda"))

    def poly_passes():
        _lib.check(lib.obia_polygon_count_i32_dev(c.handle, lab.data_ptr(), H, W, 1, ctypes.byref(nr), ctypes.byref(nv)))
        _lib.check(lib.obia_polygon_rings_i32_dev(c.handle, lab.data_ptr(), H, W, 1, R_, V_, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                                  bufs[2].data_ptr(), bufs[3].data_ptr(), ctypes.byref(nr), ctypes.byref(nv)))
    poly_ms, poly_all = timed(poly_passes)
    del bufs
    t0 = time.perf_counter()
    table = polygonize(lab, start_label=1)
    poly_total_s = time.perf_counter() - t0

    xy = torch.as_tensor(table.xy).cuda()
    off = torch.as_tensor(table.ring_offset).cuda()
    owner = torch.as_tensor(np.searchsorted(table.labels, table.ring_label).astype(np.int32)).cuda()
    vals = torch.as_tensor(table.labels.astype(np.int32)).cuda()
    out = torch.empty((H, W), dtype=torch.int32, device="cuda")
    ms, all_ms = timed(raster_call(xy, off, owner, vals, H, W, out))
    info = rasterize_info()
    by = 4 * H * W + 16 * xy.shape[0]
    res["configs2"] = {"size": a.size, "segments": int(n), "shapes": len(table), "rings": int(owner.numel()), "vertices": int(xy.shape[0]),
                       "rasterize_ms": round(ms, 3), "rasterize_all_ms": all_ms, "small_shapes": info["small"], "large_shapes": info["large"],
                       "bytes": by, "GBps": round(by / (ms * 1e-3) / 1e9, 1),
                       "polygonize_device_passes_ms": round(poly_ms, 3), "polygonize_device_passes_all_ms": poly_all,
                       "polygonize_with_host_grouping_s": round(poly_total_s, 2),
                       "round_trip_equal": bool(torch.equal(out, torch.where(lab >= 1, lab, torch.zeros_like(lab))))}
    del xy, off, owner, vals, out, lab, table

    # the large-shape regime alone: stars with many vertices over ~1000 x 1000 pixel boxes
    if a.big_vertices > 0:
        rs = np.random.RandomState(0)
        BH = BW = 4096
        rings = []
        for k in range(8):
            ang = np.sort(rs.uniform(0, 2 * np.pi, a.big_vertices))
            rad = rs.uniform(300, 560, a.big_vertices)
            rings.append(np.stack([600 + 950 * (k % 4) + rad * np.cos(ang), 1000 + 1900 * (k // 4) + rad * np.sin(ang)], 1))
        bxy = torch.as_tensor(np.concatenate(rings)).cuda()
        boff = torch.as_tensor(np.arange(9, dtype=np.int64) * a.big_vertices).cuda()
        bowner = torch.arange(8, dtype=torch.int32, device="cuda")
        bvals = torch.arange(1, 9, dtype=torch.int32, device="cuda")
        bout = torch.empty((BH, BW), dtype=torch.int32, device="cuda")
        ms, all_ms = timed(raster_call(bxy, boff, bowner, bvals, BH, BW, bout))
        info = rasterize_info()
        again = rasterize((bxy, boff, bowner), (BH, BW), values=bvals, as_tensor=True)
        res["large_regime"] = {"raster": [BH, BW], "shapes": 8, "vertices_each": a.big_vertices, "rasterize_ms": round(ms, 3),
                               "rasterize_all_ms": all_ms, "small_shapes": info["small"], "large_shapes": info["large"],
                               "covered_px": int((bout > 0).sum()), "same_through_public_call": bool(torch.equal(again, bout))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
