"""Timing of the sharpness raster (obia_amd.image.laplacian) on one GPU: the whole call on a device-resident 16384 x 16384 x 8 float32
raster (the benchmark raster's size) with ``win = 15``, and each entry point of include/obia_sharpness.h on planes of that size.  Device
events on the stream the library's context runs on.  Prints one JSON line: milliseconds (median of --reps) and the GB/s each figure
amounts to on the bytes its passes MUST move (compulsory traffic, counted below; not what the kernels really moved).

    python tools/sharpness_time.py [--size 16384] [--bands 8] [--win 15] [--reps 5]

Compulsory bytes per pixel:
  gray_lap   : min / max pass, 3 bands x 4 B read                                  = 12
               normalise + grey + Laplacian, 3 bands x 4 B read + 4 B written      = 16        obia_sharp_gray_lap_dev   = 28
  laplacian  : the stencil alone on a grey plane, 4 B read + 4 B written                        obia_sharp_laplacian_dev  =  8
  variance   : box axis 0, 4 B lap read + 2 x 4 B (mean, mean of squares) written  = 12
               box axis 1 with the variance, 2 x 4 B read + 4 B written            = 12        obia_sharp_variance_dev   = 24
  box        : axis 0 and axis 1 of one plane, 4 B read + 4 B written each                      obia_sharp_box_dev        = 16
  select     : 3 radix passes over the float32 plane, 4 B each                                  the percentile select     = 12
  stretch    : 4 B read + 4 B written                                                           obia_sharp_stretch_f32_dev =  8
  laplacian  : gray_lap + variance + select + stretch                                           obia_amd.image.laplacian  = 72
The two axes of a box filter are one entry point and are not timed apart: half of ``variance`` (``box``) is the average of its passes.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

BYTES_PER_PIXEL = {"laplacian": 72, "gray_lap": 28, "laplacian_plane": 8, "variance": 24, "box": 16, "select": 12, "stretch": 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--bands", type=int, default=8)
    ap.add_argument("--win", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sharpness_time.py needs a GPU"
    from obia_amd import _lib, _percentile
    from obia_amd import image as I

    H = W = a.size
    g = torch.Generator(device="cuda").manual_seed(0)
    raster = torch.empty((H, W, a.bands), dtype=torch.float32, device="cuda")
    for r0 in range(0, H, 1024):                              # filled in slabs: no second raster-sized temporary
        raster[r0:r0 + 1024].normal_(900.0, 300.0, generator=g)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)          # kernels on torch's stream: events bracket them
    lib = _lib.load()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        r = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def median_ms(fn):
        ts = []
        for i in range(a.warmup + a.reps):
            ms, r = timed(fn)
            del r
            if i >= a.warmup:
                ts.append(ms)
        return statistics.median(ts)

    out = {"size": a.size, "bands": a.bands, "win": a.win, "reps": a.reps, "ms": {}, "gb_per_s": {}}
    bands = (1, 2, 4) if a.bands >= 5 else (0, 1, 2)
    out["ms"]["laplacian"] = median_ms(lambda: I.laplacian(raster, None, a.win, bands=bands, ctx=ctx))
    lap = torch.empty((H, W), dtype=torch.float32, device="cuda")
    idx = (ctypes.c_int32 * 3)(*bands)
    out["ms"]["gray_lap"] = median_ms(lambda: _lib.check(lib.obia_sharp_gray_lap_dev(ctx.handle, raster.data_ptr(), H, W, a.bands, idx,
                                                                                    lap.data_ptr(), None)))
    del raster
    work = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
    sharp = torch.empty((H, W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    out["ms"]["variance"] = median_ms(lambda: _lib.check(lib.obia_sharp_variance_dev(ctx.handle, lap.data_ptr(), H, W, a.win, work.data_ptr(),
                                                                                    sharp.data_ptr())))
    out["ms"]["box"] = median_ms(lambda: _lib.check(lib.obia_sharp_box_dev(ctx.handle, lap.data_ptr(), H, W, a.win, work.data_ptr(),
                                                                          work[1].data_ptr(), None)))
    out["ms"]["laplacian_plane"] = median_ms(lambda: _lib.check(lib.obia_sharp_laplacian_dev(ctx.handle, sharp.data_ptr(), H, W,
                                                                                            work.data_ptr(), None)))
    q = _percentile.quantiles(2, 98)
    out["ms"]["select"] = median_ms(lambda: _percentile.select(lib, ctx, sharp, q))
    lo, hi, _ = _percentile.select(lib, ctx, sharp, q)
    out["ms"]["stretch"] = median_ms(lambda: _lib.check(lib.obia_sharp_stretch_f32_dev(ctx.handle, sharp.data_ptr(), H * W, lo, hi,
                                                                                      work.data_ptr())))
    for k, bpp in BYTES_PER_PIXEL.items():
        out["gb_per_s"][k] = round(bpp * H * W / out["ms"][k] / 1e6, 1)
    out["ms"] = {k: round(v, 3) for k, v in out["ms"].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
