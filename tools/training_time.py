"""Timing of the training tiles (obia_amd.training) on one GPU.  Prints one JSON line, milliseconds, median of --reps:

  * ``process_tile``: one 300 x 300 x 3 float32 tile on the device (150 m at 0.5 m pixels) -- hard blend and feathered blend
    (feather_radius 4, blur_kernel 11), each with and without a mask-free baseline to tell the new stages from the stretch and CLAHE --
    wall clock around the call, which waits for its result;
  * ``operators``: the new entry points of include/obia_training.h alone on 2048 x 2048 (blur of 3 channels with 5 x 5, 11 x 11 and
    31 x 31; distance with the window of feather_radius 4 (R = 6) and the full transform, on a mask of discs; both blends; min-max of
    2048 x 2048 x 3 float32), device events on the stream the context runs on;
  * ``tile_and_process``: the defaults (tile_size 150, overlap 50, hard blend, blur 5) over a --size x --size x 8 raster at 0.5 m
    pixels with a mask, on the device, ``as_array=True`` -- wall clock, and per tile.

    python tools/training_time.py [--size 16384] [--reps 5]
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


def discs(H, W, period=96, radius=30):
    """0 / 1 mask of discs on a grid, as a CUDA uint8 tensor"""
    yy = (torch.arange(H, device="cuda") % period - period // 2).view(-1, 1)
    xx = (torch.arange(W, device="cuda") % period - period // 2).view(1, -1)
    return ((yy * yy + xx * xx) < radius * radius).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--bands", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-raster", action="store_true", help="only the tile and the operators")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "training_time.py needs a GPU"
    from obia_amd import _lib
    from obia_amd import training as tr

    stream = torch.cuda.current_stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)          # kernels on torch's stream: events bracket them
    lib = _lib.load()

    def wall_ms(fn):
        ts = []
        for i in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            del r
            if i >= a.warmup:
                ts.append(ms)
        return statistics.median(ts)

    def event_ms(fn):
        ts = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    out = {"reps": a.reps, "process_tile_ms": {}, "operators_ms": {}, "tile_and_process": {}}

    # ---- one tile
    g = torch.Generator(device="cuda").manual_seed(0)
    tile = torch.empty((300, 300, 3), dtype=torch.float32, device="cuda").normal_(900.0, 300.0, generator=g)
    tmask = discs(300, 300)
    feathered = dict(feather_radius=4.0, blur_kernel=11)
    pt = out["process_tile_ms"]
    pt["no_mask"] = wall_ms(lambda: tr.process_tile(tile))
    pt["hard"] = wall_ms(lambda: tr.process_tile(tile, tmask))
    pt["feathered"] = wall_ms(lambda: tr.process_tile(tile, tmask, **feathered))
    pt["hard_minmax_no_clahe"] = wall_ms(lambda: tr.process_tile(tile, tmask, rescale=False, apply_clahe_flag=False))
    pt["feathered_minmax_no_clahe"] = wall_ms(lambda: tr.process_tile(tile, tmask, rescale=False, apply_clahe_flag=False, **feathered))

    # ---- the operators alone
    H = W = 2048
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    other = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    res = torch.empty_like(img)
    mask = discs(H, W)
    inv = 255 - mask * 255
    work = torch.empty((H, W), dtype=torch.int32, device="cuda")
    dist = torch.empty((H, W), dtype=torch.float32, device="cuda")
    lut = torch.as_tensor((np.arange(256, dtype=np.uint8) * 0.8).astype(np.uint8), device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    x = torch.empty((H, W, 3), dtype=torch.float32, device="cuda").normal_(900.0, 300.0, generator=g)
    mwork = torch.empty(_lib.TRAIN_MINMAX_WORK, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    op = out["operators_ms"]
    for k in (5, 11, 31):
        w = torch.as_tensor(tr.gaussian_weights(k), device="cuda")
        torch.cuda.synchronize()
        op[f"blur_{k}x{k}"] = event_ms(lambda: _lib.check(lib.obia_train_blur_u8_dev(ctx.handle, img.data_ptr(), H, W, 3, k, k, w.data_ptr(),
                                                                                   w.data_ptr(), res.data_ptr())))
    for name, R in (("distance_R6", 6), ("distance_full", H - 1)):
        op[name] = event_ms(lambda: _lib.check(lib.obia_train_distance_dev(ctx.handle, inv.data_ptr(), H, W, R, work.data_ptr(),
                                                                           dist.data_ptr())))
    op["compose_hard"] = event_ms(lambda: _lib.check(lib.obia_train_compose_u8_dev(ctx.handle, img.data_ptr(), other.data_ptr(), mask.data_ptr(),
                                                                                   None, H, W, lut.data_ptr(), 0.0, res.data_ptr(),
                                                                                   cnt.data_ptr())))
    op["compose_feathered"] = event_ms(lambda: _lib.check(lib.obia_train_compose_u8_dev(ctx.handle, img.data_ptr(), other.data_ptr(),
                                                                                        mask.data_ptr(), dist.data_ptr(), H, W, lut.data_ptr(),
                                                                                        4.0, res.data_ptr(), cnt.data_ptr())))
    op["minmax"] = event_ms(lambda: _lib.check(lib.obia_train_minmax_u8_dev(ctx.handle, x.data_ptr(), x.numel(), mwork.data_ptr(),
                                                                            res.data_ptr(), cnt.data_ptr())))
    del img, other, res, inv, work, dist, x

    # ---- the whole raster
    if not a.skip_raster:
        S = a.size
        raster = torch.empty((S, S, a.bands), dtype=torch.float32, device="cuda")
        for r0 in range(0, S, 1024):                          # filled in slabs: no second raster-sized temporary
            raster[r0:r0 + 1024].normal_(900.0, 300.0, generator=g)
        rmask = discs(S, S)
        affine = [0.5, 0.0, 0.0, -0.5, 500000.0, 5000000.0]
        bands = (4, 2, 1) if a.bands >= 5 else (0, 1, 2)
        n = [0]

        def whole():
            r = tr.tile_and_process(raster, affine, "EPSG:32610", rmask, selected_bands=bands, as_array=True)
            n[0] = len(r)
            return r

        ms = wall_ms(whole)
        out["tile_and_process"] = {"size": S, "bands": a.bands, "tiles": n[0], "ms": round(ms, 1), "ms_per_tile": round(ms / n[0], 4)}
    out["process_tile_ms"] = {k: round(v, 3) for k, v in pt.items()}
    out["operators_ms"] = {k: round(v, 3) for k, v in op.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
