"""Timing of the image previews (obia_amd.image) on one GPU: ``to_image(as_array=True)`` for each ``stretch_type`` on a device-resident
16384 x 16384 x 8 float32 raster (the benchmark raster's size), and ``Segments.to_segmented_image(as_array=True)`` on its label map.
Device events on the stream the library's context runs on.  Prints one JSON line: milliseconds (median of --reps) and the GB/s each
figure amounts to on the bytes its passes MUST move (compulsory traffic, counted below; not what the kernels really moved).

    python tools/image_time.py [--size 16384] [--bands 8] [--reps 5]

Compulsory bytes per pixel:
  gather     : 3 bands x 4 B read + 12 B written                                    = 24
  select     : 3 radix passes over the float32 plane, 12 B each                     = 36
  stretch    : 12 B read + 3 B written                                              = 15        to_image(None)          = 75
  equalise   : 3 B read + 1 B grey written; 1 B read + 3 B written                  =  8        ... histogram_equalization = 83
  clahe      : per channel 1 B read (histograms) + 1 B read + 1 B written, x 3      =  9        ... clahe                = 84
  overlay    : 3 B image + 4 B labels read, 3 B written (the host image is uploaded outside the timed span) = 10
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

BYTES_PER_PIXEL = {"to_image_none": 75, "to_image_histogram_equalization": 83, "to_image_clahe": 84, "to_segmented_image": 10,
                   "stretch_only": 15}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--bands", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "image_time.py needs a GPU"
    from obia_amd import _lib
    from obia_amd import image as I

    H = W = a.size
    g = torch.Generator(device="cuda").manual_seed(0)
    raster = torch.empty((H, W, a.bands), dtype=torch.float32, device="cuda")
    for r0 in range(0, H, 1024):                              # filled in slabs: no second raster-sized temporary
        raster[r0:r0 + 1024].normal_(900.0, 300.0, generator=g)
    yy = torch.arange(H, device="cuda", dtype=torch.int32)[:, None]
    xx = torch.arange(W, device="cuda", dtype=torch.int32)[None, :]
    labels = ((yy // 23) * ((W + 28) // 29) + xx // 29 + 1).to(torch.int32).contiguous()      # blocks of 23 x 29 pixels
    del yy, xx
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    ctx = _lib.Context(0, stream=stream.cuda_stream)          # kernels on torch's stream: events bracket them

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

    out = {"size": a.size, "bands": a.bands, "reps": a.reps, "ms": {}, "gb_per_s": {}}
    bands = [4, 2, 1]
    for st in (None, "histogram_equalization", "clahe"):
        out["ms"][f"to_image_{str(st).lower()}"] = median_ms(lambda: I.to_image(raster, bands, stretch_type=st, as_array=True, ctx=ctx))
    rgb = I.to_image(raster, bands, as_array=True, ctx=ctx)
    del raster
    lib = _lib.load()
    table = torch.as_tensor(I.mark_table(), device="cuda")
    color = (ctypes.c_uint8 * 3)(255, 255, 0)
    marked = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out["ms"]["to_segmented_image"] = median_ms(lambda: _lib.check(lib.obia_image_mark_u8_dev(
        ctx.handle, rgb.data_ptr(), 3, labels.data_ptr(), H, W, table.data_ptr(), color, marked.data_ptr())))
    # the same through the public method: the PIL image is a host array, so this figure includes its upload and the label check
    from PIL.Image import fromarray
    from obia_amd.segmentation import Segments
    pil = fromarray(rgb.cpu().numpy())
    seg = Segments(labels, None, "slic")
    out["ms"]["to_segmented_image_from_pil"] = median_ms(lambda: seg.to_segmented_image(pil, as_array=True, ctx=ctx))
    x = torch.empty((H, W, 3), dtype=torch.float32, device="cuda").normal_(900.0, 300.0, generator=g)
    u = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out["ms"]["stretch_only"] = median_ms(lambda: _lib.check(lib.obia_image_stretch_u8_dev(ctx.handle, x.data_ptr(), 0, x.numel(), 300.0, 1500.0,
                                                                                          u.data_ptr())))
    for k, bpp in BYTES_PER_PIXEL.items():
        out["gb_per_s"][k] = round(bpp * H * W / out["ms"][k] / 1e6, 1)
    out["ms"] = {k: round(v, 3) for k, v in out["ms"].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
