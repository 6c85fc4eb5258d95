"""Timing of the raster pass of the shape columns (obia_amd.shapes; include/obia_shapes.h) on one GPU, on device-resident inputs:

  * the raster of tools/adjacency_time.py: --size x --size int32 labels, the Voronoi cells of one seed per --cell x --cell square
    (about (size / cell)^2 segments, 10^6 at the defaults), generated on the device;
  * the PASS (obia_shape_sums_dev: two fills, the tile kernel, the box kernel) against the compulsory 4 bytes per pixel;
  * the DERIVED COLUMNS of the resulting table (torch, N rows), all of them once;
  * beside the pass an equal composition from torch alone -- ``index_add_`` on int64 for the six sums, four shifted comparisons for
    the perimeter, ``scatter_reduce_`` amin / amax for the box -- checked EQUAL to the pass first, with the ratio.

The context runs on torch's stream, and every figure is the time between two device events on that stream around the call (the
call returns with its work done): the first run on its own, then the median of --reps.  There is no earlier implementation to
compare with and no gate.  Prints one JSON line.

    python tools/shapes_time.py [--size 16384] [--cell 16] [--reps 5] [--pass-only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.adjacency_time import jittered_grid, timed  # noqa: E402


def composed_tables(lab, N):
    """(sums (N, 7) int64, box (N, 4) int32) of the same raster from torch alone; start_label 1.  Row band by row band, so that the
    int64 temporaries of a 16384^2 raster fit beside it."""
    H, W = lab.shape
    dev = lab.device
    sums = torch.zeros((N, 7), dtype=torch.int64, device=dev)
    lo = torch.full((N, 2), max(H, W), dtype=torch.int64, device=dev)
    hi = torch.zeros((N, 2), dtype=torch.int64, device=dev)
    cols = torch.arange(W, dtype=torch.int64, device=dev)[None, :]
    band = max(1, (1 << 24) // W)
    outside = torch.full((1, W), N + 1, dtype=torch.int64, device=dev)

    def index(a):
        s = a.to(torch.int64) - 1
        return torch.where((s >= 0) & (s < N), s, torch.full_like(s, N))
    for r0 in range(0, H, band):
        r1 = min(H, r0 + band)
        S = index(lab[r0:r1])
        up = torch.cat([index(lab[r0 - 1:r0]) if r0 else outside, S[:-1]])
        down = torch.cat([S[1:], index(lab[r1:r1 + 1]) if r1 < H else outside])
        side = torch.full((r1 - r0, 1), N + 1, dtype=torch.int64, device=dev)
        left, right = torch.cat([side, S[:, :-1]], 1), torch.cat([S[:, 1:], side], 1)
        edges = (up != S).to(torch.int64) + (down != S) + (left != S) + (right != S)
        rows = torch.arange(r0, r1, dtype=torch.int64, device=dev)[:, None].expand(r1 - r0, W)
        cc = cols.expand(r1 - r0, W)
        keep = S < N
        i, r, c, e = S[keep], rows[keep], cc[keep], edges[keep]
        sums.index_add_(0, i, torch.stack([torch.ones_like(r), r, c, r * r, c * c, r * c, e], 1))
        idx = i[:, None].expand(-1, 2)
        rc = torch.stack([r, c], 1)
        lo.scatter_reduce_(0, idx, rc, "amin", include_self=True)
        hi.scatter_reduce_(0, idx, rc + 1, "amax", include_self=True)
    lo = torch.where(sums[:, :1] > 0, lo, torch.zeros_like(lo))
    return sums, torch.cat([lo, hi], 1).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--cell", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pass-only", action="store_true", help="the pass alone, for a counter run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "shapes_time.py needs a GPU"
    from obia_amd import _lib, shapes as SH

    S = a.size
    torch.cuda.set_stream(torch.cuda.Stream())                                  # a stream of torch's own, not the null stream
    lib = _lib.load()
    ctx = _lib.Context(0, stream=torch.cuda.current_stream().cuda_stream)       # one stream: the events bracket the library's work
    lab, N = jittered_grid(S, a.cell, 7)
    npx = S * S
    out = {"size": S, "pixels": npx, "segments": N, "reps": a.reps, "tile": [_lib.ADJ_TILE_H, _lib.ADJ_TILE_W]}
    sums = torch.empty((N, _lib.SHAPE_SUMS), dtype=torch.int64, device="cuda")
    box = torch.empty((N, 4), dtype=torch.int32, device="cuda")
    t = timed(lambda: _lib.check(lib.obia_shape_sums_dev(ctx.handle, lab.data_ptr(), S, S, 1, N, sums.data_ptr(), box.data_ptr())), a.reps)
    t["GBps_of_4B_per_pixel"] = round(4 * npx / (t["ms"] * 1e-3) / 1e9, 1)
    out["shape_sums"] = t
    if a.pass_only:
        print(json.dumps(out))
        return
    table = SH.ShapeTable(sums, box, N, 1)

    def columns():
        return [getattr(table, k) for k in ("centroid", "mu", "eigenvalues", "major_axis_length", "minor_axis_length", "eccentricity", "orientation",
                                            "extent", "compactness", "shape_index", "smoothness")]
    out["derived_columns_torch"] = timed(columns, a.reps)
    out["segment_shapes_whole"] = timed(lambda: SH.segment_shapes(lab, 1, N, ctx=ctx), a.reps)

    csums, cbox = composed_tables(lab, N)
    assert bool((csums == sums).all()) and bool((cbox == box).all()), "the composition and the pass disagree"
    del csums, cbox
    torch.cuda.empty_cache()
    c = timed(lambda: composed_tables(lab, N), a.reps)
    out["torch_composition"] = c
    out["speedup_over_composition"] = round(c["ms"] / out["shape_sums"]["ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
