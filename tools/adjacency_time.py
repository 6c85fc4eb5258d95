"""Timing of the segment adjacency graph (obia_amd.adjacency; include/obia_adjacency.h) on one GPU, on device-resident inputs:

  * the raster: --size x --size int32 labels, the Voronoi cells of one seed per --cell x --cell square at a random place inside it
    (a jittered grid: about (size / cell)^2 segments, 10^6 at the defaults), generated on the device;
  * the two TILE PASSES (obia_adj_tile_count_dev, obia_adj_tile_write_dev), each against the compulsory 4 bytes per pixel;
  * the PLUMBING between them and the CSR (torch: prefix sum, sort of the keys, sums over runs of equal keys, row starts);
  * each TABLE KERNEL on that CSR: d2 and the neighbour statistics over --features columns, the border to --classes classes, the best
    neighbour, the components of `d2 <= median`, and the relabelling of the raster by them;
  * beside them what a user can compose from torch today for the same graph -- two shifted comparisons, the keys of both directions
    of every border edge, ``torch.unique(return_counts=True)`` over all of them -- checked EQUAL to the CSR, with the ratio.

The context runs on torch's stream, and every figure is the time between two device events on that stream around the call (the
library's calls return with their work done, so a figure holds the launch gaps of its call): the first run on its own, then the
median of --reps.  There is no earlier implementation to compare with and no gate.  Prints one JSON line.

    python tools/adjacency_time.py [--size 16384] [--cell 16] [--reps 5] [--passes-only]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(1 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return {"first_ms": round(ts[0], 3), "ms": round(statistics.median(ts[1:]), 3), "ms_min": round(min(ts[1:]), 3),
            "ms_max": round(max(ts[1:]), 3)}


def jittered_grid(S, cell, seed):
    """(S, S) int32 labels from 1: every pixel goes to the nearest seed, one seed per cell x cell square, ties to the lower cell"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = -(-S // cell)
    sy = (torch.arange(n, device="cuda")[:, None] + torch.rand((n, n), generator=g, device="cuda")) * cell
    sx = (torch.arange(n, device="cuda")[None, :] + torch.rand((n, n), generator=g, device="cuda")) * cell
    lab = torch.empty((S, S), dtype=torch.int32, device="cuda")
    band = max(cell, (1 << 24) // S // cell * cell)
    xs = torch.arange(S, device="cuda", dtype=torch.float32)[None, :] + 0.5
    cx = (torch.arange(S, device="cuda") // cell)[None, :]
    for r0 in range(0, S, band):
        r1 = min(S, r0 + band)
        ys = torch.arange(r0, r1, device="cuda", dtype=torch.float32)[:, None] + 0.5
        cy = (torch.arange(r0, r1, device="cuda") // cell)[:, None]
        best = torch.full((r1 - r0, S), float("inf"), device="cuda")
        arg = torch.zeros((r1 - r0, S), dtype=torch.int32, device="cuda")
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                qy, qx = (cy + dy).clamp(0, n - 1), (cx + dx).clamp(0, n - 1)
                d = (sy[qy, qx] - ys) ** 2 + (sx[qy, qx] - xs) ** 2
                better = d < best
                best = torch.where(better, d, best)
                arg = torch.where(better, (qy * n + qx + 1).to(torch.int32), arg)
        lab[r0:r1] = arg
    return lab, n * n


def composed_graph(lab, N):
    """the directed (key, edges) table of the same graph from torch alone; start_label 1"""
    S = lab.to(torch.int64) - 1
    S = torch.where((S >= 0) & (S < N), S, torch.full_like(S, N))
    keys = []

    def both(a, b):
        m = (a != b) & (torch.minimum(a, b) < N)
        a, b = a[m], b[m]
        keys.append((a * (N + 2) + b)[a < N])
        keys.append((b * (N + 2) + a)[b < N])
    both(S[:, :-1], S[:, 1:])
    both(S[:-1], S[1:])
    for edge in (S[0], S[-1], S[:, 0], S[:, -1]):
        keys.append(edge[edge < N] * (N + 2) + (N + 1))
    return torch.unique(torch.cat(keys), return_counts=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--cell", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--features", type=int, default=4)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--passes-only", action="store_true", help="the two tile passes alone, for a counter run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "adjacency_time.py needs a GPU"
    from obia_amd import _lib, adjacency as A

    S = a.size
    torch.cuda.set_stream(torch.cuda.Stream())                                  # a stream of torch's own, not the null stream
    lib = _lib.load()
    ctx = _lib.Context(0, stream=torch.cuda.current_stream().cuda_stream)       # one stream: the events bracket the library's work
    h = ctx.handle
    lab, N = jittered_grid(S, a.cell, 7)
    npx = S * S
    n_tiles = -(-S // _lib.ADJ_TILE_H) * -(-S // _lib.ADJ_TILE_W)
    out = {"size": S, "pixels": npx, "segments": N, "tiles": n_tiles, "reps": a.reps, "tile": [_lib.ADJ_TILE_H, _lib.ADJ_TILE_W]}

    count = torch.empty(n_tiles, dtype=torch.int32, device="cuda")
    t = timed(lambda: _lib.check(lib.obia_adj_tile_count_dev(h, lab.data_ptr(), S, S, 1, N, count.data_ptr())), a.reps)
    t["GBps_of_4B_per_pixel"] = round(4 * npx / (t["ms"] * 1e-3) / 1e9, 1)
    out["tile_count"] = t
    c64 = count.to(torch.int64)
    offset, total = torch.cumsum(c64, 0) - c64, int(c64.sum())
    key = torch.empty(total, dtype=torch.int64, device="cuda")
    edges = torch.empty(total, dtype=torch.int32, device="cuda")
    work = torch.empty(_lib.ADJ_WORK, dtype=torch.int32, device="cuda")
    t = timed(lambda: _lib.check(lib.obia_adj_tile_write_dev(h, lab.data_ptr(), S, S, 1, N, offset.data_ptr(), total, key.data_ptr(),
                                                             edges.data_ptr(), work.data_ptr())), a.reps)
    t["GBps_of_4B_per_pixel"] = round(4 * npx / (t["ms"] * 1e-3) / 1e9, 1)
    out["tile_write"] = t
    out["records"] = total
    out["records_per_pixel"] = round(total / npx, 4)
    if a.passes_only:
        print(json.dumps(out))
        return

    def plumbing():
        c = count.to(torch.int64)
        _ = torch.cumsum(c, 0) - c
        return A._csr_of_records(key, edges, N)
    out["plumbing_torch"] = timed(plumbing, a.reps)
    indptr, neighbor, border = plumbing()
    g = A.SegmentGraph(indptr, neighbor, border, N, 1, ctx=ctx)
    out["nnz"] = g.nnz
    out["segment_graph_whole"] = timed(lambda: A.segment_graph(lab, 1, N, ctx=ctx), a.reps)

    gen = torch.Generator(device="cuda").manual_seed(11)
    values = torch.rand((N, a.features), generator=gen, device="cuda", dtype=torch.float64)
    classes = torch.randint(0, a.classes, (N,), generator=gen, device="cuda", dtype=torch.int32)
    out["d2"] = timed(lambda: g.d2(values), a.reps)
    d2 = g.d2(values)
    out["neighbor_stats"] = timed(lambda: g.neighbor_stats(values), a.reps)
    out["border_to_class"] = timed(lambda: g.border_to_class(classes, a.classes), a.reps)
    out["best_neighbor"] = timed(lambda: g.best_neighbor(d2), a.reps)
    link = (d2 <= torch.nanmedian(d2)).to(torch.uint8)
    out["components"] = timed(lambda: g.components(link), a.reps)
    root = g.components(link)
    table = A.compact_roots(root, 1)
    out["components_found"] = int(table.max())
    t = timed(lambda: A.relabel(lab, table, 1, ctx=ctx), a.reps)
    t["GBps_of_8B_per_pixel"] = round(8 * npx / (t["ms"] * 1e-3) / 1e9, 1)
    out["relabel"] = t

    # the same graph from torch alone, checked equal
    ukey, ucount = composed_graph(lab, N)
    mine = A.SegmentGraph._rows(g) * (N + 2) + neighbor.to(torch.int64)
    assert ukey.shape == mine.shape and bool((ukey == mine).all()) and bool((ucount == border).all()), "the composition and the graph disagree"
    del ukey, ucount, mine
    torch.cuda.empty_cache()
    c = timed(lambda: composed_graph(lab, N), a.reps)
    out["torch_composition"] = c
    ours = out["tile_count"]["ms"] + out["tile_write"]["ms"] + out["plumbing_torch"]["ms"]
    out["graph_ms_passes_plus_plumbing"] = round(ours, 3)
    out["speedup_over_composition"] = round(c["ms"] / ours, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
