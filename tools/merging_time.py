"""Timing of region merging on the segment graph (obia_amd.merging; include/obia_merging.h) on one GPU, on device-resident inputs:

  * the raster of tools/adjacency_time.py: --size x --size int32 labels, the Voronoi cells of one seed per --cell x --cell square
    (about (size / cell)^2 segments, 10^6 at the defaults), and three float32 bands of smooth fields plus noise, generated on the device;
  * the state (RegionState.from_raster: graph, shapes, zonal statistics), once;
  * the kernels of ONE round on that state: the fusion cost, the best neighbour, the pair merge, and the contraction as its three
    calls (rows, count, write) and whole (SegmentGraph._contract, with torch's prefix sums);
  * beside the contraction an equal composition from torch alone -- mapped keys, one ``torch.sort``, run sums, as
    ``obia_amd.adjacency._csr_of_records`` builds a graph -- checked EQUAL to it first, with the ratio;
  * one round of ``merge_similar`` on the same raster (graph, zonal means and relabel over all pixels), what a round cost before;
  * ``multiresolution_merge`` end to end, with the number of rounds and of objects.

The context runs on torch's stream, and every figure is the time between two device events on that stream around the call (the
call returns with its work done): the first run on its own, then the median of --reps.  There is no gate.  Prints one JSON line.

    python tools/merging_time.py [--size 16384] [--cell 16] [--reps 5] [--scale 40] [--kernels-only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.adjacency_time import jittered_grid, timed  # noqa: E402


def bands_of(S, seed):
    """(S, S, 3) float32: three smooth fields of a few hundred pixels' wavelength plus unit noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = torch.arange(S, device="cuda", dtype=torch.float32)[:, None]
    x = torch.arange(S, device="cuda", dtype=torch.float32)[None, :]
    raw = torch.empty((S, S, 3), dtype=torch.float32, device="cuda")
    raw[:, :, 0] = 100 + 60 * torch.sin(x / 180.0) * torch.cos(y / 230.0)
    raw[:, :, 1] = 80 + 40 * torch.cos((x + y) / 310.0)
    raw[:, :, 2] = 50 + 30 * torch.sin(y / 140.0)
    band = max(1, (1 << 24) // S)
    for r0 in range(0, S, band):
        raw[r0:r0 + band] += torch.randn((min(band, S - r0), S, 3), generator=g, device="cuda")
    return raw


def composed_contract(g, root):
    """(indptr, neighbor, border) of the contracted graph from torch alone"""
    N = g.n_labels
    r = root.to(torch.int64)
    nb = g._neighbor.to(torch.int64)
    real = nb < N
    dst = torch.where(real, r[nb.clamp(max=N - 1)], nb)
    src = r[g._rows()]
    keep = src != dst
    key = (src * (N + 2) + dst)[keep]
    skey, order = torch.sort(key)
    uniq, runs = torch.unique_consecutive(skey, return_counts=True)
    last = torch.cumsum(runs, 0) - 1
    run = torch.cumsum(g._border[keep][order], 0)[last]
    border = run - torch.cat([torch.zeros(1, dtype=torch.int64, device=run.device), run[:-1]])
    s = torch.div(uniq, N + 2, rounding_mode="floor")
    indptr = torch.zeros(N + 1, dtype=torch.int64, device=run.device)
    indptr[1:] = torch.cumsum(torch.bincount(s, minlength=N), 0)
    return indptr, (uniq - s * (N + 2)).to(torch.int32), border


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--cell", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=40.0)
    ap.add_argument("--kernels-only", action="store_true", help="the kernels of one round alone, once each, for a counter run")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "merging_time.py needs a GPU"
    from obia_amd import _lib, adjacency as ADJ, merging as MG

    S = a.size
    torch.cuda.set_stream(torch.cuda.Stream())                                  # a stream of torch's own, not the null stream
    lib = _lib.load()
    ctx = _lib.Context(0, stream=torch.cuda.current_stream().cuda_stream)       # one stream: the events bracket the library's work
    lab, N = jittered_grid(S, a.cell, 7)
    raw = bands_of(S, 11)
    reps = 1 if a.kernels_only else a.reps
    out = {"size": S, "pixels": S * S, "segments": N, "reps": reps, "scale": a.scale, "row_cap": _lib.MERGE_ROW_CAP}
    state = MG.RegionState.from_raster(raw, lab, ctx=ctx)
    g = state.graph
    nnz, F = g.nnz, state.n_bands
    out["nnz"] = nnz
    w = torch.ones(F, dtype=torch.float64, device="cuda")
    P = lambda t: t.data_ptr() if t.numel() else None                           # noqa: E731
    head = (ctx.handle, P(g._indptr), P(g._neighbor), P(g._border), N, nnz)
    tables = (P(state._area), P(state._mean), P(state._m2), F)

    cost = torch.empty(nnz, dtype=torch.float64, device="cuda")
    out["cost"] = timed(lambda: _lib.check(lib.obia_merge_cost_dev(*head, *tables, P(w), P(state._perimeter), P(state._box), 0.9, 0.5, P(cost))), reps)
    out["best_neighbor"] = timed(lambda: g._best(cost), reps)
    partner, pairs = MG._round(state, w.cpu().numpy(), 0.9, 0.5, a.scale * a.scale)
    out["pairs_of_the_first_round"] = pairs
    o = [torch.empty_like(t) for t in (state._area, state._mean, state._m2, state._perimeter, state._box)]
    out["pair_merge"] = timed(lambda: _lib.check(lib.obia_merge_pairs_dev(*head, P(partner), *tables, P(state._perimeter), P(state._box),
                                                                          *[P(t) for t in o])), reps)
    me = torch.arange(N, dtype=torch.int32, device="cuda")
    root = torch.where(partner >= 0, torch.minimum(me, partner), me)

    rawc = torch.empty(N, dtype=torch.int64, device="cuda")
    out["contract_rows"] = timed(lambda: _lib.check(lib.obia_merge_contract_rows_dev(ctx.handle, P(g._indptr), N, nnz, P(root), P(rawc))), reps)
    raw_ptr = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    raw_ptr[1:] = torch.cumsum(rawc, 0)
    key, bw = torch.empty(nnz, dtype=torch.int32, device="cuda"), torch.empty(nnz, dtype=torch.int64, device="cuda")
    cur, cnt = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda")
    out["contract_count"] = timed(lambda: _lib.check(lib.obia_merge_contract_count_dev(*head, P(root), P(raw_ptr), P(key), P(bw), P(cur), P(cnt))), reps)
    iptr = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    iptr[1:] = torch.cumsum(cnt.to(torch.int64), 0)
    total = int(iptr[-1])
    nb, bd = torch.empty(total, dtype=torch.int32, device="cuda"), torch.empty(total, dtype=torch.int64, device="cuda")
    out["contract_write"] = timed(lambda: _lib.check(lib.obia_merge_contract_write_dev(ctx.handle, N, nnz, P(raw_ptr), P(cnt), P(key), P(bw), P(iptr),
                                                                                       total, P(nb), P(bd))), reps)
    out["nnz_after"] = total
    lens = raw_ptr[1:] - raw_ptr[:-1]
    out["gathered_rows"] = {"to_8": int((lens <= 8).sum()), "to_32": int(((lens > 8) & (lens <= 32)).sum()), "longer": int((lens > 32).sum()),
                            "longest": int(lens.max())}
    if a.kernels_only:
        print(json.dumps(out))
        return
    out["contract_whole"] = timed(lambda: g._contract(root), reps)
    cptr, cnb, cbd = composed_contract(g, root)
    assert bool((cptr == iptr).all()) and bool((cnb == nb).all()) and bool((cbd == bd).all()), "the composition and the contraction disagree"
    del cptr, cnb, cbd
    c = timed(lambda: composed_contract(g, root), reps)
    out["torch_composition"] = c
    out["speedup_over_composition"] = round(c["ms"] / out["contract_whole"]["ms"], 2)
    out["round_on_the_graph"] = timed(lambda: MG._merge_pairs(state, MG._round(state, w.cpu().numpy(), 0.9, 0.5, a.scale * a.scale)[0]), reps)
    out["merge_similar_one_round"] = timed(lambda: ADJ.merge_similar(raw, lab, a.scale, max_rounds=1, ctx=ctx), reps)
    res = {}

    def whole():
        res["counts"] = MG.multiresolution_merge(raw, lab, a.scale, ctx=ctx)[1]
    out["multiresolution_merge"] = timed(whole, max(1, reps // 2))
    out["rounds"] = len(res["counts"])
    out["objects"] = res["counts"][-1] if res["counts"] else N
    print(json.dumps(out))


if __name__ == "__main__":
    main()
