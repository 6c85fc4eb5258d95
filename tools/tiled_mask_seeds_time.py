"""Timing of the tiled driver under both seeding rules on one GPU, on bench.py's raster (16384 x 16384 x 8, tile 2048, buffer 64, crown
radius 5, 0.5 m pixels, all-ones mask, compactness 10; --size scales it down).  Per rule: the whole create_tiled_segments call with the
raster resident on the device, host clock, median of --reps after --warmup calls, as Mpixel/s.  For seeding="skimage" also what the
seeding adds per seeded tile -- (skimage call - grid call) / tiles that asked for picks: the k-means, the nearest-centroid search and
the host-side draws, which the library overlaps with the previous tile's kernels -- and the host time inside the pick function alone.
Prints one JSON line.

The same command on the parent commit (which has no `seeding` argument) gives the grid rule's figure to compare against: --rules grid.

Status of the numbers: see DESIGN.md 3.5i.

    python tools/tiled_mask_seeds_time.py [--size 16384] [--tile 2048] [--buffer 64] [--bands 8] [--reps 3] [--warmup 1] [--rules grid,skimage]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--buffer", type=int, default=64)
    ap.add_argument("--bands", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rules", default="grid,skimage")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "tiled_mask_seeds_time.py needs a GPU"
    from bench import synth_raster
    from obia_amd import segmentation, tiling
    img = synth_raster(a.size, a.size, a.bands, 0, "cuda")
    kw = dict(tile_size=a.tile, buffer=a.buffer, crown_radius=5, pixel_size=(0.5, 0.5), compactness=10.0)
    res = {"gpu": torch.cuda.get_device_name(0), "raster": [a.size, a.size, a.bands], "tile_size": a.tile, "buffer": a.buffer,
           "reference_cpu_seeding_s_per_2048_tile": 220.0}
    # host time inside the pick function, and how often it is asked: wrap the draw the pick source calls
    draw = segmentation._mask_seed_picks
    spent = {"s": 0.0, "draws": 0}

    def timed_draw(n_valid, n):
        t0 = time.perf_counter()
        out = draw(n_valid, n)
        spent["s"] += time.perf_counter() - t0
        spent["draws"] += 1
        return out
    segmentation._mask_seed_picks = timed_draw
    calls = {"n": 0}
    answer = segmentation.MaskSeedPickSource._answer

    def counted(self, *args):
        calls["n"] += 1
        return answer(self, *args)
    segmentation.MaskSeedPickSource._answer = counted
    for rule in a.rules.split(","):
        extra = {} if rule == "grid" else {"seeding": rule}          # (the parent commit has no such argument)
        for _ in range(a.warmup):
            tiling.create_tiled_segments(img, **kw, **extra)
        ms, n = [], 0
        spent.update(s=0.0, draws=0)
        calls["n"] = 0
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, n = tiling.create_tiled_segments(img, **kw, **extra)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ms)
        res[rule] = {"call_ms": round(med, 2), "call_all_ms": [round(v, 2) for v in ms], "segments": int(n),
                     "mpixel_per_s": round(a.size * a.size / (med * 1e-3) / 1e6, 2)}
        if rule != "grid":
            res[rule].update(tiles_seeded_per_call=calls["n"] // max(a.reps, 1), host_draws_per_call=spent["draws"] / max(a.reps, 1),
                             host_draw_ms_per_call=round(spent["s"] * 1e3 / max(a.reps, 1), 2))
    if "grid" in res and "skimage" in res and res["skimage"]["tiles_seeded_per_call"]:
        res["skimage"]["seeding_ms_per_tile"] = round((res["skimage"]["call_ms"] - res["grid"]["call_ms"]) / res["skimage"]["tiles_seeded_per_call"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
