"""Timing of the seeds path (obia_amd.seeds) on one GPU: peak detection on a seeded 16384^2 plane and the pairwise merge at
n = 10^4 and 5 * 10^4 seeds, device-resident inputs, host clock around calls that end in a stream synchronisation (median of
--reps after --warmup).  Prints one JSON line: milliseconds, the bytes the peak pass must move (from shapes) and the
fraction of 6.3 TB/s (measured achievable HBM bandwidth) they imply, pairs per second of the merge, and -- for scale only --
the time of the CPU restatement (tests/seeds_restatement.py) at sizes it can run.

    python tools/seeds_time.py [--size 16384] [--n 10000 50000] [--reps 5] [--cpu-size 2048] [--cpu-n 1000]
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

HBM_MEASURED = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--n", type=int, nargs="*", default=[10000, 50000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-size", type=int, default=2048)
    ap.add_argument("--cpu-n", type=int, default=1000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "seeds_time.py needs a GPU"
    from obia_amd import seeds
    from tests import seeds_restatement as R

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), [round(v, 3) for v in ms], r

    res = {"gpu": torch.cuda.get_device_name(0)}
    H = W = a.size
    P = H * W
    g = torch.Generator(device="cuda").manual_seed(0)
    # a canopy-like plane: smooth bumps every ~24 pixels plus noise, NaN speckle
    small = torch.rand((H // 8 + 1, W // 8 + 1), generator=g, device="cuda") * 30
    chm = torch.nn.functional.interpolate(small[None, None], size=(H, W), mode="bilinear", align_corners=False)[0, 0].contiguous()
    chm += torch.rand((H, W), generator=g, device="cuda")
    chm[torch.rand((H, W), generator=g, device="cuda") < 1e-4] = float("nan")
    torch.cuda.synchronize()
    for name, sigma, d in (("peaks_sigma1_d3", 1, 3), ("peaks_sigma0_d3", 0, 3), ("peaks_sigma2_d4", 2, 4)):
        ms, all_ms, out = timed(lambda: seeds.detect_peaks(chm, 2.5, d, sigma))
        # compulsory bytes: each Gaussian pass reads and writes the plane (8 P each); the flag pass reads it and writes a byte; the
        # count and the scatter read the flag bytes; the peaks themselves are noise
        by = (16 * P if sigma > 0 else 0) + 5 * P + 2 * P
        res[name] = {"size": a.size, "ms": round(ms, 3), "all_ms": all_ms, "n_peaks": int(len(out[0])), "bytes": by,
                     "frac_of_6.3TBs": round(by / (ms * 1e-3) / HBM_MEASURED, 3)}
    del chm, small

    CH = CW = 2048
    rs = np.random.RandomState(0)
    cost = torch.as_tensor(R.cost_raster(rs, CH, CW)).cuda()
    aff = R.pixel_affine(0.5, CH)
    inv = R.inverse6(aff)
    for n in a.n:
        # pixel-centre seeds at one per ~6 x 6 pixels of a square region: a few neighbours within the merge radius
        side = int(np.sqrt(n * 36.0)) + 1
        pix = rs.choice(side * side, n, replace=False)
        pix.sort()                                              # row-major, as the peak list is
        rows, cols = pix // side, pix % side
        xs = torch.as_tensor(aff[0] * (cols + 0.5) + aff[4]).cuda()
        ys = torch.as_tensor(aff[3] * (rows + 0.5) + aff[5]).cuda()
        pairs = n * (n - 1) // 2
        r = {"n": n, "pairs": pairs}
        for name, fn in (("link_ms", lambda: seeds.merge_clusters(xs, ys, cost, inv, 0.5, 0.8, 1.5)),
                         ("link_no_prune_ms", lambda: seeds.merge_clusters(xs, ys, cost, inv, 0.5, 0.8, 1.5, prune=False)),
                         ("stats_ms", lambda: seeds.pair_stats(xs, ys, cost, inv, 0.5, 0.8))):
            ms, all_ms, out = timed(fn)
            r[name] = round(ms, 3)
            r[name.replace("_ms", "_all_ms")] = all_ms
            if name == "link_ms":
                r["clusters"] = int(out.max()) + 1
        r["no_prune_pairs_per_s"] = round(pairs / (r["link_no_prune_ms"] * 1e-3), 1)
        r["stats_pair_evaluations_per_s"] = round(3 * pairs / (r["stats_ms"] * 1e-3), 1)
        res[f"merge_n{n}"] = r

    if a.cpu_size > 0:
        n = a.cpu_size
        pl = (np.kron(rs.rand(n // 8, n // 8), np.ones((8, 8))) * 30 + rs.rand(n, n)).astype(np.float32)
        t0 = time.perf_counter()
        np.where(R.peaks_scipy(pl, 2.5, 3, 1))
        res["cpu_restatement_peaks_s_at"] = {"size": n, "s": round(time.perf_counter() - t0, 3)}
    if a.cpu_n > 0:
        xs, ys, c, af = R.pixel_centre_case(0, a.cpu_n, 200, 200, 0.5)
        t0 = time.perf_counter()
        R.components(R.distance_matrix(xs, ys, c, R.inverse6(af), 0.5, 0.8, 12), 1.5)
        res["cpu_restatement_merge_s_at"] = {"n": a.cpu_n, "s": round(time.perf_counter() - t0, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
