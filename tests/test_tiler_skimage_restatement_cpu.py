"""The CPU reference of ``create_tiled_segments(..., seeding="skimage")`` (tests/tiler_skimage_restatement.py) checked on its own, without
a GPU: its override runs, one tile of it IS scikit-image's maskSLIC on a fixture that holds scikit-image's labels, its small-tile skip
works -- and the host side of the drivers refuses an unknown ``seeding`` before any device use."""
import ast
import os

import numpy as np
import pytest

from tests import tiler_skimage_restatement as TR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def synth(H, W, C, seed=0):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([400 * np.sin(xx / (11 + 3 * c)) * np.cos(yy / (13 + 2 * c)) + 1000 + 50 * c + rs.normal(0, 20, (H, W))
                     for c in range(C)], -1).astype(np.float32)


def test_all_ones_mask_differs_from_the_grid_oracle(oracle):
    """the override runs: with every pixel valid the grid oracle seeds a regular grid, scikit-image's rule a k-means of random picks"""
    from oracle import tiler
    img = synth(64, 96, 4, seed=1)
    kw = dict(tile_size=32, buffer=8, n_segments=12, compactness=10.0)
    grid, n_grid = tiler.create_tiled_segments(img, np.ones((64, 96), bool), **kw)
    info = []
    got, n = TR.create_tiled_segments(img, np.ones((64, 96), bool), tile_info=info, **kw)
    assert len(info) == 6 and all(t["skipped"] is None and t["K"] == t["n"] for t in info)
    assert not np.array_equal(got, grid)
    assert n == got.max() and len(np.unique(got[got > 0])) == n


def test_one_tile_is_scikit_images_mask_slic(oracle):
    """tile_size >= the raster: one black tile, whose seeds, steps and labels are scikit-image 0.18.3's own (the fixture's)"""
    z = np.load(os.path.join(GOLD, "mask_128x160x4_c10.npz"))
    params = ast.literal_eval(str(z["params"]))
    raw, mask = z["raw"].astype(np.float32), z["mask"] != 0
    T = 160
    n_valid = int(mask.sum())
    per_full_tile = params["n_segments"] * T * T / n_valid       # the tiler scales it back by n_valid / T^2
    assert round(per_full_tile * n_valid / float(T * T)) == params["n_segments"]
    info = []
    got, n = TR.create_tiled_segments(raw, mask, tile_size=T, buffer=16, n_segments=per_full_tile, compactness=params["compactness"],
                                      max_iter=params.get("max_iter", 10), tile_info=info)
    seeded = [t for t in info if t["skipped"] is None]
    assert len(seeded) == 1 and seeded[0]["window"] == (0, 0, 128, 160) and seeded[0]["K"] == len(z["seeds_yx"])
    want = z["labels"]
    assert (want[~mask] == 0).all() and want.max() == n
    assert np.array_equal(got, want), f"{(got != want).sum()} px differ from scikit-image's labels"


def test_small_tiles_are_skipped(oracle):
    """a tile with one valid pixel, at a density that asks for two segments of it (n >= 2, n_valid < 2), and a tile with n == 1"""
    img = synth(32, 48, 4, seed=2)
    mask = np.ones((32, 48), bool)
    mask[:16, 16:32] = False
    mask[5, 20] = True                      # white tile (0, 1): one valid pixel of its own
    kw = dict(tile_size=16, buffer=0, crown_radius=0.45, pixel_size=(1.0, 1.0), compactness=10.0)     # n = round(1.57 * n_valid)
    info = []
    got, n = TR.create_tiled_segments(img, mask, tile_info=info, **kw)
    one = [t for t in info if t["n_valid"] == 1]
    assert len(one) == 1 and one[0]["n"] == 2 and one[0]["skipped"] == "small"
    assert got[5, 20] == 0 and (got[mask & (np.arange(48)[None, :] // 16 != 1)] > 0).all()
    info = []
    mask2 = np.ones((32, 48), bool)
    mask2[:16, 16:32] = False
    mask2[4:9, 18:30] = True                # 60 valid pixels at 6 segments per 256: n = round(1.4) = 1
    got2, _ = TR.create_tiled_segments(img, mask2, tile_size=16, buffer=0, n_segments=6, compactness=10.0, tile_info=info)
    small = [t for t in info if t["skipped"] == "small"]
    assert len(small) == 1 and small[0]["n"] == 1 and small[0]["n_valid"] == 60
    assert (got2[4:9, 18:30] == 0).all()


@pytest.mark.parametrize("bad", ["random", "", None, "SKIMAGE", 1])
def test_unknown_seeding_is_refused_before_any_device_use(bad, monkeypatch):
    from obia_amd import _lib, distributed, tiling

    def no_device(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(_lib, "default_context", no_device)
    img = np.zeros((8, 8, 2), np.float32)
    with pytest.raises(ValueError, match="seeding"):
        tiling.create_tiled_segments(img, seeding=bad)
    with pytest.raises(ValueError, match="seeding"):
        distributed.ShardedTiler(img, None, 8, 1, 8, 0, comm=object(), seeding=bad)
