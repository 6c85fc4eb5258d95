"""CPU reference of the tiled driver with ``seeding="skimage"``: the oracle's tile loops (oracle/tiler.py, untouched) with ONE method
replaced -- how a tile is segmented.  Test infrastructure: the library never imports it.

Every tile is seeded as scikit-image 0.18 seeds maskSLIC, from the tile's own mask (for a white tile: the input mask minus kept segments
and corner squares, exactly the `tmask` the parent hands to ``_run_tile``): ``tests.mask_seeds_restatement.mask_centroids(tmask, n)``,
whose picks index the valid pixels of the tile window in row-major order.  The seeds go into the pinned SLIC oracle the way
tests/test_oracle_golden.py feeds scikit-image's own seeds: ``seeds_yx = centroids[:, 1:]``, ``seed_steps = [max(steps[0], steps[1]),
steps[2]]`` (step = max(steps); the depth step of a one-plane mask is 0).  The steps are NOT divided by ``spacing``: the single-raster
``slic(seeding="skimage")`` passes them on as they come out of the seeding, and the tiled driver follows it.

Same ``n`` rule and same skip rules as the parent, plus one: a tile with ``n < 2`` or fewer than two valid pixels is skipped --
scikit-image ends with a zero step there and raises, and the reference's tile loop swallows the ValueError ("empty tile").
"""
import math

import numpy as np

from oracle import oracle as orc
from oracle.tiler import OracleTiler
from tests import mask_seeds_restatement as R


class SkimageSeededTiler(OracleTiler):
    """``tile_info``: one dict per tile that reached the ``n`` rule, in processing order: window, n_valid, n, skipped (None or the
    reason), and for a seeded tile the restatement's own info (K, n_dense -- None: every valid pixel was a k-means point)."""

    tile_info = ()      # (an instance gets its own list with its first tile: _run_tile is the only method this class defines)

    def _run_tile(self, y0, x0, h, w, tmask):
        tile = self.img[y0:y0 + h, x0:x0 + w].copy()
        if any(tile[:, :, c].max() == tile[:, :, c].min() for c in range(self.C)) or not np.isfinite(tile).all():
            return
        nvalid = int(tmask.sum())
        if self.n_segments is not None:
            n = round(self.n_segments * nvalid / float(self.T * self.T))
        else:
            n = round(nvalid * self.pw * self.ph / (math.pi * self.crown_radius ** 2))
        info = dict(window=(y0, x0, h, w), n_valid=nvalid, n=int(n), skipped=None)
        self.tile_info = list(self.tile_info) + [info]
        if n < 1 or nvalid == 0:
            info["skipped"] = "empty"
            return
        if n < 2 or nvalid < 2:
            info["skipped"] = "small"
            return
        cent, steps = R.mask_centroids(tmask, int(n), info=info)
        lab = orc.slic(orc.normalize(tile), n_segments=int(n), compactness=self.compactness, max_iter=self.max_iter,
                       mask=tmask.astype(np.uint8), min_size_factor=self.msf, max_size_factor=self.xsf, sigma=self.sigma,
                       spacing=self.spacing, seeds_yx=cent[:, 1:], seed_steps=np.array([max(steps[0], steps[1]), steps[2]]))
        sub = self.G[y0:y0 + h, x0:x0 + w]
        for l in np.unique(lab[lab > 0]):
            sel = lab == l
            sub[sel] = self.next_id
            self.sizes[self.next_id] = int(sel.sum())
            self.alive[self.next_id] = True
            self.next_id += 1


def create_tiled_segments(img, mask=None, tile_size=200, buffer=30, crown_radius=5, pixel_size=(1.0, 1.0), n_segments=None,
                          compactness=10.0, max_iter=10, min_size_factor=0.5, max_size_factor=3, white_order=0, sigma=0, spacing=None,
                          tile_info=None):
    """oracle.tiler.create_tiled_segments with the tiler above.  white_order 0: raster order of the white tiles; 1: even tile rows,
    then odd ones (the sharded driver's).  ``tile_info`` (a list) receives the tiler's ``tile_info``."""
    img = np.asarray(img, np.float32)
    H = img.shape[0]
    t = SkimageSeededTiler(img, mask, H, 0, tile_size, buffer, crown_radius, pixel_size, n_segments, compactness, max_iter,
                           min_size_factor, max_size_factor, sigma, spacing)
    nty = -(-H // tile_size)
    t.run(False, 0, nty)
    if white_order == 1:
        t.run(True, 0, nty, 0)
        t.run(True, 0, nty, 1)
    else:
        t.run(True, 0, nty)
    if tile_info is not None:
        tile_info.extend(t.tile_info)
    return t.finalize()
