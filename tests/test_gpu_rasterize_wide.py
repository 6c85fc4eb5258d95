"""The rasteriser's large shapes past their first column tile (rasterize.hip: rast_large_kernel), against tests/rasterize_restatement.py:
exact, every pixel.

A workgroup of the large regime takes a band of 8 rows and walks its columns in tiles; in every tile after the first a crossing left
of the tile toggles a carry instead of a bit, and the tile origin -- the shape's first column plus a multiple of the tile width -- is
no multiple of anything.  The shapes of tests/test_gpu_rasterize.py are at most 840 columns wide: one tile.  Here a shape spans three
tiles on a raster of 21 rows (bands of 8 + 8 + 5 rows).  The tile width T is the library's (tests/launch_grids.py: unit), every
output is a guarded buffer, and the cases whose point is a tile border assert on the expected raster that the border is exercised
both ways before the GPU runs."""
import functools

import numpy as np
import pytest

from tests import launch_grids as LG
from tests import rasterize_restatement as R
from tests.test_gpu_launch_clamps import rasterize_guarded

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

I32 = np.int32
H = 21
X0 = 37.3                                                        # the wide shape's left end: its first column is neither 0 nor a multiple of 32


def tile_w():
    return LG.unit("rast_large", (1, 1), 1, "y")


def raster_w():
    return 2 * tile_w() + 400 + 60


def first_column(xmin):
    """the first column of a shape's box by the restated rule"""
    return max(R._first_centre_ge(xmin) - 1, 0)


def zigzag(rs, x_lo, x_hi, y_top, y_mid_top, y_mid_bot, y_bot, n=400):
    """a ring over [x_lo, x_hi]: n vertices along the top that alternate between y_top and y_mid_top, n along the bottom between y_bot
    and y_mid_bot, at irregular abscissae -- every row between the extremes is crossed every few columns"""
    def xs():
        return np.concatenate([[x_lo], np.sort(rs.uniform(x_lo, x_hi, n - 2)), [x_hi]])
    alt = np.arange(n) % 2 == 0
    top = np.stack([xs(), np.where(alt, y_top, y_mid_top)], 1)
    bottom = np.stack([xs()[::-1], np.where(alt, y_bot, y_mid_bot)], 1)
    return np.concatenate([top, bottom])


def tiles_of(c0, c1):
    T = tile_w()
    return [(a, min(a + T - 1, c1)) for a in range(c0, c1 + 1, T)]


@functools.lru_cache(maxsize=None)
def three_tiles():
    """the wide shape (a hole in its solid middle row, across the border of tiles 0 and 1) and its restated raster"""
    T, W = tile_w(), raster_w()
    rs = np.random.RandomState(60)
    outer = zigzag(rs, X0, X0 + 2 * T + 400, 0.2, 9.6, 11.4, 20.8)
    c0 = first_column(X0)
    hole = R.rect(c0 + T - 300.4, 9.9, c0 + T + 200.7, 11.2)
    xy, off, owner = R.pack([[outer, hole]])
    want = R.burn(xy, off, owner, [7], (H, W), fill=-1)
    return xy, off, owner, want


def test_three_tiles_from_an_odd_origin():
    T, W = tile_w(), raster_w()
    xy, off, owner, want = three_tiles()
    c0, c1 = first_column(X0), min(R._first_centre_ge(xy[:, 0].max()), W - 1)
    assert c0 > 0 and c0 % 32 != 0 and len(tiles_of(c0, c1)) == 3 and c1 < W - 1
    for a, b in tiles_of(c0, c1):
        part = want[:, a:b + 1]
        assert (part == 7).any() and (part == -1).any(), (a, b)
        assert all((part[:, w:w + 32] == 7).any() and (part[:, w:w + 32] == -1).any() for w in range(0, b + 1 - a - 31, 32)), (a, b)
    col = want[:, c0 + T]                                        # the first column of tile 1: the carry is taken odd in one row, even in another
    assert (col == 7).any() and (col == -1).any()
    assert (want[10, c0 + T - 300:c0 + T + 200] == -1).all() and want[10, c0 + T + 201] == 7        # the hole, across the border
    info = rasterize_guarded(xy, off, owner, [7], H, W, -1, want, "three tiles")
    assert (info["large"], info["small"]) == (1, 0)


def test_crossings_on_the_tile_borders():
    """vertical edges exactly on a tile's first centre (c0 + T + 0.5: the carry), one double above it (bit 1 of the tile), on the last
    centre of the tile before (its last bit) and one double above that (the tile before skips it, the next one carries) -- at both
    borders; odd notches have the edge as their right side, even ones as their left"""
    T, W = tile_w(), raster_w()
    c0 = first_column(X0)
    assert c0 + 0.5 < X0 + 1                                      # (c0 is the column before the first centre at or right of X0)
    rings = [R.rect(X0, 0.3, X0 + 2 * T + 400, 20.7)]
    xs = []
    for border in (c0 + T, c0 + 2 * T):
        for x in (border + 0.5, border - 0.5):
            xs += [x, float(np.nextafter(x, np.inf))]
    assert len(set(xs)) == 8 and all(float(np.float64(x)) == x for x in xs)
    for k, x in enumerate(xs):
        y0, y1 = 2 * k + 1.2, 2 * k + 2.9                         # rows 2k + 1 and 2k + 2
        rings.append(R.rect(x, y0, x + 9.3, y1) if k % 2 == 0 else R.rect(x - 9.3, y0, x, y1))
    xy, off, owner = R.pack([rings])
    want = R.burn(xy, off, owner, [7], (H, W), fill=-1)
    # what the rule says at the borders: an edge on a centre covers from that column, one double above it from the next
    for k, x in enumerate(xs):
        col = int(np.floor(x))                                   # the column whose centre is x, or just left of x
        on_centre = x == col + 0.5
        first_in = col if on_centre else col + 1                 # first column at or right of the edge
        inside, outside = (first_in, first_in - 1) if k % 2 == 0 else (first_in - 1, first_in)
        for r in (2 * k + 1, 2 * k + 2):
            assert want[r, inside] == -1 and want[r, outside] == 7, (k, x, r)
    info = rasterize_guarded(xy, off, owner, [7], H, W, -1, want, "tile borders")
    assert (info["large"], info["small"]) == (1, 0)


def test_a_shape_clipped_on_every_side():
    """the box starts 5000 columns left of the raster (c0 clamps to 0: many crossings at or left of tile 0's first centre), ends right of
    it (c1 clamps to W - 1), and reaches past the first and the last row"""
    T, W = tile_w(), raster_w()
    rs = np.random.RandomState(61)
    ring = zigzag(rs, -5000.3, W + 300.7, -3.2, 9.6, 11.4, H + 4.1, n=700)
    xy, off, owner = R.pack([[ring]])
    assert first_column(xy[:, 0].min()) == 0 and R._first_centre_ge(xy[:, 0].max()) > W - 1
    assert (ring[:, 0] < 0).sum() > 300 and xy[:, 1].min() < 0 and xy[:, 1].max() > H
    want = R.burn(xy, off, owner, [7], (H, W), fill=-1)
    for a, b in tiles_of(0, W - 1):
        assert (want[:, a:b + 1] == 7).any() and (want[:, a:b + 1] == -1).any()
    assert (want[:, 0] == 7).any() and (want[:, 0] == -1).any() and (want[:, W - 1] == 7).any() and (want[:, W - 1] == -1).any()
    info = rasterize_guarded(xy, off, owner, [7], H, W, -1, want, "clipped")
    assert (info["large"], info["small"]) == (1, 0)


def test_the_last_shape_wins_across_tiles():
    """40 small stars (the one-wave path), half burned before the wide shape and half after it, centred inside tiles 1 and 2 and on
    their borders"""
    T, W = tile_w(), raster_w()
    xy_w, off_w, _, _ = three_tiles()
    wide = [xy_w[off_w[i]:off_w[i + 1]] for i in range(len(off_w) - 1)]
    c0 = first_column(X0)
    rs = np.random.RandomState(62)
    cx = np.concatenate([[c0 + T, c0 + T + 0.5, c0 + 2 * T - 0.5, c0 + 2 * T], rs.uniform(c0 + T + 10, c0 + 2 * T + 390, 36)])
    rs.shuffle(cx)
    stars = [[R.star(rs, x, rs.uniform(3, 18), rs.randint(3, 40), 1, 8)] for x in cx]
    shapes = stars[:20] + [wide] + stars[20:]
    values = np.arange(1, 42, dtype=I32)
    xy, off, owner = R.pack(shapes)
    want = R.burn(xy, off, owner, values, (H, W), fill=0)
    seen = set(np.unique(want).tolist())
    assert {0, 21} < seen and len(seen & set(range(1, 21))) >= 10 and set(range(22, 42)) <= seen       # some stars lie under the wide shape
    info = rasterize_guarded(xy, off, owner, values, H, W, 0, want, "last wins")
    assert (info["large"], info["small"]) == (1, 40)


def test_input_forms_of_a_wide_shape():
    from obia_amd.polygons import rasterize
    W = raster_w()
    xy, off, owner, want = three_tiles()
    host = rasterize((xy, off, owner), (H, W), values=[7], fill=-1)
    assert host.dtype == I32 and np.array_equal(host, want)
    dev_in = tuple(torch.as_tensor(a).cuda() for a in (xy, off, owner))
    out = rasterize(dev_in, (H, W), values=torch.as_tensor(np.array([7], I32)).cuda(), fill=-1, as_tensor=True)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (H, W)
    assert np.array_equal(out.cpu().numpy(), want)
    again = rasterize(dev_in, (H, W), values=[7], fill=-1)       # a second run: identical
    assert np.array_equal(again, want)
