"""Polygons -> label raster on the GPU (obia_amd.polygons.rasterize, obia_amd.cost.rasterise_slic_gpkg).  Every comparison is
array_equal: the raster is exact against the NumPy restatement of the rule (tests/rasterize_restatement.py) and, for rings that
came from a label raster, against that raster."""
import functools
import os

import numpy as np
import pytest

from tests import rasterize_restatement as R

pytestmark = pytest.mark.gpu

TRANSFORMS = {"none": None, "flip": "flip", "utm": [0.5, 0.0, 0.0, -0.5, 443210.0, 6012345.5]}


def _transform(key, H):
    return [1.0, 0.0, 0.0, -1.0, 0.0, float(H)] if key == "flip" else TRANSFORMS[key]


def _blobs(rs, H, W, cell, n_labels):
    """Label map of square-ish blobs: repeated labels (several 4-connected parts), one-pixel segments, frames with holes."""
    coarse = rs.randint(1, n_labels, (H // cell + 1, W // cell + 1))
    lab = np.kron(coarse, np.ones((cell, cell), np.int64))[:H, :W].astype(np.int32)
    lab[rs.rand(H, W) < 0.03] = n_labels + 1                                    # speckle: many parts of one label
    for k in range(min(H, W) // 9):                                             # single pixels with labels of their own
        lab[rs.randint(H), rs.randint(W)] = n_labels + 10 + k
    if H > 30 and W > 30:
        lab[10:24, 12:27] = n_labels + 2                                        # a frame ...
        lab[13:21, 15:24] = n_labels + 3                                        # ... around another label
        lab[16:18, 18:20] = n_labels + 2                                        # ... that has an island of the frame's label inside
    return lab


def _label_maps():
    rs = np.random.RandomState(11)
    maps = {"1x1": (np.array([[5]], np.int32), 0), "1x37": (rs.randint(1, 4, (1, 37)).astype(np.int32), 0),
            "41x1": (rs.randint(0, 3, (41, 1)).astype(np.int32), 0), "blobs65": (_blobs(rs, 65, 65, 8, 7), 0)}
    big = _blobs(rs, 200, 333, 16, 40)
    big[rs.rand(200, 333) < 0.02] = 0
    big[50:90, 100:180] = -1
    big[120:, :30] = 0
    maps["masked200x333"] = (big, 1)
    return maps


LABEL_MAPS = _label_maps()


@functools.lru_cache(maxsize=None)
def _slic_labels():
    from obia_amd.segmentation import slic
    rs = np.random.RandomState(3)
    yy, xx = np.mgrid[0:96, 0:96].astype(np.float64)
    img = np.stack([300 * np.sin(xx / (7 + c)) * np.cos(yy / (9 + c)) + 900 + rs.normal(0, 15, (96, 96)) for c in range(4)], -1)
    return np.asarray(slic(img.astype(np.float32), n_segments=60, compactness=0.3, _normalize_bands=True), np.int32)


@pytest.mark.parametrize("tkey", list(TRANSFORMS))
@pytest.mark.parametrize("name", list(LABEL_MAPS) + ["slic96"])
def test_round_trip_of_our_own_polygons(name, tkey):
    from obia_amd.polygons import polygonize, rasterize, to_pixel
    labels, start = (_slic_labels(), 1) if name == "slic96" else LABEL_MAPS[name]
    H, W = labels.shape
    aff = _transform(tkey, H)
    table = polygonize(labels, aff, start_label=start)
    assert len(table) == len(np.unique(labels[labels >= start]))
    # the vertices are back on the pixel grid to ~1e-9 and every centre is half a pixel from the grid: no centre is near an
    # edge, so the answer does not depend on how ties are decided
    px = to_pixel(table.xy, aff)
    assert np.abs(px - np.round(px)).max() < 1e-6
    fill = -7
    want = np.where(labels >= start, labels, fill).astype(np.int32)
    got = rasterize(table, labels.shape, aff, fill=fill)
    assert got.dtype == np.int32 and got.shape == labels.shape
    assert np.array_equal(got, want)
    assert np.array_equal(rasterize(table.wkb(), labels.shape, aff, values=table.labels, fill=fill), want)
    ids = rasterize(table.wkb(), labels.shape, aff)                              # default values of WKB input: 1..N
    assert np.array_equal(ids, np.where(labels >= start, np.searchsorted(table.labels, labels) + 1, 0))


def _random_shapes(seed, H, W, n):
    rs = np.random.RandomState(seed)
    shapes = []
    for i in range(n):
        kind = i % 6
        cx, cy = rs.uniform(-15, W + 15), rs.uniform(-15, H + 15)
        nv = int(rs.choice([3, 4, 5, 8, 17, 60, 200]))
        ring = R.star(rs, cx, cy, nv, 0.4, rs.uniform(2, 25), shuffle=kind == 1, on_centres=kind == 2)
        rings = [ring]
        if kind == 3:
            rings.append(R.star(rs, cx, cy, 6, 0.3, 2.0))                        # a hole, or a second part, as it falls
        if kind == 4:
            x0, y0 = np.floor(cx) + 0.5, np.floor(cy) + 0.5                      # edges exactly through rows / columns of centres
            rings = [R.rect(x0, y0, x0 + rs.randint(1, 9), y0 + rs.randint(1, 9))]
        if kind == 5 and i % 12 == 5:
            rings = [R.rect(W + 3, -9, W + 30, H + 5)]                           # wholly outside
        shapes.append(rings)
    return shapes, rs.randint(1, 20, n).astype(np.int32)


@pytest.mark.parametrize("H,W,seed", [(33, 47, 0), (130, 70, 1)])
def test_general_polygons_equal_the_restatement(H, W, seed):
    from obia_amd.polygons import rasterize, rasterize_info
    shapes, values = _random_shapes(seed, H, W, 300)
    xy, off, owner = R.pack(shapes)
    want = R.burn(xy, off, owner, values, (H, W), fill=-7)
    got = rasterize((xy, off, owner), (H, W), values=values, fill=-7)
    assert np.array_equal(got, want)
    info = rasterize_info()
    assert info["small"] + info["large"] == 300
    assert (want == -7).any() and len(np.unique(want)) > 10


def test_a_large_shape_among_small_ones_runs_both_regimes():
    from obia_amd.polygons import rasterize, rasterize_info
    H, W = 700, 900
    rs = np.random.RandomState(5)
    small = [[R.star(rs, rs.uniform(0, W), rs.uniform(0, H), rs.randint(3, 40), 1, 25)] for _ in range(50)]
    big = [R.star(rs, 440.3, 361.7, 5000, 150, 420)]
    shapes = small[:25] + [big] + small[25:]
    values = np.arange(1, 52, dtype=np.int32)
    xy, off, owner = R.pack(shapes)
    got = rasterize((xy, off, owner), (H, W), values=values, fill=0)
    info = rasterize_info()
    assert info["large"] == 1 and info["small"] == 50
    want = R.burn(xy, off, owner, values, (H, W), fill=0)
    assert np.array_equal(got, want)
    assert (want == 26).sum() > 50000 and set(np.unique(want)) > {0, 26}


def test_each_side_of_the_regime_thresholds():
    """Edges: max_edges - 1, max_edges (one wave each) and max_edges + 1 (banded).  Bounding box: 63, 64 (one wave) and 65 rows;
    61, 62 (one wave) and 63 columns of centres -- the column range carries one more column on either side."""
    from obia_amd.polygons import rasterize, rasterize_info
    lim = rasterize_info()
    E, side = lim["max_edges"], lim["max_side"]
    rs = np.random.RandomState(9)
    cases = [([R.star(rs, 40.2, 38.7, E + d, 5, 28)], d > 0) for d in (-1, 0, 1)]
    cases += [([R.rect(10.2, 5.2, 30.2, 5.2 + side + d)], d > 0) for d in (-1, 0, 1)]
    cases += [([R.rect(10.2, 5.2, 10.2 + side - 2 + d, 30.2)], d > 0) for d in (-1, 0, 1)]
    for rings, large in cases:
        xy, off, owner = R.pack([rings])
        got = rasterize((xy, off, owner), (100, 100), values=[3], fill=-1)
        info = rasterize_info()
        assert (info["small"], info["large"]) == ((0, 1) if large else (1, 0)), (len(xy), xy.min(0), xy.max(0))
        assert np.array_equal(got, R.burn(xy, off, owner, [3], (100, 100), fill=-1))
        assert (got == 3).sum() > 500


def test_input_and_output_forms():
    import torch
    from obia_amd.polygons import rasterize
    shapes, values = _random_shapes(2, 60, 90, 80)
    xy, off, owner = R.pack(shapes)
    host = rasterize((xy, off, owner), (60, 90), values=values, fill=-2)
    dev_in = tuple(torch.as_tensor(a).cuda() for a in (xy, off, owner))
    dev = rasterize(dev_in, (60, 90), values=torch.as_tensor(values).cuda(), fill=-2, as_tensor=True)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.int32 and tuple(dev.shape) == (60, 90)
    assert np.array_equal(dev.cpu().numpy(), host)
    assert np.array_equal(rasterize(dev_in, (60, 90), values=values, fill=-2), host)            # a second run: identical
    assert np.array_equal(host, R.burn(xy, off, owner, values, (60, 90), fill=-2))
    aff = [0.25, 0.0, 0.0, -0.25, 1000.0, 2000.0]
    map_xy = np.stack([aff[0] * xy[:, 0] + aff[4], aff[3] * xy[:, 1] + aff[5]], 1)
    from obia_amd.polygons import to_pixel
    want = R.burn(to_pixel(map_xy, aff), off, owner, values, (60, 90), fill=-2)
    assert np.array_equal(rasterize((map_xy, off, owner), (60, 90), aff, values=values, fill=-2), want)
    assert np.array_equal(rasterize((torch.as_tensor(map_xy).cuda(),) + dev_in[1:], (60, 90), aff, values=values, fill=-2), want)
    assert np.array_equal(rasterize((xy[:0], off[:1], owner[:0]), (4, 5), fill=6), np.full((4, 5), 6, np.int32))   # nothing to burn


# ------------------------------------------------------------------------------------------------------------- GeoPackage
@pytest.fixture(scope="module")
def tiled(tmp_path_factory):
    from obia_amd.tiling import create_tiled_segments
    tmp = tmp_path_factory.mktemp("gpkg")
    rs = np.random.RandomState(1)
    H, W = 230, 260
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([400 * np.sin(xx / (11 + 3 * c)) * np.cos(yy / (13 + 2 * c)) + 1000 + rs.normal(0, 20, (H, W))
                    for c in range(4)], -1).astype(np.float32)
    mask = np.ones((H, W), bool)
    mask[:40, :60] = False
    T, n = create_tiled_segments(img, output_dir=str(tmp), input_mask=mask, tile_size=100, buffer=16, crown_radius=5,
                                 pixel_size=(1.0, 1.0))
    profile = {"height": H, "width": W, "transform": (1.0, 0.0, 0.0, 0.0, -1.0, 0.0)}
    return os.path.join(str(tmp), "segments.gpkg"), profile, np.asarray(T), n, mask


def _is_function(a, b):
    """Every value of a goes with exactly one value of b."""
    pairs = np.unique(np.stack([a.ravel(), b.ravel()], 1), axis=0)
    return len(pairs) == len(np.unique(a))


def test_segments_gpkg_comes_back_as_the_tilers_partition(tiled):
    from obia_amd.cost import rasterise_slic_gpkg, make_cost_surface
    from obia_amd.consumers import slic_edge
    path, profile, T, n, mask = tiled
    L = rasterise_slic_gpkg(path, profile)
    assert L.dtype == np.int32 and L.shape == T.shape
    assert _is_function(T, L) and _is_function(L, T)
    assert np.array_equal(L == 0, T == 0) and not L[~mask].any()
    assert len(np.unique(L[L > 0])) == n
    assert np.array_equal(slic_edge(L), slic_edge(T))
    rs = np.random.RandomState(2)
    wv3 = rs.uniform(1, 2000, T.shape + (8,)).astype(np.float32)
    chm = rs.uniform(0, 30, T.shape).astype(np.float32)
    a = make_cost_surface(wv3, chm, slic=L, weights=(0.4, 0.2, 0.2, 0.2))
    b = make_cost_surface(wv3, chm, slic=T, weights=(0.4, 0.2, 0.2, 0.2))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    import torch
    Lt = rasterise_slic_gpkg(path, profile, as_tensor=True)
    assert isinstance(Lt, torch.Tensor) and Lt.is_cuda and np.array_equal(Lt.cpu().numpy(), L)


def test_bounds_keep_the_shapes_that_meet_them(tiled):
    from obia_amd.cost import rasterise_slic_gpkg
    path, profile, T, n, mask = tiled
    H, W = T.shape
    L = rasterise_slic_gpkg(path, profile)
    half = rasterise_slic_gpkg(path, dict(profile, bounds=(0.0, -float(H), 130.0, 0.0), crs=None))
    # a shape is kept when its envelope meets x <= 130: it owns a pixel in columns 0..129 or its outline starts at x = 130
    cols = np.broadcast_to(np.arange(W), (H, W))
    first_col = np.full(L.max() + 1, W, np.int64)
    np.minimum.at(first_col, L.ravel(), cols.ravel())
    kept = first_col <= 130
    kept[0] = False
    assert np.array_equal(half, np.where(kept[L], L, 0))
    assert np.array_equal(half[:, :130], L[:, :130])
    assert not half[:, 200:].any() and L[:, 200:].any()


def test_rows_without_an_integer_segment_id_are_skipped(tiled, tmp_path):
    from obia_amd.cost import rasterise_slic_gpkg
    from obia_amd.geopackage import read_geopackage, write_geopackage
    path, profile, T, n, mask = tiled
    L = rasterise_slic_gpkg(path, profile)
    wkbs, cols, srs = read_geopackage(path)
    ids = [str(v) for v in cols["segment_id"]]
    victim = int(ids[len(ids) // 2])
    ids[len(ids) // 2] = "not a number"
    other = write_geopackage(str(tmp_path / "segments.gpkg"), wkbs, {"segment_id": ids})
    got = rasterise_slic_gpkg(other, profile)
    assert (L == victim).any()
    assert np.array_equal(got, np.where(L == victim, 0, L))
