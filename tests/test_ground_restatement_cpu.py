"""Height above ground without a GPU: the restatement (tests/ground_restatement.py) against hand-worked answers; the generators of
tests/test_gpu_ground.py hold the classes their cases exist for; the cell-side rule keeps the grid within 4 ng + 16 cells; every
argument refusal of obia_amd.pointcloud's ground functions fires before the library is loaded; the query launch is a named grid."""
import math
import os

import numpy as np
import pytest

from tests import ground_restatement as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QNAN64, QNAN32 = 0x7FF8000000000000, 0x7FC00000

# a unit lattice of four ground points with elevations 10, 20, 30, 40 in index order
LATTICE = (np.array([0.0, 1.0, 0.0, 1.0]), np.array([0.0, 0.0, 1.0, 1.0]), np.array([10.0, 20.0, 30.0, 40.0]))


def _one(x, y, count, md=0.0, ground=LATTICE):
    r = G.ground_z(ground, [x], [y], count, md)
    return float(r["zg"][0]), int(r["m"][0]), r["idx"][0].tolist()


def test_a_four_way_tie_goes_to_the_lower_index():
    # every d2 is 0.5: the order is the index order, and equal weights make the mean of the first `count` elevations
    assert _one(0.5, 0.5, 1) == (10.0, 1, [0])
    assert _one(0.5, 0.5, 2) == (15.0, 2, [0, 1])
    assert _one(0.5, 0.5, 3) == (20.0, 3, [0, 1, 2])
    assert _one(0.5, 0.5, 4) == (25.0, 4, [0, 1, 2, 3])
    assert bool(G.ground_z(LATTICE, [0.5], [0.5], 2)["tie"][0]) and not bool(G.ground_z(LATTICE, [0.25], [0.125], 3)["tie"][0])
    # a permuted ground set: the same four points, the tie goes to whoever stands first now
    p = [3, 1, 0, 2]
    assert _one(0.5, 0.5, 1, ground=tuple(v[p] for v in LATTICE))[0] == 40.0


def test_a_query_on_a_ground_point_takes_its_elevation():
    assert _one(1.0, 0.0, 3) == (20.0, 3, [1, 0, 3])                      # d2 = 0, 1, 1 (index 0 before 3), never a division by zero
    assert _one(1.0, 0.0, 1) == (20.0, 1, [1])
    # two ground points at one (x, y): the lower index answers, the other elevation is not seen
    twice = (np.array([2.0, 2.0, 5.0]), np.array([3.0, 3.0, 3.0]), np.array([7.0, 9.0, 1.0]))
    assert _one(2.0, 3.0, 2, ground=twice) == (7.0, 2, [0, 1])
    assert G.hag([7.0, 9.0], [7.0, 7.0]).tolist() == [0.0, 2.0]            # ... so the second of the pair is not at height 0


def test_fewer_neighbours_than_count():
    zg, m, idx = _one(0.25, 0.0, 8)
    assert m == 4 and idx == [0, 1, 2, 3, -1, -1, -1, -1]
    # weights 1 / d2 = 16, 16 / 9, 16 / 17, 16 / 25
    w = [1.0 / 0.0625, 1.0 / 0.5625, 1.0 / 1.0625, 1.0 / 1.5625]
    want = ((((0.0 + 10.0 / 0.0625) + 20.0 / 0.5625) + 30.0 / 1.0625) + 40.0 / 1.5625) / ((((0.0 + w[0]) + w[1]) + w[2]) + w[3])
    assert zg == want and abs(zg - (160 + 320 / 9 + 480 / 17 + 640 / 25) / (16 + 16 / 9 + 16 / 17 + 16 / 25)) < 1e-13
    assert _one(3.0, 4.0, 8, ground=(np.array([0.0]), np.array([0.0]), np.array([5.5]))) == (5.5, 1, [0] + [-1] * 7)


def test_the_cut_off_includes_equality():
    # d2 = 0.0625, 0.5625, 1.0625, 1.5625; 0.75^2 = 0.5625 exactly: the second point is in
    zg, m, idx = _one(0.25, 0.0, 3, 0.75)
    assert m == 2 and idx == [0, 1, -1]
    assert zg == (10.0 / 0.0625 + 20.0 / 0.5625) / (1.0 / 0.0625 + 1.0 / 0.5625) and abs(zg - 11.0) < 1e-14
    assert _one(0.25, 0.0, 3, np.nextafter(0.75, 0.0)) == (10.0, 1, [0, -1, -1])
    assert _one(0.25, 0.0, 3, 0.25)[:2] == (10.0, 1)                      # 0.25^2 = 0.0625: equality again
    zg, m, idx = _one(0.25, 0.0, 3, 0.2)
    assert math.isnan(zg) and m == 0 and idx == [-1, -1, -1]
    assert _one(0.25, 0.0, 1, 0.0)[:2] == (10.0, 1)                        # 0: no limit


def test_nan_and_infinity():
    r = G.ground_z(LATTICE, [np.nan, 0.2, np.inf, 0.2, 1e200], [0.2, np.nan, 0.2, -np.inf, 0.0], 2)
    assert r["m"].tolist() == [0, 0, 0, 0, 2]
    assert r["zg"].view(np.uint64).tolist()[:4] == [QNAN64] * 4
    # a finite query so far away that every d2 is infinite: two neighbours by index, and 0 / 0 from the weights
    assert r["idx"][4].tolist() == [0, 1] and r["zg"].view(np.uint64)[4] == QNAN64
    assert G.ground_z(LATTICE, [1e200], [0.0], 1)["zg"][0] == 10.0
    h = G.hag([np.nan, 5.0, np.inf, -np.inf, 300.1, 5.0], [1.0, np.nan, 1.0, 1.0, 0.1, -np.inf])
    assert h.view(np.uint32).tolist()[:2] == [QNAN32] * 2 and h[2:].tolist() == [np.inf, -np.inf, 300.0, np.inf]
    minus = -np.abs(np.array([np.nan]))                                     # a NaN with the sign bit set comes out as the quiet NaN
    assert G.hag(minus, [0.0]).view(np.uint32)[0] == QNAN32 and G.canonical(minus).view(np.uint64)[0] == QNAN64
    # one rounding: the difference in float64, then float32
    assert G.hag([300.123456789], [0.000000001])[0] == np.float32(300.123456789 - 0.000000001)


def test_the_terrain_raster_rule():
    affine = [2.0, 0.0, 0.0, -2.0, 100.0, 50.0]                             # 2 m pixels, the top-left corner at (100, 50)
    dtm = np.array([[1.0, 2.0, 3.0], [4.0, np.nan, np.inf]], np.float32)
    x = [100.0, 101.9, 102.0, 105.9, 106.0, 99.9, 103.0, 105.0, 101.0, np.nan]
    y = [50.0, 48.1, 50.0, 46.1, 49.0, 49.0, 47.0, 47.0, 45.9, 49.0]
    zg = G.dtm_z(x, y, dtm, affine)
    assert zg[:3].tolist() == [1.0, 1.0, 2.0] and zg[8:].view(np.uint64).tolist() == [QNAN64] * 2
    assert np.isnan(zg[3:]).all()                                           # the inf pixel, right of it, left, the NaN pixel, inf again, below
    cx, cy = G.pixel_centres((2, 3), affine)
    assert cx.tolist() == [101.0, 103.0, 105.0] * 2 and cy.tolist() == [49.0] * 3 + [47.0] * 3
    dtm2 = G.to_raster(LATTICE, (2, 2), [1.0, 0.0, 0.0, 1.0, -0.5, -0.5])   # pixel centres on the lattice points
    assert dtm2.dtype == np.float32 and dtm2.tolist() == [[10.0, 20.0], [30.0, 40.0]]


# --------------------------------------------------------------------------------------------- the generators of the GPU cases
def test_the_base_case_holds_the_classes_it_is_there_for():
    pytest.importorskip("torch")
    from obia_amd.pointcloud import _ground_side
    given = G.base_ground()
    ground, dropped = G.keep_ground(*given)
    gx, gy, _ = ground
    assert dropped == 5 and 2700 <= len(gx) <= 3300
    side = _ground_side(gx.min(), gx.max(), gy.min(), gy.max(), len(gx))
    x, y, z = G.base_queries(given, side)
    assert 4900 <= len(x) <= 5100 and np.isnan(z).sum() > 300
    r = G.ground_z(ground, x, y, 3, 0.0)
    nearest = np.sqrt(r["d2"][:, 0])
    finite = np.isfinite(x) & np.isfinite(y)
    assert (~finite).sum() == 6 and np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(y).any()
    assert r["tie"].sum() >= 11                                             # the duplicated ground points under a query
    assert (nearest[finite] > side).sum() > 300                             # queries that need ring 2 or more: the disc, the surroundings
    assert (nearest[finite] > 40 * side).sum() > 100                        # ... and many rings: up to three extents outside
    assert (r["d2"][:, 0] == 0.0).sum() >= 600                              # exactly on a ground point (every 7th, less those moved to a cell border)
    far = (x < gx.min() - G.EXTENT[0]) | (x > gx.max() + G.EXTENT[0]) | (y < gy.min() - G.EXTENT[1]) | (y > gy.max() + G.EXTENT[1])
    assert (far & finite).sum() > 200
    on_cell_border = (np.floor(x / side) * side == x) & finite
    assert on_cell_border.sum() > 300
    for md in (0.0, 1.5, 0.75):
        rr = G.ground_z(ground, x, y, 8, md)
        share = np.isnan(G.hag(z, rr["zg"])).mean()
        assert share < 0.5, (md, share)
        if md:
            assert ((rr["m"] > 0) & (rr["m"] < 8)).sum() > 300 and (rr["m"][finite] == 0).sum() > 300 and (rr["m"] == 8).sum() >= (50 if md > 1 else 0)
    assert (G.ground_z(ground, x, y, 1, 0.75)["m"][finite] == 0).sum() > 300      # "so small that some queries find nothing"


@pytest.mark.parametrize("ng", [1, 2, 3, 7, 100, 3000, 10 ** 6, 2 ** 31 - 1])
def test_the_cell_side_keeps_the_grid_within_4_ng_plus_16(ng):
    pytest.importorskip("torch")
    from obia_amd.pointcloud import _ground_side
    rs = np.random.RandomState(ng % 1000)
    boxes = [(5.0, 5.0, 5.0, 5.0), (0.0, 0.0, 0.0, 0.0), (0.0, 100.0, 3.0, 3.0), (7.0, 7.0, -1e6, 1e6), (6e5, 6e5 + 1e-3, 4.2e6, 4.2e6 + 1e3),
              (-1e-300, 1e-300, 0.0, 1e-300), (-1e15, 1e15, -1.0, 1.0), (0.0, 1e-9, 0.0, 1e9)]
    for _ in range(200):
        x0, y0 = rs.uniform(-1, 1, 2) * 10.0 ** rs.uniform(-3, 7, 2)
        boxes.append((x0, x0 + 10.0 ** rs.uniform(-6, 6), y0, y0 + 10.0 ** rs.uniform(-6, 6)))
    for x0, x1, y0, y1 in boxes:
        side = _ground_side(x0, x1, y0, y1, ng)
        assert side > 0.0 and math.isfinite(side)
        ncx = math.floor(x1 / side) - math.floor(x0 / side) + 1
        ncy = math.floor(y1 / side) - math.floor(y0 / side) + 1
        assert 1 <= ncx * ncy <= 4 * ng + 16, (x0, x1, y0, y1, side, ncx, ncy)
        assert max(abs(v) / side for v in (x0, x1, y0, y1)) <= 2.0 ** 29 * (1 + 1e-15)
    with pytest.raises(ValueError, match="not finite"):
        _ground_side(-1.7e308, 1.7e308, 0.0, 1.0, 5)


# ------------------------------------------------------------------------------------------------------ refusals before the library
@pytest.fixture()
def no_library(monkeypatch):
    pytest.importorskip("torch")
    from obia_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were judged")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "default_context", boom)


def _raw(n=4, classification=(2, 1, 2, 5), **extra):
    d = {"X": np.arange(n, dtype=np.float64), "Y": np.zeros(n), "Z": np.full(n, 300.0)}
    if classification is not None:
        d["Classification"] = np.array(classification, np.uint8)
    d.update(extra)
    return d


def test_every_argument_refusal_fires_before_the_library_loads(no_library):
    import torch
    from obia_amd import pointcloud as P
    cloud = _raw()
    bare = P.GroundIndex.__new__(P.GroundIndex)                              # the methods judge their arguments before they look at the index
    for count in (0, 9, -1, 1.5):
        for call in (lambda: P.height_above_ground(cloud, count=count), lambda: P.normalize_heights(cloud, count=count),
                     lambda: bare.ground_z([0.0], [0.0], count=count), lambda: bare.height_above_ground(cloud, count=count),
                     lambda: bare.to_raster((2, 2), [1, 0, 0, 1, 0, 0], count=count), lambda: bare.neighbours([0.0], [0.0], count=count)):
            with pytest.raises(ValueError, match="count"):
                call()
    for md in (-1.0, -1e-300, float("nan")):
        for call in (lambda: P.height_above_ground(cloud, max_distance=md), lambda: bare.ground_z([0.0], [0.0], max_distance=md),
                     lambda: bare.to_raster((2, 2), [1, 0, 0, 1, 0, 0], max_distance=md)):
            with pytest.raises(ValueError, match="max_distance"):
                call()
    for call in (lambda: P.height_above_ground(_raw(classification=None)), lambda: P.GroundIndex.from_cloud(_raw(classification=None)),
                 lambda: P.normalize_heights(_raw(classification=None))):
        with pytest.raises(ValueError, match="Classification"):
            call()
    empty = [lambda: P.GroundIndex(_raw(0, ())), lambda: P.GroundIndex(dict(_raw(), Z=np.full(4, np.nan))),
             lambda: P.GroundIndex(dict(_raw(), X=np.array([np.inf, np.nan, -np.inf, np.nan]))),
             lambda: P.GroundIndex.from_cloud(_raw(classification=(1, 1, 3, 5))), lambda: P.GroundIndex.from_cloud(_raw(), ground_class=7),
             lambda: P.height_above_ground(_raw(classification=(0, 0, 0, 0))), lambda: P.height_above_ground(cloud, ground=_raw(0, ()))]
    for call in empty:
        with pytest.raises(ValueError, match="ground set is empty"):
            call()
    mixed = dict(_raw(), Y=torch.zeros(4, dtype=torch.float64))
    for call in (lambda: P.GroundIndex(mixed), lambda: P.height_above_ground(mixed), lambda: P.height_above_dtm(mixed, np.zeros((2, 2), np.float32), [1, 0, 0, 1, 0, 0]),
                 lambda: bare.ground_z(np.zeros(2), torch.zeros(2, dtype=torch.float64)), lambda: P.normalize_heights(mixed)):
        with pytest.raises(ValueError, match="all tensors or all arrays"):
            call()
    cpu = {k: torch.as_tensor(v) for k, v in _raw().items()}
    for call in (lambda: P.GroundIndex(cpu), lambda: P.GroundIndex.from_cloud(cpu), lambda: P.height_above_ground(cpu),
                 lambda: P.height_above_dtm(cpu, np.zeros((2, 2), np.float32), [1, 0, 0, 1, 0, 0]), lambda: P.normalize_heights(cpu),
                 lambda: bare.ground_z(cpu["X"], cpu["Y"]), lambda: bare.height_above_ground(cpu)):
        with pytest.raises(ValueError, match="must live on the GPU"):
            call()
    with pytest.raises(ValueError, match="no Z field"):
        P.height_above_ground({"X": np.zeros(2), "Y": np.zeros(2), "HeightAboveGround": np.zeros(2), "Classification": np.full(2, 2)})
    with pytest.raises(ValueError, match="one length"):
        P.GroundIndex({"X": np.zeros(2), "Y": np.zeros(3), "Z": np.zeros(2)})
    with pytest.raises(ValueError, match="one length"):
        bare.ground_z(np.zeros(2), np.zeros(3))
    for shape, affine in (((0, 4), [1, 0, 0, 1, 0, 0]), ((4,), [1, 0, 0, 1, 0, 0]), ((4, 4), [1, 2, 2, 4, 0, 0]), ((4, 4), [1, 0, 0])):
        with pytest.raises(ValueError):
            bare.to_raster(shape, affine)
    with pytest.raises(NotImplementedError, match="2\\^31 pixels"):
        bare.to_raster((65536, 65536), [1, 0, 0, 1, 0, 0])
    for dtm, affine in ((np.zeros(4, np.float32), [1, 0, 0, 1, 0, 0]), (np.zeros((0, 4), np.float32), [1, 0, 0, 1, 0, 0]),
                        (np.zeros((2, 2), np.float32), [1, 2, 2, 4, 0, 0]), (np.zeros((2, 2), np.float32), None)):
        with pytest.raises(ValueError):
            P.height_above_dtm(cloud, dtm, affine)
    with pytest.raises(ValueError, match="not both"):
        P.normalize_heights(cloud, ground=cloud, dtm=np.zeros((2, 2), np.float32), affine_transformation=[1, 0, 0, 1, 0, 0])
    with pytest.raises(TypeError):
        P.GroundIndex(np.zeros((4, 3)))


def test_the_existing_functions_keep_reading_heights_as_given():
    pytest.importorskip("torch")
    from obia_amd.pointcloud import as_points
    d = dict(_raw(), HeightAboveGround=np.full(4, 2.0, np.float32))
    assert as_points(d).z.tolist() == [2.0] * 4 and as_points(_raw()).z.tolist() == [300.0] * 4


def test_public_names():
    pytest.importorskip("torch")
    import inspect
    from obia_amd import pointcloud as P
    for name in ("GroundIndex", "height_above_ground", "height_above_dtm", "normalize_heights"):
        assert callable(getattr(P, name))
    for name in ("from_cloud", "ground_z", "height_above_ground", "to_raster"):
        assert callable(getattr(P.GroundIndex, name))
    sig = inspect.signature(P.height_above_ground).parameters
    assert list(sig)[:2] == ["pointcloud", "ground"] and sig["ground"].default is None
    assert all(sig[k].kind is sig[k].KEYWORD_ONLY for k in ("ground_class", "count", "max_distance"))
    assert (sig["ground_class"].default, sig["count"].default, sig["max_distance"].default) == (2, 1, 0.0)
    assert inspect.signature(P.GroundIndex.from_cloud).parameters["ground_class"].default == 2


def test_the_query_launch_is_a_named_grid():
    pytest.importorskip("torch")
    from obia_amd import _lib
    from tests import launch_grids as LG
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert LG.names()["ground_query"] == ("n",)
    n2 = LG.crossing("ground_query", (1,), 0, "x")
    assert n2 is not None and n2 % 256 == 1 and n2 <= 2 ** 21              # 256 queries per workgroup; a second trip a test can afford
    gx, gy, tx, ty = LG.grid("ground_query", n2)
    assert (gy, tx, ty) == (1, 2, 1) and LG.grid("ground_query", n2 - 1) == (gx, 1, 1, 1)
    src = open(os.path.join(ROOT, "obia_amd", "csrc", "ground.hip")).read()
    assert "grids::ground_query(" in src and "flat_grid(" in src
