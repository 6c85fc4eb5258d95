"""Point clouds without a GPU: the restatement (tests/pointcloud_restatement.py) against hand-worked answers and against the
reference's arithmetic (np.mean / np.var of Intensity, segment_statistics.py:332-389), the telescoping of ``pad`` to ``pai``, and
the refusals of obia_amd.pointcloud and create_objects that fire before the device is touched."""
import numpy as np
import pytest

from tests import pointcloud_restatement as R

# a 2 x 2 raster of unit pixels whose top-left corner is the map point (0, 2): col = X, row = 2 - Y
AFFINE_2X2 = [1.0, 0.0, 0.0, -1.0, 0.0, 2.0]
LABELS_2X2 = np.array([[1, 2], [3, 0]], np.int32)
BELOW_HALF = np.nextafter(np.float32(0.5), np.float32(0.0))
#            X      Y      z           I        where it goes (dz = 0.5, z_max = 2.0: five bins)
POINTS = [(0.0,   2.0,   0.5,        10),     # the raster's corner is inside: pixel (0, 0), label 1; 0.5 is the edge of bin 1
          (1.0,   2.0,   1.0,        20),     # the border of two columns belongs to the right one: pixel (0, 1), label 2, bin 2
          (2.0,   2.0,   1.0,        30),     # the right edge of the raster is outside
          (0.0,   1.0,   2.0,        40),     # the border of two rows belongs to the lower one: pixel (1, 0), label 3; z_max: bin 4
          (1.0,   1.0,   1.0,        50),     # the corner all four pixels share: pixel (1, 1), label 0: no row
          (0.5,   0.0,   1.0,        60),     # the bottom edge is outside
          (0.5,   1.5,   2.5,        70),     # label 1, one bin above the profile: out of range, its intensity counts
          (-0.0,  1.5,   -0.25,      80),     # minus zero is column 0; a negative height is out of range
          (np.nan, 1.5,  1.0,        90),     # outside
          (0.5,   np.inf, 1.0,       100),    # outside
          (0.25,  1.75,  np.nan,     0),      # label 1, NaN height: out of range
          (0.75,  1.25,  0.0,        65535),  # label 1, bin 0
          (1.5,   1.5,   BELOW_HALF, 5)]      # label 2, the float32 just below the edge: bin 0


def _tiny():
    p = np.array([(a, b) for a, b, _, _ in POINTS], np.float64)
    z = np.array([c for _, _, c, _ in POINTS], np.float32)
    inten = np.array([d for _, _, _, d in POINTS], np.uint16)
    return p[:, 0], p[:, 1], z, inten, R.invert_affine(AFFINE_2X2)


def test_the_pixel_rule_on_every_border_and_corner():
    x, y, _, _, inv = _tiny()
    assert R.pixel_of(x, y, inv, 2, 2).tolist() == [0, 1, -1, 2, 3, -1, 0, 0, -1, -1, 0, 0, 1]


def test_the_state_of_the_hand_worked_case():
    x, y, z, inten, inv = _tiny()
    st = R.segments_state(x, y, z, inten, inv, LABELS_2X2, 1, 3, 5, 0.5)
    assert st["counters"].tolist() == [4, 1, 3, 5]
    assert st["profile"].tolist() == [[1, 1, 0, 0, 0], [1, 0, 1, 0, 0], [0, 0, 0, 0, 1]]
    assert R.zunkey(st["top"]).tolist() == [0.5, 1.0, 2.0]
    assert st["n_int"].tolist() == [5, 2, 1]
    assert st["s1"].tolist() == [10 + 70 + 80 + 0 + 65535, 25, 40]
    assert st["s2"].tolist() == [100 + 4900 + 6400 + 65535 ** 2, 425, 1600]
    zk, count = R.rasters_state(x, y, z, inv, 2, 2)
    assert count.tolist() == [[5, 2], [1, 1]]
    chm, density = R.rasters_finish(zk, count, 1.0)
    assert chm.tolist() == [[2.5, 1.0], [2.0, 1.0]] and density.tolist() == [[5.0, 2.0], [1.0, 1.0]]
    zk0, count0 = R.rasters_state(x[:0], y[:0], z[:0], inv, 2, 2)
    chm0, density0 = R.rasters_finish(zk0, count0, 0.25)
    assert np.isnan(chm0).all() and (density0 == 0).all() and (zk0 == 0).all()
    # a state is added to: the cloud in two cuts
    a = R.rasters_state(x[:6], y[:6], z[:6], inv, 2, 2)
    b = R.rasters_state(x[6:], y[6:], z[6:], inv, 2, 2, *a)
    assert np.array_equal(b[0], zk) and np.array_equal(b[1], count)


def test_the_columns_of_the_hand_worked_case():
    x, y, z, inten, inv = _tiny()
    st = R.segments_state(x, y, z, inten, inv, LABELS_2X2, 1, 3, 5, 0.5)
    assert R.j0_of(0.5, 0.5, 5) == 1 and R.j0_of(1.0, 0.3, 106) == 4 and R.j0_of(-2.0, 0.5, 5) == 0 and R.j0_of(99.0, 0.5, 5) == 5
    col = R.columns(st, 0.5, min_height=0.5, k=2.0, pad=True)
    assert col["n_points"].tolist() == [2, 2, 1] and col["ch"].tolist() == [0.5, 1.0, 2.0]
    assert col["pai"][:2].tolist() == [np.log(2.0) / 2.0] * 2 and np.isnan(col["pai"][2])          # row 2: nothing below the floor
    assert col["fhd"].tolist() == [0.0, 0.0, 0.0]                                                  # one occupied bin above the floor
    assert col["mean_intensity"].tolist() == [65695 / 5, 12.5, 40.0]
    assert col["variance_intensity"][1:].tolist() == [56.25, 0.0]
    pad = col["pad"]
    assert np.isnan(pad[0, 0]) and pad[0, 1] == np.log(2.0) / (2.0 * 0.5) and pad[0, 2:].tolist() == [0.0, 0.0, 0.0]
    assert np.isnan(pad[2, :5]).all()                                                              # nothing, then the first returns
    # two occupied bins above the floor: p = 1/2 each
    st2 = dict(st, profile=np.array([[3, 2, 0, 2, 0]] * 3, np.uint32))
    col2 = R.columns(st2, 0.5, min_height=0.5, k=1.0)
    assert col2["fhd"][0] == -(0.5 * np.log(0.5) + 0.5 * np.log(0.5)) and col2["pai"][0] == np.log(7.0 / 3.0)


def test_z_on_a_bin_edge_and_at_z_max():
    z = np.array([0.0, -0.0, 0.3, 0.6, 31.7, 31.8, 1e30, np.inf, -1e-30, np.nan], np.float32)
    j = R.bins_of(z, 0.3, 106)
    # float32(0.3) is above 0.3 and float32(0.6) above 0.6: bins 1 and 2; float32(31.7) / 0.3 = 105.66; float32(31.8) is below 106 * 0.3
    assert j.tolist() == [0, 0, 1, 2, 105, 105, -1, -1, -1, -1]
    assert R.bins_of(np.array([31.800001], np.float32), 0.3, 106).tolist() == [-1]
    assert int(np.floor(31.7 / 0.3)) + 1 == 106


def test_intensity_mean_and_variance_are_numpys():
    rs = np.random.RandomState(1)
    labels = np.ones((1, 1), np.int32)
    for n in (1, 2, 37, 5000):
        inten = rs.randint(0, 65536, n).astype(np.uint16)
        x = np.full(n, 0.5)
        st = R.segments_state(x, x, np.zeros(n, np.float32), inten, [1.0, 0.0, 0.0, 1.0, 0.0, 0.0], labels, 1, 1, 1, 1.0)
        col = R.columns(st, 1.0)
        mean, var = R.exact_intensity(st)[0]
        assert R.ulps(col["mean_intensity"], [mean])[0] <= 1.0 and R.ulps(col["variance_intensity"], [var])[0] <= 4.0
        # the reference computes np.mean / np.var of the field: float64 pairwise sums, a few ulp from the exact value themselves
        assert np.isclose(col["mean_intensity"][0], np.mean(inten.astype(np.float64)), rtol=1e-13, atol=0)
        assert np.isclose(col["variance_intensity"][0], np.var(inten.astype(np.float64)), rtol=1e-11, atol=1e-9)
    empty = R.segments_state(x[:0], x[:0], np.zeros(0, np.float32), inten[:0], [1.0, 0.0, 0.0, 1.0, 0.0, 0.0], labels, 1, 1, 1, 1.0)
    col = R.columns(empty, 1.0)
    assert np.isnan(col["mean_intensity"][0]) and np.isnan(col["variance_intensity"][0])            # the "missing or empty" branch


def test_pad_telescopes_to_pai():
    c = R.base_case()
    st = R.segments_state(c["x"], c["y"], c["z"], c["intensity"], c["inv"], c["labels"], 1, R.NSEG, 106, R.DZ)
    for T, rtol in ((np.float64, 1e-12), (np.longdouble, 1e-15)):
        col = R.columns(st, R.DZ, min_height=1.0, k=0.5, dtype=T, pad=True)
        j0 = R.j0_of(1.0, R.DZ, 106)
        ok = ~np.isnan(col["pai"])
        assert ok.sum() > 40
        tel = col["pad"][ok][:, j0:].sum(1) * T(R.DZ)
        assert not np.isnan(tel).any() and np.allclose(tel.astype(np.float64), col["pai"][ok].astype(np.float64), rtol=rtol, atol=rtol)


def test_the_key_keeps_the_order_of_the_floats():
    z = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 0.3, 31.7, np.inf], np.float32)
    k = R.zkey(z)
    assert (np.diff(k.astype(np.int64)) > 0).all() and (k != 0).all()
    assert np.array_equal(R.zunkey(k).view(np.uint32), z.view(np.uint32))


# ------------------------------------------------------------------------------------------------------ refusals before the device
def _cloud(n=4, intensity=np.uint16):
    d = {"X": np.zeros(n), "Y": np.zeros(n), "HeightAboveGround": np.ones(n, np.float32)}
    if intensity is not None:
        d["Intensity"] = np.zeros(n, intensity)
    return d


def test_as_points_forms_and_refusals():
    pytest.importorskip("torch")
    from obia_amd.pointcloud import as_points
    rec = np.zeros(5, dtype=[("X", "f8"), ("Y", "f8"), ("Z", "f8"), ("HeightAboveGround", "f4"), ("Intensity", "u2")])
    rec["HeightAboveGround"], rec["Z"] = 2.0, 300.0
    p = as_points(rec)
    assert not p.is_torch and p.z.tolist() == [2.0] * 5 and p.intensity.dtype == np.uint16               # HeightAboveGround before Z
    assert as_points([rec, {"meta": 1}]).x.shape == (5,)                                               # the pyforestscan list
    assert as_points(rec[["X", "Y", "Z"]]).z.tolist() == [300.0] * 5 and as_points(rec[["X", "Y", "Z"]]).intensity is None
    assert as_points(_cloud(3, np.uint8)).intensity.dtype == np.uint8
    assert as_points(p) is p
    for bad in (np.float32, np.float64, np.int32, np.int16):
        with pytest.raises(TypeError, match="uint8 or uint16"):
            as_points(_cloud(3, bad))
    with pytest.raises(TypeError):
        as_points(np.zeros((4, 3)))
    with pytest.raises(ValueError, match="X, Y and HeightAboveGround"):
        as_points({"X": np.zeros(2), "Y": np.zeros(2)})
    with pytest.raises(ValueError, match="one length"):
        as_points({"X": np.zeros(2), "Y": np.zeros(3), "Z": np.zeros(2)})
    with pytest.raises(ValueError, match="empty"):
        as_points([])


def test_accumulators_refuse_before_the_device():
    pytest.importorskip("torch")
    from obia_amd.pointcloud import PointRasters, SegmentPoints
    labels = np.ones((3, 3), np.int32)
    for kw in (dict(dz=0.0), dict(dz=-1.0), dict(dz=float("nan")), dict(z_max=-1.0), dict(z_max=float("inf")),
               dict(affine=[1.0, 0.0, 0.0, 0.0, 0.0, 0.0]), dict(affine=[1.0, 0.0, 0.0]), dict(labels=np.ones(3, np.int32)),
               dict(labels=np.ones((0, 3), np.int32))):
        a = dict(labels=labels, affine=R.AFFINE, dz=0.5, z_max=10.0)
        a.update(kw)
        with pytest.raises(ValueError):
            SegmentPoints(a["labels"], a["affine"], a["dz"], a["z_max"])
    with pytest.raises(NotImplementedError, match="height bins"):
        SegmentPoints(labels, R.AFFINE, 0.001, 100.0)
    for shape in ((0, 4), (4,), (4, 4, 1)):
        with pytest.raises(ValueError):
            PointRasters(shape, R.AFFINE)
    with pytest.raises(ValueError, match="singular"):
        PointRasters((4, 4), [1.0, 2.0, 2.0, 4.0, 0.0, 0.0])
    acc = PointRasters((4, 4), R.AFFINE)
    assert acc.pixel_area == 0.25 and acc.total == 0
    acc.total = 2 ** 32 - 1 - 3
    with pytest.raises(OverflowError, match="2\\^32 - 1"):
        acc.add(_cloud(4))
    with pytest.raises(TypeError):
        acc.add(_cloud(2, np.float32))
    assert acc.total == 2 ** 32 - 4


class _Image:
    def __init__(self, affine=None):
        self.img_data = np.zeros((3, 3, 1), np.float32)
        if affine is not None:
            self.affine_transformation = affine


def test_create_objects_refusals():
    pytest.importorskip("torch")
    pytest.importorskip("pandas")
    import inspect
    from obia_amd.statistics import create_objects
    p = inspect.signature(create_objects).parameters["pointcloud"]
    assert p.kind is p.KEYWORD_ONLY and p.default is None
    labels, img, pc = np.ones((3, 3), np.int32), _Image(R.AFFINE), _cloud()
    disabled = "Point-cloud workflows are temporarily disabled"
    for kw in (dict(calculate_structural=True), dict(calculate_radiometric=True), dict(ept="a.json"),
               dict(ept="a.json", pointcloud=pc, voxel_resolution=(1, 1, 1), calculate_structural=True)):
        with pytest.raises(NotImplementedError, match=disabled):                       # unchanged, and ept stays refused
            create_objects(labels, img, **kw)
    for voxel in (None, (1.0, 1.0), (1.0, 1.0, 0.0), (1.0, -1.0, 0.5), (1.0, 1.0, float("nan")), 0.5):
        with pytest.raises(ValueError, match="voxel_resolution"):
            create_objects(labels, img, voxel_resolution=voxel, calculate_structural=True, pointcloud=pc)
    for image in (_Image(), np.zeros((3, 3, 1), np.float32)):
        with pytest.raises(ValueError, match="affine_transformation"):
            create_objects(labels, image, voxel_resolution=(1, 1, 0.5), calculate_structural=True, pointcloud=pc)
    with pytest.raises(ValueError, match="At least one"):
        create_objects(labels, img, calculate_spectral=False, calculate_textural=False, pointcloud=pc)


def test_public_names():
    pytest.importorskip("torch")
    from obia_amd import pointcloud
    for name in ("as_points", "PointRasters", "points_to_rasters", "SegmentPoints", "segment_point_stats"):
        assert callable(getattr(pointcloud, name))
