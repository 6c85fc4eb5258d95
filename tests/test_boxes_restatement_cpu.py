"""Segments and boxes without a GPU: the restatement (tests/boxes_restatement.py) against an exact oracle and hand-checked answers,
the argument checks of obia_amd.boxes that fire before the device is touched, and the host glue (predictions_to_map,
save_predictions_to_gpkg)."""
import json
import os

import numpy as np
import pytest

from tests import boxes_restatement as R

# Every term of the area is fl(fl(wx * wy) * n) with wx and wy one rounded subtraction each: four roundings, (1 + u)^4, u = 2^-53.
# The nine non-negative terms are added with at most eight rounded additions, (1 + u)^8.  (1 + u)^12 - 1 < 16 u.
AREA_RTOL = 16 * 2.0 ** -53


def _random_case(rs):
    H, W = int(rs.randint(3, 10)), int(rs.randint(3, 12))
    labels = rs.randint(0, 6, (H, W)).astype(np.int32)
    kind = rs.randint(0, 4)
    if kind == 0:                                                  # fractional
        x = np.sort(rs.uniform(-1.5, W + 1.5, 2))
        y = np.sort(rs.uniform(-1.5, H + 1.5, 2))
    elif kind == 1:                                                # integer-aligned
        x = np.sort(rs.randint(-1, W + 2, 2)).astype(np.float64)
        y = np.sort(rs.randint(-1, H + 2, 2)).astype(np.float64)
    elif kind == 2:                                                # inside one column, any rows
        c = rs.randint(0, W)
        x = c + np.sort(rs.uniform(0, 1, 2))
        y = np.sort(rs.uniform(-1.5, H + 1.5, 2))
    else:                                                          # one side on a pixel edge, the other not
        x = np.array([float(rs.randint(0, W)), rs.uniform(0, W + 1)])
        x.sort()
        y = np.sort(rs.uniform(0, H, 2))
    return labels, np.array([x[0], y[0], x[1], y[1]])


def test_the_restatement_is_within_the_derived_bound_of_the_exact_area():
    rs = np.random.RandomState(20261020)
    pairs = positive = 0
    for _ in range(240):
        labels, box = _random_case(rs)
        got = R.pairs_of_box(labels, box, 5)
        exact = R.exact_areas(labels, box, 5)
        assert set(got) == set(exact)                              # the pairs are the segments whose pixels meet the closed box
        for seg, (area, meets) in got.items():
            want = exact[seg]
            assert meets >= 1 and area >= 0.0
            assert abs(R.Fraction(area) - want) <= R.Fraction(AREA_RTOL) * want, (box, seg, area, float(want))
            pairs += 1
            positive += want > 0
    assert pairs > 600 and positive > 300 and pairs - positive > 20   # areas of both kinds: positive, and exactly 0


def test_a_box_inside_one_pixel():
    labels = np.arange(1, 10, dtype=np.int32).reshape(3, 3)
    t = R.pair_table(labels, [[1.25, 1.25, 1.75, 1.5]])
    assert t["box"].tolist() == [0] and t["segment"].tolist() == [5] and t["meets"].tolist() == [1]
    assert t["area"].tolist() == [0.125]                           # 0.5 x 0.25, exact in binary
    assigned, area = R.assign(labels, [[1.25, 1.25, 1.75, 1.5]])
    assert assigned.tolist() == [-1, -1, -1, -1, -1, 0, -1, -1, -1, -1] and area[5] == 0.125 and area.sum() == 0.125


def test_an_integer_aligned_box_is_only_touched_by_its_neighbours():
    labels = np.arange(1, 10, dtype=np.int32).reshape(3, 3)
    t = R.pair_table(labels, [[1.0, 1.0, 2.0, 2.0]])
    assert t["segment"].tolist() == list(range(1, 10)) and t["meets"].tolist() == [1] * 9
    assert t["area"].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    assigned, _ = R.assign(labels, [[1.0, 1.0, 2.0, 2.0]])
    assert assigned.tolist() == [-1] + [0] * 9                     # touching is a pair: area 0, the first box


def test_a_segment_with_a_hole_around_the_box_has_no_pair():
    labels = np.ones((5, 5), np.int32)
    labels[1:4, 1:4] = 2
    t = R.pair_table(labels, [[1.5, 1.5, 3.5, 3.5]])
    assert t["segment"].tolist() == [2] and t["area"].tolist() == [4.0] and t["meets"].tolist() == [9]
    assigned, area = R.assign(labels, [[1.5, 1.5, 3.5, 3.5]])
    assert assigned.tolist() == [-1, -1, 0] and area.tolist() == [0.0, 0.0, 4.0]
    assert R.dissolve(labels, assigned)[2, 2] == 1 and R.dissolve(labels, assigned)[0, 0] == 0


def test_restated_nms_and_iou_known_answers():
    a, b, c = [0, 0, 10, 10], [5, 0, 15, 10], [10, 0, 20, 10]      # a and b overlap by half, b and c too, a and c only touch
    assert R.calculate_iou(a, b) == 50 / (150 + 1e-6) and R.calculate_iou(a, c) == 0.0
    keep, kept = R.nms([a, b, c], [0.9, 0.8, 0.7], 0.3)
    assert keep.tolist() == [True, False, True] and kept.tolist() == [0, 2]      # b is gone, so it does not suppress c
    keep, _ = R.nms([a, b, c], [0.9, 0.8, 0.7], R.calculate_iou(a, b))
    assert keep.tolist() == [True, True, True]                     # "greater than": a threshold equal to the IoU keeps
    keep, _ = R.nms([a, b, c], [0.9, 0.8, 0.7], 0.3, groups=[0, 1, 0])
    assert keep.tolist() == [True, True, True]


def test_public_names():
    import obia_amd
    from obia_amd import boxes
    for name in ("box_overlaps", "assign_boxes", "dissolve_by_box", "box_iou", "box_nms", "predictions_to_map", "save_predictions_to_gpkg",
                 "mosaic_predictions", "BoxAssignment"):
        assert getattr(obia_amd, name) is getattr(boxes, name)
    assert boxes.BoxAssignment._fields == ("assigned", "area")


# --------------------------------------------------------------------------------------------- checks before the device is used
@pytest.fixture()
def no_device(monkeypatch):
    """Any use of the library fails the test."""
    from obia_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device library was used")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "default_context", boom)


LAB = np.ones((4, 5), np.int32)
NORTH_UP = [0.5, 0.0, 0.0, -0.5, 100.0, 200.0]


def test_overlap_arguments_are_checked_before_device_use(no_device):
    pytest.importorskip("torch")
    from obia_amd import boxes as B
    ok = np.array([[0.0, 0.0, 1.0, 1.0]])
    for call in (B.box_overlaps, lambda lab, bx, **k: B.assign_boxes(lab, None, bx, pixel=True, **k)):
        with pytest.raises(ValueError, match=r"\(n, 4\) table"):
            call(LAB, np.zeros((3, 5)))
        with pytest.raises(ValueError, match=r"\(n, 4\) table"):
            call(LAB, np.zeros(4))
        with pytest.raises(ValueError, match="no boxes"):
            call(LAB, np.zeros((0, 4)))
        with pytest.raises(ValueError, match="must be finite"):
            call(LAB, np.array([[0.0, 0.0, np.inf, 1.0]]))
        with pytest.raises(ValueError, match="must be finite"):
            call(LAB, np.array([[0.0, np.nan, 1.0, 1.0]]))
        with pytest.raises(ValueError, match="x0 <= x1"):
            call(LAB, np.array([[2.0, 0.0, 1.0, 1.0]]))
        with pytest.raises(ValueError, match="x0 <= x1"):
            call(LAB, np.array([[0.0, 1.5, 1.0, 1.0]]))
        with pytest.raises(ValueError, match=r"\(H, W\) raster"):
            call(np.ones((2, 3, 4), np.int32), ok)
        with pytest.raises(ValueError, match=r"\(H, W\) raster"):
            call(np.ones((0, 3), np.int32), ok)
        with pytest.raises(ValueError, match="n_labels"):
            call(LAB, ok, n_labels=-1)
        with pytest.raises(ValueError, match="n_labels"):
            call(LAB, ok, n_labels=2.5)


def test_the_transform_must_be_north_up(no_device):
    pytest.importorskip("torch")
    from obia_amd import boxes as B
    bounds = np.array([[100.0, 198.0, 101.0, 199.0]])
    for bad in ([0.5, 0.1, 0.0, -0.5, 0, 0], [0.5, 0.0, 0.2, -0.5, 0, 0], [-0.5, 0, 0, -0.5, 0, 0], [0.5, 0, 0, 0.5, 0, 0]):
        with pytest.raises(ValueError, match="north-up"):
            B.assign_boxes(LAB, bad, bounds)
    with pytest.raises(ValueError, match="six values"):
        B.assign_boxes(LAB, None, bounds)
    with pytest.raises(ValueError, match=r"\(N, 4\) table of polygon bounds"):
        B.assign_boxes(LAB, NORTH_UP, np.zeros((2, 3)))
    # plain division, in float64: x0 = (minx - xoff) / a, y0 = (maxy - yoff) / e, ...
    px = B.map_to_pixel(bounds, NORTH_UP)
    assert px.tolist() == [[(100.0 - 100.0) / 0.5, (199.0 - 200.0) / -0.5, (101.0 - 100.0) / 0.5, (198.0 - 200.0) / -0.5]]

    class Frame:
        bounds = np.array([[100.0, 198.0, 101.0, 199.0]])
    with pytest.raises(ValueError, match="n_labels"):               # .bounds is taken, and the next check fires
        B.assign_boxes(LAB, NORTH_UP, Frame(), n_labels=-3)


def test_nms_iou_and_dissolve_arguments_are_checked_before_device_use(no_device):
    torch = pytest.importorskip("torch")
    from obia_amd import boxes as B
    bx = np.array([[0.0, 0.0, 1.0, 1.0], [0.5, 0.0, 1.5, 1.0]])
    with pytest.raises(ValueError, match="scores contain NaN"):
        B.box_nms(bx, [0.5, float("nan")], 0.3)
    with pytest.raises(ValueError, match="one length"):
        B.box_nms(bx, [0.5], 0.3)
    with pytest.raises(ValueError, match="one length"):
        B.box_nms(bx, [0.5, 0.4], 0.3, groups=[1, 2, 3])
    with pytest.raises(ValueError, match="iou_threshold"):
        B.box_nms(bx, [0.5, 0.4], -0.1)
    with pytest.raises(ValueError, match="iou_threshold"):
        B.box_nms(bx, [0.5, 0.4], float("nan"))
    with pytest.raises(ValueError, match="must be finite"):
        B.box_nms(np.array([[0.0, 0.0, np.inf, 1.0]]), [0.5], 0.3)
    with pytest.raises(ValueError, match="x0 <= x1"):
        B.box_nms(np.array([[0.0, 2.0, 1.0, 1.0]]), [0.5], 0.3)
    with pytest.raises(ValueError, match=r"\(n, 4\) table"):
        B.box_iou(np.zeros((2, 3)), bx)
    with pytest.raises(ValueError, match="no boxes"):
        B.box_iou(bx, np.zeros((0, 4)))
    with pytest.raises(ValueError, match="assigned must be"):
        B.dissolve_by_box(LAB, np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError, match="assigned must be"):
        B.dissolve_by_box(LAB, np.zeros(0, np.int32))
    with pytest.raises(ValueError, match="must live on the GPU"):
        B.box_overlaps(torch.ones(4, 5, dtype=torch.int32), bx)
    with pytest.raises(ValueError, match="must live on the GPU"):
        B.box_nms(torch.zeros(2, 4, dtype=torch.float64), [0.5, 0.4], 0.3)

    class Huge:
        shape = (2 ** 31, 4)
    with pytest.raises(ValueError, match="fewer than 2\\^31 rows"):
        B.box_iou(Huge(), bx)


# ------------------------------------------------------------------------------------------------------------------ host glue
TILE = {"transform": [0.5, 0.0, 431000.0, 0.0, -0.5, 5012350.0], "crs": "EPSG:32610"}
PRED = {"xmin": [10, 40.5], "ymin": [20, 3.25], "xmax": [30, 60.0], "ymax": [44, 9.0], "label": ["Tree", "Snag"], "score": [0.9, 0.25]}


def test_predictions_to_map_takes_the_four_corners_in_the_reference_order():
    from obia_amd.boxes import predictions_to_map
    rings = predictions_to_map(np.array([[10, 20, 30, 44]]), TILE["transform"])
    a, b, c, d, e, f = TILE["transform"]
    corner = lambda col, row: [col * a + row * b + c, col * d + row * e + f]   # noqa: E731  (tile_affine * (col, row))
    assert rings.shape == (1, 5, 2)
    assert rings[0].tolist() == [corner(10, 20), corner(30, 20), corner(30, 44), corner(10, 44), corner(10, 20)]
    rot = [0.3, 0.4, 7.0, -0.4, 0.3, 9.0]                                       # a rotated tile is mapped too
    r = predictions_to_map(np.array([[1.5, 2.0, 4.0, 8.5]]), rot)[0]
    assert r[2].tolist() == [4.0 * 0.3 + 8.5 * 0.4 + 7.0, 4.0 * -0.4 + 8.5 * 0.3 + 9.0]


def test_save_predictions_round_trip_and_the_two_skips(tmp_path, capsys):
    from obia_amd.boxes import predictions_to_map, save_predictions_to_gpkg
    from obia_amd.geopackage import read_geopackage, wkb_rings
    transforms = {"img_007.jpg": TILE}
    out = str(tmp_path / "pred.gpkg")
    assert save_predictions_to_gpkg(PRED, "img_007.jpg", transforms, out) == out
    wkbs, cols, srs = read_geopackage(out, table="predictions")
    assert srs == 32610 and cols["label"] == ["Tree", "Snag"] and cols["score"] == [0.9, 0.25]
    boxes = np.array([PRED[k] for k in ("xmin", "ymin", "xmax", "ymax")], np.float64).T
    want = predictions_to_map(boxes, TILE["transform"])
    for w, ring in zip(wkbs, want):
        (rings,) = wkb_rings(w)
        assert len(rings) == 1 and np.array_equal(rings[0], ring)
    # the same from the path of transforms.json, without the optional columns
    path = str(tmp_path / "transforms.json")
    with open(path, "w") as f:
        json.dump(transforms, f)
    bare = {k: PRED[k] for k in ("xmin", "ymin", "xmax", "ymax")}
    out2 = str(tmp_path / "bare.gpkg")
    assert save_predictions_to_gpkg(bare, "img_007.jpg", path, out2) == out2
    _, cols, _ = read_geopackage(out2, table="predictions")
    assert cols["label"] == ["Tree", "Tree"] and cols["score"] == [None, None]
    # the reference's two silent skips: nothing is written
    capsys.readouterr()
    skipped = str(tmp_path / "none.gpkg")
    assert save_predictions_to_gpkg(PRED, "img_999.jpg", transforms, skipped) is None
    assert "not found in transforms.json" in capsys.readouterr().out
    empty = {k: [] for k in PRED}
    assert save_predictions_to_gpkg(empty, "img_007.jpg", transforms, skipped) is None
    assert "No predictions to save" in capsys.readouterr().out
    assert not os.path.exists(skipped)
    with pytest.raises(ValueError, match="xmin, ymin, xmax, ymax"):
        save_predictions_to_gpkg({"xmin": [1]}, "img_007.jpg", transforms, skipped)
