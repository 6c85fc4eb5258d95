"""Segments and boxes on the GPU (obia_amd.boxes, include/obia_boxes.h) against the restatement (tests/boxes_restatement.py), bit for
bit: the winner and its area per segment, the pair table, the keep mask and the IoU matrix; two runs of everything agree."""
import functools
import json

import numpy as np
import pytest

from tests import boxes_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W = 96, 128


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


def same_table(got, want):
    return list(got) == list(want) and all(same(got[k], want[k]) for k in want)


@functools.lru_cache(maxsize=None)
def scene():
    """a 96 x 128 raster of blocky random segments with label-0 background and 3001 boxes of every kind"""
    rs = np.random.RandomState(7)
    coarse = rs.randint(0, 400, (H // 4, W // 4))
    coarse[rs.rand(*coarse.shape) < 0.15] = 0
    labels = np.kron(coarse, np.ones((4, 4), np.int64))
    ragged = rs.rand(H, W) < 0.1                                   # ragged block edges: a pixel takes its left neighbour's label
    labels[:, 1:][ragged[:, 1:]] = labels[:, :-1][ragged[:, 1:]]
    labels = labels.astype(np.int32)
    boxes = []
    for i in range(3000):
        kind = i % 8
        w, h = rs.uniform(0.3, 14, 2)
        x0, y0 = rs.uniform(0, W - 1), rs.uniform(0, H - 1)
        if kind == 1:                                              # integer-aligned
            x0, y0, w, h = [float(v) for v in (rs.randint(0, W - 8), rs.randint(0, H - 8), rs.randint(1, 9), rs.randint(1, 9))]
        elif kind == 2:                                            # inside one column
            x0, w = np.floor(x0) + rs.uniform(0, 0.5), rs.uniform(0, 0.5)
        elif kind == 3:                                            # inside one row
            y0, h = np.floor(y0) + rs.uniform(0, 0.5), rs.uniform(0, 0.5)
        elif kind == 4:                                            # zero width, on a pixel edge every other time
            x0, w = (np.floor(x0) if i % 16 == 4 else x0), 0.0
        elif kind == 5:                                            # partly off the raster
            x0, y0 = rs.choice([-5.5, -1.0, x0, W - 2.25]), rs.choice([-3.0, y0, H - 0.5, H - 1.0])
        elif kind == 6:                                            # wholly off the raster, or touching its edge from outside
            x0, y0 = rs.choice([-40.0, W + 0.0, W + 3.5, -w]), rs.choice([-30.0, H + 2.0, y0])
        boxes.append([x0, y0, x0 + w, y0 + h])
        if kind == 7:                                              # a duplicate of an earlier box: ties
            boxes[-1] = list(boxes[rs.randint(0, len(boxes) - 1)])
    boxes.append([20.5, 30.25, 60.5, 70.25])                       # 40 x 40: a footprint of several strides of the workgroup
    boxes = np.array(boxes, np.float64)
    assert np.isfinite(boxes).all() and (boxes[:, 0] <= boxes[:, 2]).all() and (boxes[:, 1] <= boxes[:, 3]).all()
    return labels, boxes


@functools.lru_cache(maxsize=None)
def scene_reference(n_labels=None):
    labels, boxes = scene()
    return R.pair_table(labels, boxes, n_labels), R.assign(labels, boxes, n_labels)


def test_assignment_and_pair_table_of_mixed_boxes():
    from obia_amd import assign_boxes, box_overlaps
    labels, boxes = scene()
    table, (assigned, area) = scene_reference()
    assert (assigned >= 0).sum() > 200 and (assigned[1:] < 0).any() and (table["area"] == 0).any() and len(table["box"]) > 5000
    dl, db = torch.as_tensor(labels).cuda(), torch.as_tensor(boxes).cuda()
    runs = []
    for _ in range(2):
        got = assign_boxes(dl, None, db, pixel=True)
        assert got.assigned.is_cuda and same(got.assigned.cpu().numpy(), assigned) and same(got.area.cpu().numpy(), area)
        pairs = box_overlaps(dl, db)
        assert same_table({k: v.cpu().numpy() for k, v in pairs.items()}, table)
        runs.append((got.assigned.cpu().numpy().tobytes(), got.area.cpu().numpy().tobytes(), [v.cpu().numpy().tobytes() for v in pairs.values()]))
    assert runs[0] == runs[1]
    host = assign_boxes(labels, None, boxes, pixel=True)           # NumPy in, NumPy out
    assert isinstance(host.assigned, np.ndarray) and same(host.assigned, assigned) and same(host.area, area)
    assert assign_boxes(labels, None, boxes, pixel=True, as_array=True).area.is_cuda


def test_n_labels_smaller_than_the_largest_id():
    from obia_amd import assign_boxes, box_overlaps
    labels, boxes = scene()
    table, (assigned, area) = scene_reference(200)
    assert labels.max() > 200 and len(assigned) == 201
    got = assign_boxes(labels, None, boxes, n_labels=200, pixel=True)
    assert same(got.assigned, assigned) and same(got.area, area)
    assert same_table(box_overlaps(labels, boxes, n_labels=200), table)


def test_map_bounds_are_divided_into_pixel_boxes():
    from obia_amd import assign_boxes
    from obia_amd.boxes import map_to_pixel
    labels, boxes = scene()
    affine = [0.25, 0.0, 0.0, -0.25, 431000.0, 5012350.0]
    rs = np.random.RandomState(8)
    bounds = np.stack([431000.0 + 0.25 * boxes[:400, 0], 5012350.0 - 0.25 * boxes[:400, 3], 431000.0 + 0.25 * boxes[:400, 2] + rs.uniform(0, 0.1, 400),
                       5012350.0 - 0.25 * boxes[:400, 1]], 1)
    px = map_to_pixel(bounds, affine)
    want = R.assign(labels, px)

    class Frame:
        pass
    frame = Frame()
    frame.bounds = bounds
    for b in (bounds, frame):
        got = assign_boxes(labels, affine, b)
        assert same(got.assigned, want[0]) and same(got.area, want[1])


@pytest.mark.parametrize("scale", [1, 4096], ids=["dense-ids", "ids-multiples-of-4096"])
def test_a_footprint_with_more_labels_than_the_table_is_split_into_passes(scale):
    """every pixel its own label under one box that covers the raster: the labels exceed the table twice over, and with ids that are
    all multiples of 4096 the passes P = 2 .. 4096 split nothing"""
    from obia_amd import _lib, assign_boxes, box_overlaps
    side = 47
    assert side * side > 2 * _lib.BOXES_TABLE
    labels = (scale * np.arange(1, side * side + 1, dtype=np.int64)).reshape(side, side).astype(np.int32)
    boxes = np.array([[3.3, 2.2, 40.7, 44.1], [-0.5, -0.5, side + 0.5, side + 0.5], [10.0, 10.0, 12.0, 12.0]])
    want_table, want = R.pair_table(labels, boxes), R.assign(labels, boxes)
    runs = []
    for _ in range(2):
        got = assign_boxes(labels, None, boxes, pixel=True)
        assert same(got.assigned, want[0]) and same(got.area, want[1])
        pairs = box_overlaps(labels, boxes)
        assert same_table(pairs, want_table)
        runs.append((got.assigned.tobytes(), got.area.tobytes(), [v.tobytes() for v in pairs.values()]))
    assert runs[0] == runs[1]
    assert (want[0][labels[5, 5]], want[0][labels[0, 0]], want[0][labels[11, 11]]) == (0, 1, 0)


def test_a_workgroup_goes_on_to_its_next_box_after_a_walk_that_did_not_fit():
    """more boxes than workgroups of a launch (4096), so that workgroups 0 .. 119 take a second box: the first of each does not fit
    the table, the second is small or does not fit either"""
    from obia_amd import _lib, assign_boxes, box_overlaps
    side = 47
    labels = np.arange(1, side * side + 1, dtype=np.int32).reshape(side, side)
    rs = np.random.RandomState(21)
    n = 4096 + 120
    xy = rs.uniform(0, side - 2, (n, 2))
    boxes = np.concatenate([xy, xy + rs.uniform(0.1, 1.5, (n, 2))], 1)                   # a few pixels each
    big = np.r_[0:120, 4096:4216:3]
    xy = rs.uniform(0, side - 20, (len(big), 2))
    boxes[big] = np.concatenate([xy, xy + rs.uniform(17.5, 19.5, (len(big), 2))], 1)     # 18 x 18 pixels and more, each its own label
    assert 18 * 18 > _lib.BOXES_TABLE
    want_table, want = R.pair_table(labels, boxes), R.assign(labels, boxes)
    runs = []
    for _ in range(2):
        got = assign_boxes(labels, None, boxes, pixel=True)
        assert same(got.assigned, want[0]) and same(got.area, want[1])
        pairs = box_overlaps(labels, boxes)
        assert same_table(pairs, want_table)
        runs.append((got.assigned.tobytes(), got.area.tobytes(), [v.tobytes() for v in pairs.values()]))
    assert runs[0] == runs[1]


def test_a_segment_only_touched_goes_to_the_first_touching_box_with_area_zero():
    from obia_amd import assign_boxes, box_overlaps
    labels = np.zeros((6, 6), np.int32)
    labels[2, 2] = 7                                               # the square [2, 3] x [2, 3]
    labels[0, 0] = 3
    boxes = np.array([[4.0, 4.0, 5.5, 5.5], [3.0, 3.0, 5.0, 5.0], [0.5, 3.0, 2.5, 4.0], [3.0, 0.0, 4.0, 6.0]])   # none; corner; edge; edge
    got = assign_boxes(labels, None, boxes, pixel=True)
    assert got.assigned.tolist() == [-1, -1, -1, -1, -1, -1, -1, 1] and got.area.tolist() == [0.0] * 8
    pairs = box_overlaps(labels, boxes)
    assert pairs["box"].tolist() == [1, 2, 3] and pairs["segment"].tolist() == [7, 7, 7] and pairs["area"].tolist() == [0.0] * 3
    assert same(got.assigned, R.assign(labels, boxes)[0])
    none = box_overlaps(labels, boxes[:1])                         # no pair at all: an empty table
    assert all(len(v) == 0 for v in none.values()) and none["area"].dtype == np.float64


def test_dissolve_then_polygonize_merges_the_segments_of_one_box():
    from obia_amd import assign_boxes, dissolve_by_box, polygonize
    labels = np.array([[1, 1, 1, 2, 2, 2, 3, 3]] * 4 + [[4] * 8], np.int32)
    boxes = np.array([[0.5, 0.5, 5.5, 3.5], [6.2, 0.0, 7.9, 2.0]])
    got = assign_boxes(labels, None, boxes, pixel=True)
    assert got.assigned.tolist() == [-1, 0, 0, 1, -1]
    crowns = dissolve_by_box(labels, got.assigned)
    assert crowns.dtype == np.int32 and same(crowns, R.dissolve(labels, got.assigned))
    assert crowns[0].tolist() == [1, 1, 1, 1, 1, 1, 2, 2] and crowns[4].tolist() == [0] * 8
    t = polygonize(crowns, start_label=1)
    assert np.asarray(t.labels).tolist() == [1, 2] and len(t.ring_label) == 2 and not np.asarray(t.ring_is_hole).any()
    ring = np.asarray(t.xy)[int(t.ring_offset[0]):int(t.ring_offset[1])]
    assert ring.min(0).tolist() == [0.0, 0.0] and ring.max(0).tolist() == [6.0, 4.0]      # segments 1 and 2 as one rectangle
    dev = dissolve_by_box(torch.as_tensor(labels).cuda(), torch.as_tensor(got.assigned).cuda())
    assert dev.is_cuda and same(dev.cpu().numpy(), crowns)


# --------------------------------------------------------------------------------------------------------------- IoU and NMS
def test_iou_matrix_is_the_reference_formula_bit_for_bit():
    from obia_amd import box_iou
    rs = np.random.RandomState(3)
    a = np.concatenate([rs.uniform(0, 50, (30, 2)), rs.uniform(0, 30, (30, 2))], 1)
    a[:, 2:] += a[:, :2]
    b = np.concatenate([rs.uniform(0, 50, (41, 2)), rs.uniform(0, 30, (41, 2))], 1)
    b[:, 2:] += b[:, :2]
    b[:5] = a[:5]                                                  # identical boxes
    b[5] = [a[6, 2], a[6, 1], a[6, 2] + 4, a[6, 3]]                # touching
    b[6] = [-0.0, 0.0, 0.0, -0.0]                                  # degenerate, signed zeros
    b[7] = [30.0, 30.0, 10.0, 10.0]                                # reversed corners: the formula is applied as it is
    want = R.iou_matrix(a, b)
    assert (want > 0).sum() > 100 and (want == 0).sum() > 100
    for _ in range(2):
        assert same(box_iou(a, b), want)
    dev = box_iou(torch.as_tensor(a).cuda(), torch.as_tensor(b).cuda())
    assert dev.is_cuda and same(dev.cpu().numpy(), want)
    a32 = a.astype(np.float32)                                     # float32 tables are widened
    assert same(box_iou(a32, b), R.iou_matrix(a32.astype(np.float64), b))
    assert same(box_iou(a[:1], b[:1]), want[:1, :1])


def check_nms(boxes, scores, thr, groups=None):
    from obia_amd import box_nms
    want_keep, want_kept = R.nms(boxes, scores, thr, groups)
    out = []
    for _ in range(2):
        keep, kept = box_nms(boxes, scores, thr, groups)
        assert keep.dtype == np.bool_ and same(keep, want_keep) and same(kept, want_kept)
        out.append(keep.tobytes() + kept.tobytes())
    assert out[0] == out[1]
    return want_keep


def test_nms_known_orders():
    a, b, c = [0, 0, 10, 10], [5, 0, 15, 10], [10, 0, 20, 10]
    chain = np.array([a, b, [9, 0, 19, 10]], np.float64)            # a suppresses b; b would have suppressed c, but is gone
    assert R.calculate_iou(chain[1], chain[2]) > 0.3 > R.calculate_iou(chain[0], chain[2]) > 0
    assert check_nms(chain, [0.9, 0.8, 0.7], 0.3).tolist() == [True, False, True]
    assert check_nms(chain, [0.7, 0.8, 0.9], 0.3).tolist() == [True, False, True]      # the other way round: c, not b, then a
    assert check_nms(chain, [0.5, 0.5, 0.5], 0.3).tolist() == [True, False, True]      # equal scores: the earlier row first
    exact = R.calculate_iou(a, b)
    assert check_nms(np.array([a, b], np.float64), [0.9, 0.8], exact).tolist() == [True, True]       # equal to the threshold: kept
    assert check_nms(np.array([a, b], np.float64), [0.9, 0.8], np.nextafter(exact, 0)).tolist() == [True, False]
    assert check_nms(np.array([a, b, c], np.float64), [0.9, 0.8, 0.7], 0.0).tolist() == [True, False, True]   # touching is not overlap
    assert check_nms(chain, [0.9, 0.8, 0.7], 0.3, groups=np.array([4, 9, 4])).tolist() == [True, True, True]
    assert check_nms(chain, [0.9, 0.8, 0.7], 0.3, groups=np.array([4, 4, 9])).tolist() == [True, False, True]
    assert check_nms(np.array([a], np.float64), [0.1], 0.5).tolist() == [True]                    # n = 1
    same_box = np.tile(np.array([[3.5, 4.5, 20.0, 30.0]]), (300, 1))                              # all identical: the first stays
    keep = check_nms(same_box, np.linspace(0, 1, 300), 0.5)
    assert keep.sum() == 1 and keep[299]
    long_chain = np.array([[4.0 * i, 0.0, 4.0 * i + 10.0, 10.0] for i in range(40)])              # every box waits for the one before
    assert check_nms(long_chain, -np.arange(40.0), 0.4).sum() == 20


def test_nms_of_random_boxes_of_many_sizes():
    rs = np.random.RandomState(11)
    n = 2000
    xy = rs.uniform(0, 400, (n, 2))
    wh = np.exp(rs.uniform(np.log(0.5), np.log(60), (n, 2)))       # sides from half a unit to 60: many span several cells of the small ones
    boxes = np.concatenate([xy, xy + wh], 1)
    boxes[17] = [100.0, 100.0, 190.0, 130.0]                       # the largest side
    boxes[100:140] = boxes[60:100] + rs.uniform(-0.5, 0.5, (40, 4)) * [1, 1, 0, 0]      # near copies
    boxes[:, 2:] = np.maximum(boxes[:, 2:], boxes[:, :2])
    scores = rs.uniform(0, 1, n)
    scores[200:260] = scores[300]                                  # ties
    scores[17] = 2.0                                               # the largest box is first: it suppresses across several cells
    groups = rs.randint(0, 3, n)
    keep = check_nms(boxes, scores, 0.15)
    assert 40 < keep.sum() < n - 40 and keep[17]
    keep_g = check_nms(boxes, scores, 0.15, groups)
    assert not np.array_equal(keep_g, keep)
    from obia_amd import box_nms
    dk, dkept = box_nms(torch.as_tensor(boxes).cuda(), torch.as_tensor(scores).cuda(), 0.15)
    assert dk.is_cuda and dk.dtype == torch.bool and same(dk.cpu().numpy(), keep) and dkept.dtype == torch.int64


def test_mosaic_keeps_one_copy_of_a_box_seen_in_four_tiles(tmp_path):
    from obia_amd import assign_boxes, mosaic_predictions
    from obia_amd.training import tile_windows
    affine = [0.5, 0.0, 0.0, -0.5, 1000.0, 2000.0]
    windows, transforms = tile_windows((100, 100), affine, 30.0, 15.0)      # 60-pixel tiles every 30 pixels
    names = [f"img_{i:03d}.jpg" for i in range(len(windows))]
    tree = (1016.0, 1974.5, 1019.5, 1978.0)                        # map bounds (minx, miny, maxx, maxy): columns 32 .. 39, rows 44 .. 51
    lone = (1002.0, 1995.0, 1004.0, 1998.0)                        # columns 4 .. 8, rows 4 .. 10: reported by one tile only
    per_tile, seen = {}, [0, 0]
    for (r0, c0, h, w), t, name in zip(windows, transforms, names):
        rows = {"xmin": [], "ymin": [], "xmax": [], "ymax": [], "score": []}
        for k, (minx, miny, maxx, maxy) in enumerate((tree, lone)):
            x0, x1 = (minx - t[2]) / t[0], (maxx - t[2]) / t[0]
            y0, y1 = (maxy - t[5]) / t[4], (miny - t[5]) / t[4]
            if x0 >= 0 and y0 >= 0 and x1 <= w and y1 <= h and not (k == 1 and seen[1]):
                for key, v in zip(rows, (x0, y0, x1, y1, 0.5 + 0.01 * len(per_tile) - 0.2 * k)):
                    rows[key].append(v)
                seen[k] += 1
        per_tile[name] = rows
    assert seen == [4, 1]
    transforms_json = {n: {"transform": t, "crs": "EPSG:32610"} for n, t in zip(names, transforms)}
    table = mosaic_predictions(per_tile, transforms_json)
    assert table.bounds.tolist() == [list(tree), list(lone)] and len(table.score) == 2 and table.label == ["Tree", "Tree"]
    assert table.score[0] == max(max(p["score"], default=0) for p in per_tile.values())
    path = tmp_path / "transforms.json"                             # the same from the file tile_and_process writes
    path.write_text(json.dumps(transforms_json))
    from_file = mosaic_predictions(per_tile, str(path))
    assert from_file.bounds.tolist() == table.bounds.tolist() and from_file.tile == table.tile and same(from_file.score, table.score)
    every = mosaic_predictions(per_tile, transforms_json, iou_threshold=1.0)
    assert len(every.score) == 5
    assert len(mosaic_predictions(per_tile, transforms_json, score_threshold=0.4).score) == 1
    labels = np.arange(1, 10001, dtype=np.int32).reshape(100, 100)
    got = assign_boxes(labels, affine, table)                      # the table's .bounds is what assign_boxes takes
    assert got.assigned[labels[47, 35]] == 0 and got.assigned[labels[5, 5]] == 1 and got.assigned[labels[60, 60]] == -1
