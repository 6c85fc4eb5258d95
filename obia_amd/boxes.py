"""Segments and detection boxes on the GPU: the last cell of the reference author's workflow (notebooks/deepfor2.ipynb, ``assign_fid``)
and the box helpers around it (obia/detection/utils.py:63-81 ``calculate_iou``, obia/utils/utils.py:70-145
``save_deepforest_predictions_to_gpkg``).

Superpixels are joined with tree boxes -- detector predictions or hand-drawn ones: every segment goes to the box it shares the most
area with, and the segments of one box are one crown.  On a label raster that needs no geometry (include/obia_boxes.h, DESIGN.md
3.5r): ``box_overlaps`` is the pair table, ``assign_boxes`` the winner of every segment, ``dissolve_by_box`` the raster of the crowns,
which goes into ``polygonize``, ``create_objects`` and ``classify`` as any label raster does.  ``box_iou`` and ``box_nms`` are the
reference's IoU and a greedy suppression with it; ``predictions_to_map``, ``save_predictions_to_gpkg`` and ``mosaic_predictions``
take the boxes a detector returns for the tiles of ``tile_and_process`` back to the map, the last one dropping the copies the
overlapping tiles produce.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out; there is no CPU path."""
import collections
import json
import struct

import numpy as np

from . import _device, _lib
from .cost import _shape
from .training import _bounds_table

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

BoxAssignment = collections.namedtuple("BoxAssignment", "assigned area")
BoxTable = collections.namedtuple("BoxTable", "bounds score label tile")
PAIR_COLUMNS = ("box", "segment", "area", "meets")


def _need_torch():
    _device.need_torch("obia_amd.boxes")


def _box_rows(boxes, what="boxes"):
    """rows of an (n, 4) table, 1 .. 2^31 - 1; touches no device"""
    s = _shape(boxes)
    if len(s) != 2 or s[1] != 4:
        raise ValueError(f"{what} must be an (n, 4) table, got shape {s}")
    if s[0] < 1:
        raise ValueError(f"{what}: no boxes")
    if s[0] >= 2 ** 31:
        raise ValueError(f"{what} must have fewer than 2^31 rows")
    return int(s[0])


def _check_boxes(boxes, what="boxes"):
    """finite and ordered: on the host for host input, before any device use; a tensor is checked where it lives"""
    b = boxes if _device.is_torch(boxes) else np.asarray(boxes, dtype=np.float64)
    xp = torch if _device.is_torch(boxes) else np
    if not bool(xp.isfinite(b).all()):
        raise ValueError(f"{what} must be finite")
    if not bool(((b[:, 0] <= b[:, 2]) & (b[:, 1] <= b[:, 3])).all()):
        raise ValueError(f"{what} must have x0 <= x1 and y0 <= y1")


def _check_labels(labels, n_labels):
    s = _shape(labels)
    if len(s) != 2 or 0 in s:
        raise ValueError(f"labels must be a non-empty (H, W) raster, got shape {s}")
    if s[0] >= 2 ** 31 or s[1] >= 2 ** 31:
        raise ValueError("labels must have fewer than 2^31 rows and columns")
    if n_labels is not None and (int(n_labels) != n_labels or not 0 <= int(n_labels) < 2 ** 31 - 1):
        raise ValueError(f"n_labels must be an integer in 0 .. 2^31 - 2, got {n_labels!r}")


def _overlap_args(labels, boxes_px, n_labels, ctx):
    _need_torch()
    _check_labels(labels, n_labels)
    n = _box_rows(boxes_px, "boxes_px")
    dev = _device.device_of(ctx, labels, boxes_px)
    if not _device.is_torch(boxes_px):
        _check_boxes(boxes_px, "boxes_px")
    lab = _device.as_dev(labels, torch.int32, dev)
    b = _device.as_dev(boxes_px, torch.float64, dev)
    if _device.is_torch(boxes_px):
        _check_boxes(b, "boxes_px")
    nl = max(0, int(lab.max())) if n_labels is None else int(n_labels)
    if nl >= 2 ** 31 - 1:
        raise ValueError("labels must be below 2^31 - 1")
    return n, dev, lab, b, nl


def box_overlaps(labels, boxes_px, n_labels=None, ctx=None):
    """The pair table of a label raster and axis-aligned boxes: a dict of ``box`` (int32), ``segment`` (int32), ``area`` (float64) and
    ``meets`` (int32: the segment's pixels whose closed square meets the closed box), one row per (box, segment) that meet, sorted
    by (box, segment).  ``boxes_px``: (n, 4) ``(x0, y0, x1, y1)`` in pixel-corner coordinates, pixel (r, c) being the square
    [c, c + 1] x [r, r + 1]; finite, x0 <= x1, y0 <= y1.  Ids outside 1 .. ``n_labels`` (default: the largest id) are background.
    The area is exact up to the rounding of nine products and eight additions (include/obia_boxes.h); a pair that only touches has
    area 0, as shapely's ``intersects`` is true for it."""
    n, dev, lab, b, nl = _overlap_args(labels, boxes_px, n_labels, ctx)
    is_t = _device.is_torch(labels)
    H, W = lab.shape
    lib, c = _device.begin(dev, ctx)
    count = torch.empty(n, dtype=torch.int64, device=lab.device)
    passes = torch.empty(n, dtype=torch.int32, device=lab.device)
    _lib.check(lib.obia_boxes_pair_count_dev(c.handle, lab.data_ptr(), H, W, b.data_ptr(), n, nl, count.data_ptr(), passes.data_ptr()))
    offset = torch.cumsum(count, 0) - count
    total = int(count.sum())
    box = torch.empty(total, dtype=torch.int32, device=lab.device)
    seg = torch.empty(total, dtype=torch.int32, device=lab.device)
    area = torch.empty(total, dtype=torch.float64, device=lab.device)
    meets = torch.empty(total, dtype=torch.int32, device=lab.device)
    if total:
        torch.cuda.current_stream(dev).synchronize()
        _lib.check(lib.obia_boxes_pair_write_dev(c.handle, lab.data_ptr(), H, W, b.data_ptr(), n, nl, offset.data_ptr(), passes.data_ptr(),
                                                 total, box.data_ptr(), seg.data_ptr(), area.data_ptr(), meets.data_ptr()))
        order = torch.sort(box.to(torch.int64) * (nl + 1) + seg.to(torch.int64)).indices     # no two rows share a key
        box, seg, area, meets = box[order], seg[order], area[order], meets[order]
    return _device.out(dict(zip(PAIR_COLUMNS, (box, seg, area, meets))), is_t)


def _north_up(affine_transformation):
    if affine_transformation is None or len(affine_transformation) != 6:
        raise ValueError("affine_transformation must hold six values [a, b, d, e, xoff, yoff]")
    a, b, d, e, xoff, yoff = [float(v) for v in affine_transformation]
    if b != 0.0 or d != 0.0 or not a > 0.0 or not e < 0.0:
        raise ValueError(f"assign_boxes takes a north-up transform (b = d = 0, a > 0, e < 0), got {list(affine_transformation)!r}")
    return a, e, xoff, yoff


def map_to_pixel(bounds, affine_transformation):
    """Map bounds ``(minx, miny, maxx, maxy)`` -> pixel-corner boxes ``(x0, y0, x1, y1)`` under a north-up transform, in float64 by
    plain division: x0 = (minx - xoff) / a, x1 = (maxx - xoff) / a, y0 = (maxy - yoff) / e, y1 = (miny - yoff) / e."""
    a, e, xoff, yoff = _north_up(affine_transformation)
    t = np.asarray(bounds, dtype=np.float64)
    return np.stack([(t[:, 0] - xoff) / a, (t[:, 3] - yoff) / e, (t[:, 2] - xoff) / a, (t[:, 1] - yoff) / e], 1)


def assign_boxes(labels, affine_transformation, boxes, n_labels=None, *, pixel=False, as_array=False, ctx=None):
    """``assign_fid`` of the reference's notebook: the box every segment shares the most area with.

    ``boxes``: an (n, 4) table of map bounds ``(minx, miny, maxx, maxy)`` or anything with ``.bounds`` (a GeoDataFrame, the table of
    :func:`mosaic_predictions`); ``affine_transformation`` = [a, b, d, e, xoff, yoff] of the raster, north-up.  ``pixel=True``: the
    table holds pixel-corner boxes ``(x0, y0, x1, y1)`` already and the transform is not used.  Returns
    ``BoxAssignment(assigned, area)``: ``assigned`` (n_labels + 1,) int32, the row of the winning box per segment id, ties to the
    lowest row (``idxmax``), -1 where the segment meets no box; ``area`` (n_labels + 1,) float64, the shared area in pixels.  Row 0 is
    unused and holds -1 / 0.  NumPy unless ``labels`` is a CUDA tensor; ``as_array=True`` leaves CUDA tensors whatever came in.

    shapely's ``intersects`` is true for a pair that only touches, so the notebook's ``touches`` branch never runs: a segment that
    boxes only touch goes to the first of them, with area 0, here as there."""
    _need_torch()
    if pixel:
        if hasattr(boxes, "bounds"):
            boxes = boxes.bounds
        px = boxes
    else:
        if _device.is_torch(boxes):
            raise ValueError("map bounds are converted on the host: pass a host table, or pixel boxes with pixel=True")
        px = map_to_pixel(_bounds_table(boxes), affine_transformation)
    n, dev, lab, b, nl = _overlap_args(labels, px, n_labels, ctx)
    H, W = lab.shape
    lib, c = _device.begin(dev, ctx)
    assigned = torch.empty(nl + 1, dtype=torch.int32, device=lab.device)
    area = torch.empty(nl + 1, dtype=torch.float64, device=lab.device)
    _lib.check(lib.obia_boxes_assign_dev(c.handle, lab.data_ptr(), H, W, b.data_ptr(), n, nl, assigned.data_ptr(), area.data_ptr()))
    return BoxAssignment(*_device.out((assigned, area), as_array or _device.is_torch(labels)))


def dissolve_by_box(labels, assigned, ctx=None):
    """The raster of the crowns: ``assigned[label] + 1`` per pixel, 0 where the label is outside 1 .. len(assigned) - 1 or has no
    box.  (H, W) int32.  Equal ids that touch are one region for ``polygonize``: the segments of one box become one crown."""
    _need_torch()
    _check_labels(labels, None)
    if len(_shape(assigned)) != 1 or _shape(assigned)[0] < 1 or _shape(assigned)[0] >= 2 ** 31:
        raise ValueError(f"assigned must be an (n_labels + 1,) table, got shape {_shape(assigned)}")
    dev = _device.device_of(ctx, labels, assigned)
    lab = _device.as_dev(labels, torch.int32, dev)
    a = _device.as_dev(assigned, torch.int32, dev)
    lib, c = _device.begin(dev, ctx)
    out = torch.empty_like(lab)
    _lib.check(lib.obia_boxes_dissolve_dev(c.handle, lab.data_ptr(), lab.numel(), a.data_ptr(), a.numel() - 1, out.data_ptr()))
    return _device.out(out, _device.is_torch(labels))


def box_iou(a, b, ctx=None):
    """``calculate_iou`` (obia/detection/utils.py:63-81) of every row of ``a`` (na, 4) with every row of ``b`` (nb, 4), boxes
    ``[x_min, y_min, x_max, y_max]``: (na, nb) float64, bit for bit what the reference returns for the pair as Python floats.
    float32 tables are widened first -- the reference, given float32 scalars, would compute in float32."""
    _need_torch()
    na, nb = _box_rows(a, "a"), _box_rows(b, "b")
    dev = _device.device_of(ctx, a, b)
    ta, tb = _device.as_dev(a, torch.float64, dev), _device.as_dev(b, torch.float64, dev)
    lib, c = _device.begin(dev, ctx)
    out = torch.empty((na, nb), dtype=torch.float64, device=ta.device)
    _lib.check(lib.obia_boxes_iou_dev(c.handle, ta.data_ptr(), na, tb.data_ptr(), nb, out.data_ptr()))
    return _device.out(out, _device.is_torch(a))


def box_nms(boxes, scores, iou_threshold, groups=None, ctx=None):
    """Greedy non-maximum suppression with the reference's IoU: ``(keep, kept)``, ``keep`` (n,) bool and ``kept`` (int64) the rows
    that stay, by descending score.

    The rows are taken by score descending, ties to the earlier row; a row stays unless an earlier row of that order stays, is of
    the same group (``groups``: any integer column; None: one group) and has ``iou > iou_threshold`` with it.  ``iou_threshold``
    must be >= 0; boxes finite with x0 <= x1, y0 <= y1; NaN scores are refused.  Memory is O(n): neighbours are found on the
    uniform grid of include/obia_seed_table.h."""
    from . import seeds
    _need_torch()
    n = _box_rows(boxes)
    if _shape(scores) != (n,) or (groups is not None and _shape(groups) != (n,)):
        raise ValueError("boxes, scores and groups must be of one length")
    thr = float(iou_threshold)
    if not thr >= 0.0:
        raise ValueError(f"iou_threshold must be >= 0, got {iou_threshold!r}")
    is_t = _device.is_torch(boxes)
    dev = _device.device_of(ctx, boxes, scores, groups)
    if not is_t:
        _check_boxes(boxes)
    if not _device.is_torch(scores) and bool(np.isnan(np.asarray(scores, dtype=np.float64)).any()):
        raise ValueError("scores contain NaN")
    b = _device.as_dev(boxes, torch.float64, dev)
    s = _device.as_dev(scores, torch.float64, dev)
    if is_t:
        _check_boxes(b)
    if _device.is_torch(scores) and bool(torch.isnan(s).any()):
        raise ValueError("scores contain NaN")
    lib, c = _device.begin(dev, ctx)
    by_score = torch.sort(s, descending=True, stable=True).indices
    pos = torch.empty(n, dtype=torch.int64, device=b.device)
    pos[by_score] = torch.arange(n, dtype=torch.int64, device=b.device)
    side = float(torch.maximum((b[:, 2] - b[:, 0]).max(), (b[:, 3] - b[:, 1]).max()))
    order, skey, ncx = seeds._grid(lib, c, dev, b[:, 0].contiguous(), b[:, 1].contiguous(), side)
    b_s, pos_s = b[order].contiguous(), pos[order].to(torch.int32).contiguous()
    g_s = None
    if groups is not None:
        g = torch.as_tensor(groups, device=b.device) if is_t or _device.is_torch(groups) else torch.as_tensor(np.asarray(groups), device=b.device)
        g_s = torch.unique(g, return_inverse=True)[1].to(torch.int32)[order].contiguous()
    keep_s = torch.empty(n, dtype=torch.uint8, device=b.device)
    torch.cuda.current_stream(dev).synchronize()
    _lib.check(lib.obia_boxes_nms_dev(c.handle, b_s.data_ptr(), pos_s.data_ptr(), None if g_s is None else g_s.data_ptr(), skey.data_ptr(), n,
                                      ncx, thr, keep_s.data_ptr(), None))
    keep = torch.empty(n, dtype=torch.bool, device=b.device)
    keep[order] = keep_s != 0
    return _device.out((keep, by_score[keep[by_score]]), is_t)


# ------------------------------------------------------------------------------------------------------------- host glue
def _columns(predictions):
    """xmin, ymin, xmax, ymax (n, 4) float64 and the optional label / score columns of a mapping of columns (a DataFrame is one)"""
    try:
        cols = [np.asarray(predictions[k], dtype=np.float64).reshape(-1) for k in ("xmin", "ymin", "xmax", "ymax")]
    except (KeyError, TypeError, IndexError):
        raise ValueError("predictions must be a mapping with the columns xmin, ymin, xmax, ymax") from None
    if len({len(v) for v in cols}) != 1:
        raise ValueError("the columns of predictions must be of one length")
    n = len(cols[0])
    keys = set(predictions.keys()) if hasattr(predictions, "keys") else set()
    label = [str(v) for v in predictions["label"]] if "label" in keys else ["Tree"] * n
    score = np.asarray(predictions["score"], dtype=np.float64).reshape(-1) if "score" in keys else None
    if len(label) != n or (score is not None and len(score) != n):
        raise ValueError("the columns of predictions must be of one length")
    return np.stack(cols, 1).reshape(n, 4), label, score


def _transforms(transforms):
    """the dict of ``tile_and_process``, read from ``transforms.json`` when a path is given"""
    if isinstance(transforms, (str, bytes)) or hasattr(transforms, "__fspath__"):
        with open(transforms, "r") as f:
            return json.load(f)
    return transforms


def predictions_to_map(boxes_px, transform):
    """The four corners of every pixel box ``(xmin, ymin, xmax, ymax)`` of a tile under its transform ``[a, b, c, d, e, f]``
    (rasterio's order, as ``transforms.json`` holds it), in the reference's order (utils.py:118-128: top-left, top-right,
    bottom-right, bottom-left) and closed: (n, 5, 2) float64, ``tile_affine * (col, row)`` = (col a + row b + c, col d + row e + f)."""
    a, b, c, d, e, f = [float(v) for v in transform]
    t = np.asarray(boxes_px, dtype=np.float64).reshape(-1, 4)
    col = t[:, [0, 2, 2, 0, 0]]
    row = t[:, [1, 1, 3, 3, 1]]
    return np.stack([col * a + row * b + c, col * d + row * e + f], 2)


def _ring_wkb(ring):
    return struct.pack("<BIII", 1, 3, 1, len(ring)) + np.ascontiguousarray(ring, dtype="<f8").tobytes()


def _epsg(crs):
    s = str(crs)
    return int(s[5:]) if s.upper().startswith("EPSG:") and s[5:].isdigit() else None


def save_predictions_to_gpkg(predictions, tile_name, transforms, output_gpkg):
    """``save_deepforest_predictions_to_gpkg`` (obia/utils/utils.py:70-145): the pixel boxes a detector returned for one tile as
    polygons in map coordinates, in a GeoPackage with the columns ``label`` (default "Tree") and ``score``.  ``predictions``: a
    mapping of columns ``xmin ymin xmax ymax`` and optionally ``label`` and ``score`` (a DataFrame is one); ``transforms``: the dict
    of ``tile_and_process`` or the path of its ``transforms.json``.  Like the reference it returns None without writing when the tile
    is not in ``transforms`` or there is no row; otherwise the path."""
    from .geopackage import write_geopackage
    info = _transforms(transforms).get(tile_name)
    if info is None:
        print(f"Tile '{tile_name}' not found in transforms.json. Skipping.")
        return None
    boxes, label, score = _columns(predictions)
    if not len(boxes):
        print(f"No predictions to save for tile {tile_name}")
        return None
    rings = predictions_to_map(boxes, info["transform"])
    score = np.full(len(boxes), np.nan) if score is None else score
    return write_geopackage(output_gpkg, [_ring_wkb(r) for r in rings], {"label": label, "score": score}, table="predictions",
                            srs_epsg=_epsg(info.get("crs")))


def mosaic_predictions(per_tile, transforms, iou_threshold=0.15, score_threshold=None, ctx=None):
    """The detections of all tiles as one table without the copies: ``per_tile`` maps a tile's name to its predictions (as
    :func:`save_predictions_to_gpkg` takes them, ``score`` required); every box is taken to map coordinates through its tile's
    transform, rows below ``score_threshold`` are dropped, and :func:`box_nms` runs across the tiles -- the tiles of
    ``tile_and_process`` overlap, so a tree arrives up to four times.  Returns ``BoxTable(bounds, score, label, tile)`` by
    descending score: ``bounds`` (m, 4) ``(minx, miny, maxx, maxy)``, which :func:`assign_boxes` accepts.  A tile that is not in
    ``transforms`` is an error here; a tile without rows adds nothing."""
    transforms = _transforms(transforms)
    bounds, scores, labels, tiles = [], [], [], []
    for name, pred in per_tile.items():
        info = transforms.get(name)
        if info is None:
            raise ValueError(f"tile {name!r} is not in transforms")
        boxes, label, score = _columns(pred)
        if not len(boxes):
            continue
        if score is None:
            raise ValueError(f"the predictions of tile {name!r} have no score column")
        rings = predictions_to_map(boxes, info["transform"])
        bounds.append(np.concatenate([rings.min(1), rings.max(1)], 1))
        scores.append(score)
        labels += label
        tiles += [name] * len(boxes)
    if not bounds:
        return BoxTable(np.zeros((0, 4)), np.zeros(0), [], [])
    bounds, scores = np.concatenate(bounds), np.concatenate(scores)
    rows = np.arange(len(scores)) if score_threshold is None else np.flatnonzero(scores >= float(score_threshold))
    if not len(rows):
        return BoxTable(np.zeros((0, 4)), np.zeros(0), [], [])
    _, kept = box_nms(bounds[rows], scores[rows], iou_threshold, ctx=ctx)
    rows = rows[kept]
    return BoxTable(bounds[rows], scores[rows], [labels[i] for i in rows], [tiles[i] for i in rows])
