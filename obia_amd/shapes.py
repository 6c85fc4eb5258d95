"""How large, how elongated, how compact and which way round every segment is: the geometric columns of an object-based feature
table (include/obia_shapes.h).  The reference has no counterpart: its objects table holds spectral, textural and
structural columns only.

``segment_shapes`` is one pass over the label raster -- per segment the area, the raw first and second moments of the pixel indices,
the perimeter in pixel edges and the bounding box, all integers -- and returns a :class:`ShapeTable`.  Every derived column is a table
of N rows computed with torch from those integers, in float64 and in a stated order: centroid, central second moments, eigenvalues,
axis lengths, eccentricity and orientation as scikit-image's ``regionprops`` defines them, extent, and the compactness and smoothness
terms of Baatz and Schaepe.  ``ShapeTable.merge`` gives the table of the objects a ``root`` column forms without another pass over
the raster, ``pair_shapes`` the shape of the union of the two ends of every edge of a :class:`~obia_amd.adjacency.SegmentGraph` -- a
shape criterion for a link rule -- and ``shape_columns`` the DataFrame that goes beside ``create_objects``.

NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out.  There is no CPU path."""
import math

import numpy as np

from . import _device, _lib
from .adjacency import _check_labels, _count_labels, _ptr
from .cost import _shape

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

FOUR_PI = 4.0 * math.pi
QUARTER_PI = math.pi / 4.0
SHAPE_COLUMNS = ("area", "perimeter", "bbox_height", "bbox_width", "centroid_row", "centroid_col", "mu_rr", "mu_cc", "mu_rc",
                 "major_axis_length", "minor_axis_length", "eccentricity", "orientation", "extent", "compactness", "shape_index", "smoothness")


def _need_torch():
    _device.need_torch("obia_amd.shapes")


def _check_sums_fit(H, W):
    """include/obia_shapes.h, NO SUM OVERFLOWS: every sum of every labelling is below max(H, W)^2 H W"""
    if max(H, W) ** 2 * H * W >= 2 ** 63:
        raise NotImplementedError(f"max(H, W)^2 * H * W must be below 2^63 (no sum can overflow then), got {H} x {W}")


def _nan_where(x, keep):
    return torch.where(keep if x.dim() == 1 else keep[:, None], x, torch.full_like(x, float("nan")))


def _shape_terms(area, perimeter, height, width, keep):
    """extent, compactness, shape_index, smoothness (float64) of int64 columns; the quiet NaN where ``keep`` is not set"""
    fn, fp = area.to(torch.float64), perimeter.to(torch.float64)
    extent = fn / (height * width).to(torch.float64)
    compactness = (FOUR_PI * fn) / (fp * fp)
    shape_index = fp / (4.0 * torch.sqrt(fn))
    smoothness = fp / (2.0 * (height + width).to(torch.float64))
    return {"extent": _nan_where(extent, keep), "compactness": _nan_where(compactness, keep), "shape_index": _nan_where(shape_index, keep),
            "smoothness": _nan_where(smoothness, keep)}


class ShapeTable:
    """The integer tables of include/obia_shapes.h over the segments 0 .. ``n_labels`` - 1 (segment i carries the label
    ``start_label`` + i) and the columns derived from them.  ``sums`` (N, 7) int64: area, sum r, sum c, sum r^2, sum c^2, sum r c,
    perimeter; ``box`` (N, 4) int32: (r0, c0, r1, c1), half-open; a row without pixels is all zeros, and the quiet NaN in every
    float column."""

    def __init__(self, sums, box, n_labels, start_label=1, as_tensor=None):
        _need_torch()
        self._is_t = (_device.is_torch(sums) or _device.is_torch(box)) if as_tensor is None else bool(as_tensor)
        self._dev = _device.device_of(None, sums, box)
        self.n_labels, self.start_label = int(n_labels), int(start_label)
        self._sums = _device.as_dev(sums, torch.int64, self._dev)
        self._box = _device.as_dev(box, torch.int32, self._dev)
        if tuple(self._sums.shape) != (self.n_labels, _lib.SHAPE_SUMS) or tuple(self._box.shape) != (self.n_labels, 4):
            raise ValueError(f"sums must be (n_labels, {_lib.SHAPE_SUMS}) and box (n_labels, 4) with n_labels = {self.n_labels}, got shapes "
                             f"{tuple(self._sums.shape)} and {tuple(self._box.shape)}")

    def _out(self, t):
        return _device.out(t, self._is_t)

    # ---- the raw tables
    sums = property(lambda self: self._out(self._sums))
    box = property(lambda self: self._out(self._box))

    def _present(self):
        return self._sums[:, 0] > 0

    def _sides(self):
        b = self._box.to(torch.int64)
        return b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]

    present = property(lambda self: self._out(self._present()), doc="(N) bool: the segments that have pixels")
    area = property(lambda self: self._out(self._sums[:, 0].clone()), doc="(N) int64: pixels")
    perimeter = property(lambda self: self._out(self._sums[:, 6].clone()), doc="(N) int64: pixel edges around the segment")
    bbox_height = property(lambda self: self._out(self._sides()[0]), doc="(N) int64")
    bbox_width = property(lambda self: self._out(self._sides()[1]), doc="(N) int64")

    # ---- the moments
    def _centroid(self):
        fn = self._sums[:, 0].to(torch.float64)
        c = torch.stack([self._sums[:, 1].to(torch.float64) / fn, self._sums[:, 2].to(torch.float64) / fn], 1)
        return _nan_where(c, self._present())

    def _mu_raw(self):
        """(mu_rr, mu_cc, mu_rc) before the NaN of the empty rows.  The sums are first moved to the box origin in exact (wrapping)
        int64, so the columns depend on a segment's extent and not on where it lies; then (n S2 - S1 S1) / (n n) in float64."""
        s = self._sums
        n, sr, sc, srr, scc, src = (s[:, k] for k in range(6))
        r0, c0 = self._box[:, 0].to(torch.int64), self._box[:, 1].to(torch.int64)
        s_r, s_c = sr - n * r0, sc - n * c0
        s_rr = srr - 2 * r0 * sr + n * r0 * r0
        s_cc = scc - 2 * c0 * sc + n * c0 * c0
        s_rc = src - c0 * sr - r0 * sc + n * r0 * c0
        fn, f_r, f_c = n.to(torch.float64), s_r.to(torch.float64), s_c.to(torch.float64)
        nn = fn * fn
        return ((fn * s_rr.to(torch.float64) - f_r * f_r) / nn, (fn * s_cc.to(torch.float64) - f_c * f_c) / nn,
                (fn * s_rc.to(torch.float64) - f_r * f_c) / nn)

    def _eig_raw(self):
        mu_rr, mu_cc, mu_rc = self._mu_raw()
        t, d = mu_rr + mu_cc, mu_rr - mu_cc
        q = torch.sqrt(d * d + 4.0 * (mu_rc * mu_rc))
        return (t + q) / 2.0, torch.maximum((t - q) / 2.0, torch.zeros_like(t))

    def _orientation(self):
        """scikit-image 0.18.3: with a, b, c = mu_cc, -mu_rc, mu_rr of the inertia tensor, -pi/4 (b < 0) or pi/4 when a == c,
        atan2(-2 b, c - a) / 2 otherwise"""
        mu_rr, mu_cc, mu_rc = self._mu_raw()
        d = mu_rr - mu_cc
        angle = 0.5 * torch.atan2(2.0 * mu_rc, d)
        quarter = torch.where(mu_rc > 0, torch.full_like(d, -QUARTER_PI), torch.full_like(d, QUARTER_PI))
        return _nan_where(torch.where(d == 0, quarter, angle), self._present())

    def _eccentricity(self):
        l1, l2 = self._eig_raw()
        return _nan_where(torch.where(l1 == 0, torch.zeros_like(l1), torch.sqrt(1.0 - l2 / l1)), self._present())

    def _terms(self):
        return _shape_terms(self._sums[:, 0], self._sums[:, 6], *self._sides(), self._present())

    centroid = property(lambda self: self._out(self._centroid()), doc="(N, 2) float64: (sum r / n, sum c / n), in pixel indices")
    mu = property(lambda self: self._out(_nan_where(torch.stack(self._mu_raw(), 1), self._present())),
                  doc="(N, 3) float64: (mu_rr, mu_cc, mu_rc), the central second moments divided by n")
    eigenvalues = property(lambda self: self._out(_nan_where(torch.stack(self._eig_raw(), 1), self._present())),
                           doc="(N, 2) float64: l1 >= l2 >= 0 of [[mu_rr, mu_rc], [mu_rc, mu_cc]]")
    major_axis_length = property(lambda self: self._out(_nan_where(4.0 * torch.sqrt(self._eig_raw()[0]), self._present())))
    minor_axis_length = property(lambda self: self._out(_nan_where(4.0 * torch.sqrt(self._eig_raw()[1]), self._present())))
    eccentricity = property(lambda self: self._out(self._eccentricity()), doc="(N) float64: sqrt(1 - l2 / l1), 0 where l1 == 0")
    orientation = property(lambda self: self._out(self._orientation()), doc="(N) float64: as regionprops of scikit-image 0.18.3")
    extent = property(lambda self: self._out(self._terms()["extent"]), doc="(N) float64: area / (bbox_height bbox_width)")
    compactness = property(lambda self: self._out(self._terms()["compactness"]), doc="(N) float64: 4 pi area / perimeter^2; a square: pi / 4")
    shape_index = property(lambda self: self._out(self._terms()["shape_index"]), doc="(N) float64: perimeter / (4 sqrt(area)); a square: 1")
    smoothness = property(lambda self: self._out(self._terms()["smoothness"]), doc="(N) float64: perimeter / (2 (bbox_height + bbox_width))")

    def _centroid_xy(self, affine):
        a, b, d, e, xoff, yoff = [float(v) for v in affine]
        c = self._centroid()
        rr, cc = c[:, 0] + 0.5, c[:, 1] + 0.5
        xy = torch.stack([(a * cc + b * rr) + xoff, (d * cc + e * rr) + yoff], 1)
        return torch.where(xy != xy, torch.full_like(xy, float("nan")), xy)

    def centroid_xy(self, affine):
        """(N, 2) float64: the centroid in map units, at pixel centres: ``x = a (c + 0.5) + b (r + 0.5) + xoff`` and y likewise,
        with ``affine`` = [a, b, d, e, xoff, yoff] as everywhere in this package"""
        if len(affine) != 6:
            raise ValueError(f"affine must be [a, b, d, e, xoff, yoff], got {affine!r}")
        return self._out(self._centroid_xy(affine))

    # ---- objects made of segments
    def merge(self, root, graph):
        """The table of the objects ``root`` (N) forms -- ``root[i]`` is the row the segment i goes to, as
        :meth:`SegmentGraph.components` gives it -- without another pass over the raster: areas and sums add, boxes unite, and the
        perimeter is the members' less every border between two of them (``graph``: the :class:`SegmentGraph` of the same labels).
        The result is stored at row ``root[i]``; every other row is empty."""
        N = self.n_labels
        r = _device.as_dev(root, torch.int64, self._dev)
        if tuple(r.shape) != (N,):
            raise ValueError(f"root must be an (n_labels,) column with n_labels = {N}, got shape {tuple(r.shape)}")
        if graph.n_labels != N:
            raise ValueError(f"the graph has {graph.n_labels} segments, the table {N}")
        if N and (int(r.min()) < 0 or int(r.max()) >= N):
            raise ValueError("root must hold rows 0 .. n_labels - 1")
        sums = torch.zeros_like(self._sums).index_add_(0, r, self._sums)
        if graph.nnz and N:
            nb = graph._neighbor.to(torch.int64)
            real = graph._real()
            inner = real & (r[graph._rows()] == r[nb.clamp(max=N - 1)])
            sums[:, 6] -= torch.zeros(N, dtype=torch.int64, device=r.device).index_add_(0, r[graph._rows()], graph._border * inner)
        box = self._box.to(torch.int64)
        has = self._present()
        big = torch.iinfo(torch.int32).max
        lo = torch.where(has[:, None], box[:, :2], torch.full_like(box[:, :2], big))
        hi = torch.where(has[:, None], box[:, 2:], torch.zeros_like(box[:, 2:]))
        idx = r[:, None].expand(N, 2)
        lo = torch.full((N, 2), big, dtype=torch.int64, device=r.device).scatter_reduce_(0, idx, lo, "amin", include_self=True)
        hi = torch.zeros((N, 2), dtype=torch.int64, device=r.device).scatter_reduce_(0, idx, hi, "amax", include_self=True)
        lo = torch.where(sums[:, :1] > 0, lo, torch.zeros_like(lo))
        return ShapeTable(sums, torch.cat([lo, hi], 1).to(torch.int32), N, self.start_label, as_tensor=self._is_t)


def segment_shapes(labels, start_label=1, n_labels=None, ctx=None):
    """The :class:`ShapeTable` of a label raster (H, W): label l is segment l - ``start_label`` when that lies in 0 .. ``n_labels``
    - 1 (default: up to the largest label), every other value is background.  4-connectivity."""
    _need_torch()
    _check_labels(labels, start_label, n_labels)
    _check_sums_fit(*_shape(labels))
    dev = _device.device_of(ctx, labels)
    lab = _device.as_dev(labels, torch.int32, dev)
    N = _count_labels(lab, start_label, n_labels)
    H, W = lab.shape
    sums = torch.empty((N, _lib.SHAPE_SUMS), dtype=torch.int64, device=lab.device)
    box = torch.empty((N, 4), dtype=torch.int32, device=lab.device)
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_shape_sums_dev(c.handle, lab.data_ptr(), H, W, int(start_label), N, _ptr(sums), _ptr(box)))
    return ShapeTable(sums, box, N, start_label, as_tensor=_device.is_torch(labels))


def pair_shapes(graph, shapes):
    """For every entry i -> j of the graph's CSR, the shape of the union of its two ends: a dict of ``area``, ``perimeter`` (int64:
    the two perimeters less twice the shared border), ``box`` (nnz, 4) int32, and ``compactness``, ``shape_index`` and ``smoothness``
    (float64) of that union.  A pseudo entry (background, frame) gets 0 and NaN.  A link rule with a shape criterion is
    ``graph.components((d2 <= t * t) & (pairs["compactness"] >= c))``."""
    _need_torch()
    N = shapes.n_labels
    if graph.n_labels != N:
        raise ValueError(f"the graph has {graph.n_labels} segments, the table {N}")
    dev = graph._neighbor.device
    s, b = shapes._sums.to(dev), shapes._box.to(dev).to(torch.int64)
    real = graph._real()
    i = graph._rows()
    j = torch.where(real, graph._neighbor.to(torch.int64), torch.zeros_like(i))
    zero = torch.zeros_like(i)
    if N == 0 or graph.nnz == 0:
        area = perimeter = zero
        box = torch.zeros((graph.nnz, 4), dtype=torch.int64, device=dev)
    else:
        area = torch.where(real, s[i, 0] + s[j, 0], zero)
        perimeter = torch.where(real, s[i, 6] + s[j, 6] - 2 * graph._border, zero)
        box = torch.cat([torch.minimum(b[i, :2], b[j, :2]), torch.maximum(b[i, 2:], b[j, 2:])], 1) * real[:, None]
    terms = _shape_terms(area, perimeter, box[:, 2] - box[:, 0], box[:, 3] - box[:, 1], real)
    out = {"area": area, "perimeter": perimeter, "box": box.to(torch.int32), "compactness": terms["compactness"],
           "shape_index": terms["shape_index"], "smoothness": terms["smoothness"]}
    return _device.out(out, graph._is_t)


def shape_columns(objects, shapes, affine=None):
    """The geometric part of an objects table: a DataFrame aligned with the rows of ``create_objects`` -- the segments that have
    pixels, in ascending label order -- with the columns ``SHAPE_COLUMNS`` and, with ``affine`` = [a, b, d, e, xoff, yoff],
    ``centroid_x`` and ``centroid_y`` in map units."""
    import pandas as pd
    t = shapes
    host = lambda x: np.asarray(_device.out(x, False))               # noqa: E731
    present = host(t._present())
    if int(present.sum()) != len(objects):
        raise ValueError(f"the table has {len(objects)} rows, the shapes {int(present.sum())} segments with pixels")
    centroid, mu, terms = host(t._centroid()), host(torch.stack(t._mu_raw(), 1)), t._terms()
    l1, l2 = t._eig_raw()
    h, w = t._sides()
    data = {"area": host(t._sums[:, 0]), "perimeter": host(t._sums[:, 6]), "bbox_height": host(h), "bbox_width": host(w),
            "centroid_row": centroid[:, 0], "centroid_col": centroid[:, 1], "mu_rr": mu[:, 0], "mu_cc": mu[:, 1], "mu_rc": mu[:, 2],
            "major_axis_length": host(4.0 * torch.sqrt(l1)), "minor_axis_length": host(4.0 * torch.sqrt(l2)),
            "eccentricity": host(t._eccentricity()), "orientation": host(t._orientation())}
    data.update({k: host(terms[k]) for k in ("extent", "compactness", "shape_index", "smoothness")})
    if affine is not None:
        xy = host(t._centroid_xy(affine))
        data["centroid_x"], data["centroid_y"] = xy[:, 0], xy[:, 1]
    return pd.DataFrame({k: v[present] for k, v in data.items()}, index=objects.index)
