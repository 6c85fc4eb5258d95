"""Label raster -> polygons: host-side mirror of the vectorisation half of ``create_segments``.

The reference (obia/segmentation/segment_boundaries.py:59-77) loops over ``np.unique(segments)``, builds a
full-raster mask per id, runs ``rasterio.features.shapes`` (GDAL polygonize, 4-connected) on it, applies
``image.affine_transformation`` ([a, b, d, e, xoff, yoff], shapely order) and numbers the polygons 1..N in that order.
Here the rings of ALL labels come from one GPU pass (libobia_hip.so: obia_polygon_rings_i32_dev); this module groups
them per label (exterior ring first, then holes), applies the affine transform and hands them over as plain arrays,
GeoJSON-like dicts, WKB, or -- when geopandas / shapely are installed on the user's side -- a GeoDataFrame with the
reference's ``segment_id`` column.
"""
import ctypes
import struct

import numpy as np

from . import _device, _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


class PolygonTable:
    """Rings of every label of a raster.

    ``xy``            (V, 2) float64 vertex coordinates (map coordinates when a transform was given, else pixel-corner
                      coordinates, (0,0) = top-left corner of the raster); vertices only where the outline turns;
                      every ring is closed (first vertex repeated)
    ``ring_offset``   (R + 1,) int64: ring r owns ``xy[ring_offset[r]:ring_offset[r+1]]``
    ``ring_label``    (R,) int32 label of the ring, ``ring_is_hole`` (R,) bool
    Rings are ordered by label, and within a label the exterior ring comes first, then its holes (each label of a
    connectivity-enforced label map is one 4-connected component, hence one exterior ring).
    ``labels``        (N,) the distinct labels in ascending order -- polygon i gets ``segment_id = i + 1`` like the
                      reference's ``range(1, len(gdf) + 1)``; ``poly_ring_start`` (N + 1,) indexes the rings of polygon i.
    """

    def __init__(self, xy, ring_offset, ring_label, ring_is_hole, ring_part=None):
        self.xy, self.ring_offset, self.ring_label, self.ring_is_hole = xy, ring_offset, ring_label, ring_is_hole
        self.labels, first = np.unique(ring_label, return_index=True)
        self.poly_ring_start = np.append(first, len(ring_label)).astype(np.int64)
        # ring_part[r]: index of the exterior ring whose polygon ring r belongs to (itself for exterior rings)
        self.ring_part = ring_part if ring_part is not None else first[np.searchsorted(self.labels, ring_label)]

    def __len__(self):
        return len(self.labels)

    def rings_of(self, i):
        """[(is_hole, (n, 2) coordinates), ...] of polygon i (exterior first)."""
        out = []
        for r in range(self.poly_ring_start[i], self.poly_ring_start[i + 1]):
            out.append((bool(self.ring_is_hole[r]), self.xy[self.ring_offset[r]:self.ring_offset[r + 1]]))
        return out

    def _parts(self, i):
        """Polygons of label i as lists of rings: one part per exterior ring (a label that is not connected has several)."""
        lo, hi = self.poly_ring_start[i], self.poly_ring_start[i + 1]
        parts = {}
        for r in range(lo, hi):
            ring = self.xy[self.ring_offset[r]:self.ring_offset[r + 1]]
            parts.setdefault(int(self.ring_part[r]), []).append((bool(self.ring_is_hole[r]), ring))
        return [[ring for hole, ring in sorted(v, key=lambda t: t[0])] for k, v in sorted(parts.items())]

    def geojson_features(self):
        """GeoJSON-like Feature dicts with ``segment_id`` = 1..N in label order (segment_boundaries.py:76)."""
        feats = []
        for i in range(len(self)):
            parts = self._parts(i)
            if len(parts) == 1:
                geom = {"type": "Polygon", "coordinates": [r.tolist() for r in parts[0]]}
            else:
                geom = {"type": "MultiPolygon", "coordinates": [[r.tolist() for r in part] for part in parts]}
            feats.append({"type": "Feature", "properties": {"segment_id": i + 1, "label": int(self.labels[i])},
                          "geometry": geom})
        return feats

    def wkb(self):
        """Little-endian WKB of every polygon (list of bytes), ready for ``shapely.from_wkb`` / a GeoPackage writer."""
        out = []
        for i in range(len(self)):
            parts = self._parts(i)

            def poly_bytes(rings):
                b = struct.pack("<BII", 1, 3, len(rings))
                for r in rings:
                    b += struct.pack("<I", len(r)) + np.ascontiguousarray(r, "<f8").tobytes()
                return b
            if len(parts) == 1:
                out.append(poly_bytes(parts[0]))
            else:
                out.append(struct.pack("<BII", 1, 6, len(parts)) + b"".join(poly_bytes(p) for p in parts))
        return out

    def to_geodataframe(self, crs=None):
        """GeoDataFrame(geometry, segment_id) as create_segments returns it; needs geopandas + shapely (not part of this
        package's requirements -- the reference's own stack provides them)."""
        import geopandas as gpd
        import shapely
        gdf = gpd.GeoDataFrame(geometry=list(shapely.from_wkb(self.wkb())), crs=crs)
        gdf["segment_id"] = range(1, len(gdf) + 1)
        return gdf

    def areas(self):
        """Signed shoelace area per ring in the units of ``xy`` (exterior and holes have opposite signs)."""
        x, y = self.xy[:, 0], self.xy[:, 1]
        cross = x[:-1] * y[1:] - x[1:] * y[:-1]
        cs = np.concatenate([[0.0], np.cumsum(cross)])
        lo, hi = self.ring_offset[:-1], self.ring_offset[1:] - 1      # the closing edge is part of the ring
        return 0.5 * (cs[hi] - cs[lo])


def _point_in_ring(p, ring):
    x, y = ring[:, 0], ring[:, 1]
    x0, y0, x1, y1 = x[:-1], y[:-1], x[1:], y[1:]
    cond = (y0 > p[1]) != (y1 > p[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        xi = x0 + (p[1] - y0) * (x1 - x0) / (y1 - y0)
    return bool(np.count_nonzero(cond & (p[0] < xi)) & 1)


def polygonize(labels, affine_transformation=None, start_label=0, ctx=None):
    """Polygons of a label raster (``create_segments`` back half, segment_boundaries.py:59-77).

    ``labels``: (H, W) integer raster, NumPy or CUDA tensor; pixels with a label below ``start_label`` (the reference
    writes -1 where the mask is 0 and skips that id) get no polygon.  ``affine_transformation``: the reference's
    ``image.affine_transformation`` = [a, b, d, e, xoff, yoff] (x' = a*x + b*y + xoff, y' = d*x + e*y + yoff applied to
    pixel-corner coordinates); None keeps pixel-corner coordinates.  Returns a :class:`PolygonTable`.
    """
    _device.need_torch("obia_amd.polygons")
    lab = _device.as_dev(labels, torch.int32, _device.device_of(ctx, labels))
    if lab.dim() != 2:
        raise ValueError("labels must be (H, W)")
    H, W = lab.shape
    dev = lab.device
    lib, c = _device.begin(dev.index, ctx)
    n_r, n_v = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.obia_polygon_count_i32_dev(c.handle, lab.data_ptr(), H, W, int(start_label), ctypes.byref(n_r),
                                              ctypes.byref(n_v)))
    R, V = int(n_r.value), int(n_v.value)
    ring_label = torch.empty((max(R, 1),), dtype=torch.int32, device=dev)
    ring_hole = torch.empty((max(R, 1),), dtype=torch.uint8, device=dev)
    ring_off = torch.zeros((R + 1,), dtype=torch.int64, device=dev)
    xy = torch.empty((max(V, 1), 2), dtype=torch.int32, device=dev)
    torch.cuda.current_stream(dev).synchronize()   # ring_off's zeros are in place before the context's stream writes the offsets over them
    _lib.check(lib.obia_polygon_rings_i32_dev(c.handle, lab.data_ptr(), H, W, int(start_label), R, V, ring_label.data_ptr(),
                                              ring_hole.data_ptr(), ring_off.data_ptr(), xy.data_ptr(), ctypes.byref(n_r),
                                              ctypes.byref(n_v)))
    xyf = xy[:V].to(torch.float64)
    if affine_transformation is not None:
        a, b, d, e, xoff, yoff = [float(v) for v in affine_transformation]
        xyf = torch.stack([a * xyf[:, 0] + b * xyf[:, 1] + xoff, d * xyf[:, 0] + e * xyf[:, 1] + yoff], dim=1)
    xy_h = xyf.cpu().numpy()
    rl = ring_label[:R].cpu().numpy()
    rh = ring_hole[:R].cpu().numpy().astype(bool)
    ro = ring_off.cpu().numpy()
    # group: by label, exterior before holes, otherwise raster order of the rings' smallest corners (stable sort)
    order = np.lexsort((rh, rl)) if R else np.zeros((0,), np.int64)
    lens = (ro[1:] - ro[:-1])[order]
    new_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([np.arange(ro[r], ro[r + 1]) for r in order]) if R and R < 64 else None
    if R:
        if idx is None:      # vectorised gather of the vertex ranges
            starts = ro[:-1][order]
            idx = np.repeat(starts - new_off[:-1], lens) + np.arange(new_off[-1])
        xy_h = xy_h[idx]
    rl, rh = rl[order], rh[order]
    ring_part = _assign_parts(xy[:V].cpu().numpy()[idx] if R else np.zeros((0, 2), np.int32), new_off, rl, rh)
    return PolygonTable(xy_h, new_off, rl, rh, ring_part)


def _assign_parts(xy_pix, off, ring_label, ring_hole):
    """Exterior ring of every ring, decided on pixel-corner coordinates.  A connectivity-enforced label map has one
    exterior ring per label (every hole belongs to it); a label with several 4-connected parts gets its holes assigned
    to the smallest exterior ring that contains them."""
    R = len(ring_label)
    part = np.arange(R, dtype=np.int64)
    if R == 0:
        return part
    labels, first, counts = np.unique(ring_label, return_index=True, return_counts=True)
    n_ext = np.add.reduceat((~ring_hole).astype(np.int64), first)
    single = np.repeat(n_ext == 1, counts)
    part[single] = np.repeat(first, counts)[single]          # the exterior ring is the first ring of its label
    for li in np.nonzero(n_ext > 1)[0]:
        lo, hi = first[li], first[li] + counts[li]
        exts = [r for r in range(lo, hi) if not ring_hole[r]]
        rings = {r: xy_pix[off[r]:off[r + 1]].astype(np.float64) for r in range(lo, hi)}
        area = {r: abs(_shoelace(rings[r])) for r in exts}
        for r in range(lo, hi):
            if not ring_hole[r]:
                continue
            a, b = rings[r][0], rings[r][1]
            d = b - a
            n = np.array([d[1], -d[0]]) / max(np.hypot(*d), 1e-30)
            p = 0.5 * (a + b) + 0.25 * n                     # just beside the middle of the first edge: off the pixel grid
            inside = [e for e in exts if _point_in_ring(p, rings[e])]
            part[r] = min(inside, key=lambda e: area[e]) if inside else exts[0]
    return part


def _shoelace(ring):
    x, y = ring[:, 0], ring[:, 1]
    return 0.5 * float(np.sum(x[:-1] * y[1:] - x[1:] * y[:-1]))


# ------------------------------------------------------------------------------------------------- polygons -> label raster
def to_pixel(xy, affine_transformation=None):
    """Map coordinates -> pixel coordinates (x = column axis, y = row axis, (0, 0) = top-left corner of the raster) on the
    host in NumPy float64: ``col = ra*x + rb*y + rc``, ``row = rd*x + re*y + rf`` with the six numbers of
    :func:`obia_amd.seeds.invert_affine`.  ``None`` means the coordinates are pixel coordinates already.  This is the one
    place the transform is applied, so the rasteriser and anything that checks it start from the same bits."""
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    if affine_transformation is None:
        return xy
    from .seeds import invert_affine
    if len(affine_transformation) != 6:
        raise ValueError("affine_transformation must hold six values [a, b, d, e, xoff, yoff]")
    ra, rb, rc, rd, re, rf = invert_affine(affine_transformation)
    x, y = xy[:, 0], xy[:, 1]
    return np.stack([ra * x + rb * y + rc, rd * x + re * y + rf], axis=1)


def _rings_of_wkb(wkbs):
    """(xy (V, 2) float64, ring_offset, ring_shape) of a sequence of little-endian WKB Polygon / MultiPolygon blobs: one shape
    per blob, its rings (exterior rings and holes of all parts) in file order."""
    from .geopackage import wkb_rings
    chunks, lens, shape = [], [], []
    for i, w in enumerate(wkbs):
        if not isinstance(w, (bytes, bytearray, memoryview)):
            raise ValueError(f"shape {i} is not WKB bytes")
        w = bytes(w)
        if len(w) < 9 or w[0] != 1 or struct.unpack_from("<I", w, 1)[0] not in (3, 6):
            raise ValueError(f"shape {i} is not a little-endian WKB Polygon or MultiPolygon")
        try:
            parts = wkb_rings(w)
        except (struct.error, ValueError) as e:
            raise ValueError(f"shape {i}: truncated WKB") from e
        for part in parts:
            for ring in part:
                chunks.append(ring)
                lens.append(len(ring))
                shape.append(i)
    xy = np.concatenate(chunks) if chunks else np.zeros((0, 2), np.float64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return xy, off, np.asarray(shape, np.int32)


def _host(x):
    return x.cpu().numpy() if _device.is_torch(x) else np.asarray(x)


def rasterize(shapes, out_shape, affine_transformation=None, values=None, fill=0, ctx=None, as_tensor=False):
    """Burn polygons into an (H, W) int32 raster: ``rasterio.features.rasterize(shapes, out_shape, fill=fill,
    all_touched=False)`` (rasterise_slic_gpkg, obia/utils/cost.py:78-85) on the GPU -- the way back from :func:`polygonize`.

    ``shapes``: a :class:`PolygonTable` (one shape per polygon, in table order), a sequence of little-endian WKB ``Polygon`` /
    ``MultiPolygon`` bytes (one shape per blob), or the ring arrays themselves as a tuple ``(xy (V, 2), ring_offset (R + 1,),
    ring_shape (R,))`` of NumPy arrays or CUDA tensors, ``ring_shape`` non-decreasing.  ``values``: the burn value of every shape
    (int32); default ``table.labels`` for a table and 1..N otherwise.  ``affine_transformation``: [a, b, d, e, xoff, yoff] of
    the coordinates as elsewhere (inverted and applied on the host in float64, :func:`to_pixel`); None: the coordinates are
    pixel-corner coordinates.

    The rule: pixel (r, c) has its centre at (c + 0.5, r + 0.5); an edge (x0, y0) -> (x1, y1) of a shape
    counts when ``(y0 <= yc) != (y1 <= yc)`` and ``x0 + (yc - y0) * (x1 - x0) / (y1 - y0) <= xc``; the shape covers the pixel
    iff an odd number of its edges count (even-odd over all its rings, the ring roles are not used).  A pixel gets the value of
    the last shape in input order that covers it, ``fill`` when none does.  Rings may lie partly or wholly outside the raster.
    Returns an (H, W) int32 NumPy array, or a CUDA tensor with ``as_tensor=True``.  There is no CPU path.
    """
    try:
        H, W = (int(v) for v in out_shape)
    except Exception:
        raise ValueError(f"out_shape must be (H, W), got {out_shape!r}") from None
    if H <= 0 or W <= 0 or tuple(out_shape) != (H, W):
        raise ValueError(f"out_shape must be two positive integers, got {out_shape!r}")
    if H * W >= 2 ** 31:
        raise NotImplementedError(f"rasters of 2^31 pixels or more are not supported (got {H} x {W})")
    on_device = False
    if isinstance(shapes, PolygonTable):
        xy, off, n_shapes = shapes.xy, shapes.ring_offset, len(shapes)
        rshape = np.searchsorted(shapes.labels, shapes.ring_label).astype(np.int32)
        default_values = shapes.labels
    elif isinstance(shapes, tuple) and len(shapes) == 3 and not isinstance(shapes[0], (bytes, bytearray, memoryview)):
        xy, off, rshape = shapes
        on_device = any(_device.is_torch(t) for t in shapes)
        if on_device and not all(_device.is_torch(t) and t.is_cuda for t in shapes):
            raise ValueError("ring arrays must be all NumPy arrays or all CUDA tensors")
        if not on_device:
            xy, off, rshape = np.asarray(xy), np.asarray(off), np.asarray(rshape)
        if len(xy.shape) != 2 or xy.shape[1] != 2:
            raise ValueError(f"xy must be (V, 2), got shape {tuple(xy.shape)}")
        if len(off.shape) != 1 or len(rshape.shape) != 1 or off.shape[0] != rshape.shape[0] + 1:
            raise ValueError("ring_offset must hold one more entry than ring_shape")
        n_shapes = (int(rshape.max()) + 1) if rshape.shape[0] else 0
        if values is not None:
            n_shapes = len(values)
        default_values = None
    else:
        if isinstance(shapes, (bytes, bytearray, str)) or not hasattr(shapes, "__len__"):
            raise ValueError("shapes must be a PolygonTable, a sequence of WKB bytes or (xy, ring_offset, ring_shape)")
        xy, off, rshape = _rings_of_wkb(shapes)
        n_shapes = len(shapes)
        default_values = None
    if values is None:
        values = default_values if default_values is not None else np.arange(1, n_shapes + 1)
    values = _host(values)
    if values.ndim != 1 or len(values) != n_shapes:
        raise ValueError(f"values holds {values.size} entries for {n_shapes} shapes")
    if values.size and (values.dtype.kind not in "iub" or values.min() < -2 ** 31 or values.max() >= 2 ** 31):
        raise ValueError("values must be integers that fit int32")
    if not -2 ** 31 <= int(fill) < 2 ** 31:
        raise ValueError("fill must fit int32")
    # the ring tables are small: check them on the host whichever side they live on
    off_h, rshape_h = _host(off).astype(np.int64), _host(rshape).astype(np.int64)
    if off_h[0] != 0 or off_h[-1] != xy.shape[0] or (np.diff(off_h) < 0).any():
        raise ValueError("ring_offset must start at 0, never decrease and end at the number of vertices")
    if rshape_h.size and ((np.diff(rshape_h) < 0).any() or rshape_h[0] < 0 or rshape_h[-1] >= n_shapes):
        raise ValueError("ring_shape must not decrease and must lie in [0, number of shapes)")
    if max(xy.shape[0], n_shapes, rshape_h.size) >= 2 ** 31:
        raise NotImplementedError("2^31 or more vertices, rings or shapes are not supported")
    if not on_device and not np.isfinite(np.asarray(xy, dtype=np.float64)).all():
        raise ValueError("vertex coordinates must be finite")
    if affine_transformation is not None or not on_device:
        xy = to_pixel(_host(xy), affine_transformation)       # (raises ValueError for a singular or malformed transform)

    _device.need_torch("obia_amd.polygons")
    _lib.load()                                               # (a library that is not built is reported before anything is uploaded)
    dev = _device.device_of(ctx, *(shapes if on_device else ()))
    d = f"cuda:{dev}"
    xy_d = torch.as_tensor(xy, device=d).to(torch.float64).contiguous()
    if on_device and not bool(torch.isfinite(xy_d).all()):
        raise ValueError("vertex coordinates must be finite")
    off_d = torch.as_tensor(off_h, device=d)
    rs_d = torch.as_tensor(rshape_h.astype(np.int32), device=d)
    val_d = torch.as_tensor(np.ascontiguousarray(values, dtype=np.int32), device=d)
    out = torch.empty((H, W), dtype=torch.int32, device=d)
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_rasterize_polygons_dev(c.handle, xy_d.data_ptr() if xy_d.numel() else None, off_d.data_ptr(),
                                               int(rs_d.numel()), rs_d.data_ptr() if rs_d.numel() else None,
                                               val_d.data_ptr() if val_d.numel() else None, n_shapes, H, W, int(fill),
                                               out.data_ptr()))
    return out if as_tensor else out.cpu().numpy()


def rasterize_info():
    """Developer aid: {"small", "large"} = shapes the last :func:`rasterize` of this process handled one wave each / through the
    banded large-shape path, and the limits of the one-wave path ("max_edges", "max_side" in pixel centres)."""
    info = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().obia_rasterize_info(info))
    return {"small": int(info[0]), "large": int(info[1]), "max_edges": int(info[2]), "max_side": int(info[3])}
