"""Point clouds on the GPU (include/obia_points.h): the LiDAR leg of both chains.

``points_to_rasters`` / :class:`PointRasters` turn points into the canopy height model and the point-density raster that
``make_chm_seeds``, ``make_density_seeds`` and ``make_cost_surface`` start from; ``segment_point_stats`` / :class:`SegmentPoints` join
points to the segments of a label raster and form the five point-cloud columns of the objects table (``pai``, ``fhd``, ``ch``,
``mean_intensity``, ``variance_intensity``), which ``create_objects(..., pointcloud=...)`` fills with them.

The radiometric pair is the reference's (segment_statistics.py:332-389: ``np.mean`` / ``np.var`` of ``Intensity``).  Its structural
code is gone (:326-329 raises), so the structural columns are this project's definitions: one vertical profile per segment -- the
segment footprint is the voxel column -- in bins of ``dz``.  These functions take heights above ground as given; reading EPT / LAZ,
float intensities and return-number weighting are out of scope.

Heights above ground come from raw ``Z`` through :class:`GroundIndex` / ``height_above_ground`` (the ``count`` nearest
ground-classified points, inverse-distance weighted) or ``height_above_dtm`` (a terrain raster), and ``normalize_heights`` hands the
result on as a cloud (include/obia_ground.h).  The definitions are modelled on PDAL's ``filters.hag_nn`` and
``filters.hag_dtm`` -- what pyforestscan's ``read_lidar(..., hag=True)`` runs -- and are NOT compared with PDAL anywhere.

A cloud without a ground class gets one from ``classify_ground`` / ``ground_filter`` / :class:`GroundFilter`, a progressive
morphological filter (the minimum elevation of every cell, grey openings with growing windows -- ``grey_erosion``, ``grey_dilation``,
``grey_opening`` -- one threshold raster, one test per point; include/obia_groundfilter.h), so
``normalize_heights(classify_ground(raw))`` is the chain from raw ``X, Y, Z``.  The definitions are modelled on Zhang et al. 2003 and
PDAL's ``filters.pmf`` and are NOT compared with PDAL anywhere.

The accumulators keep their state on the device and take a cloud in any number of ``add`` calls: every sum is an integer, so the
result is the same bits for every order and every cut.  NumPy in -> NumPy out, CUDA tensors in -> CUDA tensors out; there is no
CPU path."""
import collections
import ctypes
import math

import numpy as np

from . import _device, _lib
from .consumers import invert_affine
from .statistics import _n_labels

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

Points = collections.namedtuple("Points", "x y z intensity is_torch")
COLUMNS = ("n_points", "ch", "pai", "fhd", "mean_intensity", "variance_intensity")
COUNTERS = ("outside", "unlabelled", "out_of_range", "in_profile")
U32_MAX = 2 ** 32 - 1


def _need_torch():
    _device.need_torch("obia_amd.pointcloud")


def _field(pc, name):
    if isinstance(pc, dict):
        return pc.get(name)
    names = getattr(getattr(pc, "dtype", None), "names", None)
    if names is None:
        raise TypeError("a point cloud is a structured NumPy array or a dict of arrays with X, Y, HeightAboveGround (or Z) and "
                        "optionally Intensity")
    return pc[name] if name in names else None


def as_points(pointcloud):
    """The arrays of a point cloud: ``Points(x, y, z, intensity, is_torch)``.

    Accepts the reference's two forms (segment_statistics.py:361-369) -- a structured NumPy array, or a dict -- with the fields
    ``X``, ``Y``, ``HeightAboveGround`` (``Z`` when that is absent) and optionally ``Intensity``; a dict of CUDA tensors; and a
    pyforestscan-style list whose first element is such an array.  ``Intensity`` must be uint8 or uint16 (``TypeError`` otherwise:
    float intensities are out of scope).  Touches no device."""
    if isinstance(pointcloud, Points):
        return pointcloud
    if isinstance(pointcloud, (list, tuple)):
        if not pointcloud:
            raise ValueError("the point cloud list is empty")
        pointcloud = pointcloud[0]
    x, y = _field(pointcloud, "X"), _field(pointcloud, "Y")
    z = _field(pointcloud, "HeightAboveGround")
    if z is None:
        z = _field(pointcloud, "Z")
    if x is None or y is None or z is None:
        raise ValueError("a point cloud needs the fields X, Y and HeightAboveGround (or Z)")
    inten = _field(pointcloud, "Intensity")
    is_t = any(_device.is_torch(v) for v in (x, y, z, inten))
    if is_t and not all(_device.is_torch(v) for v in (x, y, z, inten) if v is not None):
        raise ValueError("the fields of a point cloud must be all tensors or all arrays")
    if not is_t:
        x, y, z = np.asarray(x), np.asarray(y), np.asarray(z)
        inten = None if inten is None else np.asarray(inten)
    n = tuple(x.shape)
    if len(n) != 1 or any(tuple(v.shape) != n for v in (y, z, inten) if v is not None):
        raise ValueError("the fields of a point cloud must be one-dimensional and of one length")
    if inten is not None:
        ok = (torch.uint8, torch.uint16) if is_t else (np.dtype(np.uint8), np.dtype(np.uint16))
        if inten.dtype not in ok:
            raise TypeError(f"Intensity must be uint8 or uint16, got {inten.dtype} (float intensities are out of scope)")
    return Points(x, y, z, inten, is_t)


def _device_points(p, dev):
    """x, y float64, z float32 and the intensity as the bits of uint16 (an int16 tensor) on the device"""
    x, y = _device.as_dev(p.x, torch.float64, dev), _device.as_dev(p.y, torch.float64, dev)
    z = _device.as_dev(p.z, torch.float32, dev)
    inten = None
    if p.intensity is not None:
        if p.is_torch:
            t = p.intensity.to(device=f"cuda:{dev}").contiguous()
            inten = t.view(torch.int16) if t.dtype == torch.uint16 else t.to(torch.int16)
        else:
            inten = torch.as_tensor(np.ascontiguousarray(p.intensity.astype(np.uint16, copy=False)).view(np.int16), device=f"cuda:{dev}")
    return x, y, z, inten


def _forward(affine_transformation):
    if affine_transformation is None or len(affine_transformation) != 6:
        raise ValueError("affine_transformation must hold six values [a, b, d, e, xoff, yoff]")
    t = [float(v) for v in affine_transformation]
    inv = invert_affine(t)                                      # ValueError when singular
    return t, (ctypes.c_double * 6)(*inv)


def _raster_shape(shape):
    s = tuple(int(v) for v in shape)
    if len(s) != 2 or s[0] < 1 or s[1] < 1 or s[0] >= 2 ** 31 or s[1] >= 2 ** 31:
        raise ValueError(f"shape must be (H, W) with 1 <= H, W < 2^31, got {tuple(shape)}")
    return s


class _Accumulator:
    """the host-side running total that keeps every uint32 count of the state from wrapping"""
    total = 0

    def _admit(self, n):
        if n >= 2 ** 31:
            raise NotImplementedError("one add takes fewer than 2^31 points: cut the cloud")
        if self.total + n > U32_MAX:
            raise OverflowError(f"{self.total} + {n} points could carry a uint32 count past 2^32 - 1")

    def _device_cloud(self, points):
        p = as_points(points)
        if p.is_torch:
            _device.device_of(None, p.x, p.y, p.z, p.intensity)          # refuses CPU tensors
        self._admit(int(p.x.shape[0]))
        self._tensor_in = self._tensor_in or p.is_torch
        return p, int(p.x.shape[0])


class PointRasters(_Accumulator):
    """Canopy height model and point density of a cloud on the grid of a raster: ``add`` points in any number of calls, then
    ``result``.  ``shape`` = (H, W), ``affine_transformation`` = [a, b, d, e, xoff, yoff] of the raster (any affine map)."""

    def __init__(self, shape, affine_transformation, ctx=None):
        _need_torch()
        self.shape = _raster_shape(shape)
        t, self._inv = _forward(affine_transformation)
        self.pixel_area = abs(t[0] * t[3] - t[1] * t[2])
        self.ctx = ctx
        self.dev = _device.device_of(ctx)
        self._tensor_in = False
        self._zkey = self._count = None

    def add(self, points):
        p, n = self._device_cloud(points)
        if self._zkey is None and p.is_torch and self.ctx is None:
            self.dev = _device.device_of(None, p.x)
        self._planes()
        x, y, z, _ = _device_points(p._replace(intensity=None), self.dev)
        lib, c = _device.begin(self.dev, self.ctx)
        _lib.check(lib.obia_points_rasters_dev(c.handle, x.data_ptr(), y.data_ptr(), z.data_ptr(), n, self._inv, self.shape[0], self.shape[1],
                                               self._zkey.data_ptr(), self._count.data_ptr()))
        self.total += n
        return self

    def _planes(self):
        if self._zkey is None:
            self._zkey = torch.zeros(self.shape, dtype=torch.int32, device=f"cuda:{self.dev}")
            self._count = torch.zeros(self.shape, dtype=torch.int32, device=f"cuda:{self.dev}")
        return self._zkey, self._count

    def state(self, as_array=False):
        """the raw state: ``zkey`` and ``count`` (H, W) as int64 values of the uint32 planes"""
        zk, count = self._planes()
        return _device.out({"zkey": _u32(zk), "count": _u32(count)}, as_array or self._tensor_in)

    def result(self, as_array=False):
        """``{"chm", "density", "count"}``: (H, W) float32, float32 and int64.  ``chm`` is the highest finite height of a pixel's
        points, NaN where there is none; ``density`` = count / pixel area; ``count`` every point of the pixel.  NumPy unless a
        tensor was added; ``as_array=True`` leaves CUDA tensors whatever came in."""
        zk, count = self._planes()
        chm = torch.empty(self.shape, dtype=torch.float32, device=zk.device)
        density = torch.empty_like(chm)
        lib, c = _device.begin(self.dev, self.ctx)
        _lib.check(lib.obia_points_rasters_finish_dev(c.handle, self._zkey.data_ptr(), self._count.data_ptr(), self.shape[0], self.shape[1],
                                                      self.pixel_area, chm.data_ptr(), density.data_ptr()))
        count = _u32(self._count)
        return _device.out({"chm": chm, "density": density, "count": count}, as_array or self._tensor_in)


def points_to_rasters(points, affine_transformation, shape, as_array=False, ctx=None):
    """One shot of :class:`PointRasters`: ``{"chm", "density", "count"}`` of a cloud on the (H, W) grid of ``affine_transformation``."""
    return PointRasters(shape, affine_transformation, ctx=ctx).add(points).result(as_array=as_array)


def _u32(t):
    """a uint32 state array (kept as int32 bits) as int64 values"""
    return t.to(torch.int64) & 0xFFFFFFFF


class SegmentPoints(_Accumulator):
    """Points joined to the segments of a label raster.  Row ``label - start_label`` of every result belongs to ``label``;
    N = ``n_labels`` (default: the largest label - ``start_label`` + 1) as in ``zonal_stats``, so a row exists for a label that does
    not occur.  The vertical profile of a segment has ``nz = floor(z_max / dz) + 1`` bins of ``dz``; a point enters it when its
    height is finite, >= 0 and below ``nz * dz``."""

    def __init__(self, labels, affine_transformation, dz, z_max, start_label=1, n_labels=None, ctx=None):
        _need_torch()
        dz, z_max = float(dz), float(z_max)
        if not (math.isfinite(dz) and dz > 0.0):
            raise ValueError(f"dz must be finite and positive, got {dz!r}")
        if not (math.isfinite(z_max) and z_max >= 0.0):
            raise ValueError(f"z_max must be finite and not negative, got {z_max!r}")
        shape = tuple(labels.shape)
        if len(shape) != 2 or 0 in shape:
            raise ValueError(f"labels must be a non-empty (H, W) raster, got shape {shape}")
        self.shape = _raster_shape(shape)
        _, self._inv = _forward(affine_transformation)
        nzf = math.floor(z_max / dz) + 1
        if nzf > _lib.POINTS_MAX_NZ:
            raise NotImplementedError(f"z_max / dz gives {nzf} height bins, more than {_lib.POINTS_MAX_NZ}")
        self.dz, self.z_max, self.nz, self.start_label, self.ctx = dz, z_max, int(nzf), int(start_label), ctx
        self._tensor_in = _device.is_torch(labels)
        self.dev = _device.device_of(ctx, labels)
        self._labels = _device.as_dev(labels, torch.int32, self.dev)
        self.N = _n_labels(n_labels, self._labels, self.start_label)
        self._rows = max(self.N, 1)                              # the state of a raster without rows is one unused row
        if self._rows * self.nz >= 2 ** 31:
            raise NotImplementedError(f"{self._rows} segments x {self.nz} height bins: the profile must have fewer than 2^31 cells")
        d = self._labels.device
        self._profile = torch.zeros((self._rows, self.nz), dtype=torch.int32, device=d)
        self._top = torch.zeros(self._rows, dtype=torch.int32, device=d)
        self._n_int = torch.zeros(self._rows, dtype=torch.int32, device=d)
        self._s1 = torch.zeros(self._rows, dtype=torch.int64, device=d)
        self._s2 = torch.zeros(self._rows, dtype=torch.int64, device=d)
        self._counters = torch.zeros(4, dtype=torch.int64, device=d)
        self.has_intensity = None

    def add(self, points):
        p, n = self._device_cloud(points)
        if n and self.has_intensity is not None and self.has_intensity != (p.intensity is not None):
            raise ValueError("every add of one accumulator comes with Intensity, or none does")
        x, y, z, inten = _device_points(p, self.dev)
        lib, c = _device.begin(self.dev, self.ctx)
        H, W = self.shape
        _lib.check(lib.obia_points_segments_dev(c.handle, x.data_ptr(), y.data_ptr(), z.data_ptr(), None if inten is None else inten.data_ptr(),
                                                n, self._inv, self._labels.data_ptr(), H, W, self.start_label, self.N, self.nz, self.dz,
                                                self._profile.data_ptr(), self._top.data_ptr(), self._n_int.data_ptr(), self._s1.data_ptr(),
                                                self._s2.data_ptr(), self._counters.data_ptr()))
        if n:
            self.has_intensity = p.intensity is not None
        self.total += n
        return self

    def _out(self, v, as_array=False):
        return _device.out(v, as_array or self._tensor_in)

    def profile(self, as_array=False):
        """(N, nz) int64: the points of every segment per height bin"""
        return self._out(_u32(self._profile[:self.N]), as_array)

    def counters(self):
        """dict of Python ints: points ``outside`` the raster, inside but ``unlabelled`` (no row), with a row but ``out_of_range``
        (NaN, negative or above the profile) and ``in_profile``"""
        return dict(zip(COUNTERS, (int(v) for v in self._counters.cpu().tolist())))

    def state(self, as_array=False):
        """the raw state: ``profile`` (N, nz), ``top``, ``n_int`` (N,) as int64 values of the uint32 arrays, ``s1``, ``s2`` (N,)
        int64 bits of the uint64 sums, ``counters`` (4,) int64"""
        N = self.N
        return self._out({"profile": _u32(self._profile[:N]), "top": _u32(self._top[:N]), "n_int": _u32(self._n_int[:N]),
                          "s1": self._s1[:N].clone(), "s2": self._s2[:N].clone(), "counters": self._counters.clone()}, as_array)

    def columns(self, min_height=1.0, beer_lambert_constant=1.0, pad=False, as_array=False):
        """The (N,) columns ``n_points`` (int64), ``ch``, ``pai``, ``fhd``, ``mean_intensity``, ``variance_intensity`` (float64) and,
        with ``pad=True``, ``pad`` (N, nz): include/obia_points.h has every formula.  ``ch`` is the highest height of the profile;
        ``pai`` = log(n_all / n_below) / k, the Beer-Lambert gap fraction of the canopy above ``min_height`` (NaN without a return
        from below it); ``fhd`` the Shannon entropy of the profile above ``min_height``; the intensity pair is ``np.mean`` /
        ``np.var`` over every point of the segment.  Rows without points are NaN."""
        mh, k = float(min_height), float(beer_lambert_constant)
        if not math.isfinite(mh):
            raise ValueError(f"min_height must be finite, got {min_height!r}")
        if not (math.isfinite(k) and k > 0.0):
            raise ValueError(f"beer_lambert_constant must be finite and positive, got {beer_lambert_constant!r}")
        d = self._labels.device
        out = {"n_points": torch.empty(self._rows, dtype=torch.int64, device=d)}
        for name in COLUMNS[1:]:
            out[name] = torch.empty(self._rows, dtype=torch.float64, device=d)
        if pad:
            out["pad"] = torch.empty((self._rows, self.nz), dtype=torch.float64, device=d)
        lib, c = _device.begin(self.dev, self.ctx)
        if self.N:
            _lib.check(lib.obia_points_segment_columns_dev(c.handle, self._profile.data_ptr(), self._top.data_ptr(), self._n_int.data_ptr(),
                                                           self._s1.data_ptr(), self._s2.data_ptr(), self.N, self.nz, self.dz, mh, k,
                                                           *(out[name].data_ptr() for name in COLUMNS), out["pad"].data_ptr() if pad else None))
        return self._out({name: v[:self.N] for name, v in out.items()}, as_array)


def segment_point_stats(points, labels, affine_transformation, dz, z_max=None, start_label=1, n_labels=None, min_height=1.0,
                        beer_lambert_constant=1.0, pad=False, as_array=False, ctx=None):
    """One shot of :class:`SegmentPoints`: the columns of :meth:`SegmentPoints.columns` plus ``profile`` (N, nz) and ``counters``.
    ``z_max=None`` takes the largest finite height of the cloud (0 when there is none)."""
    _need_torch()
    p = as_points(points)
    if z_max is None:
        dev = _device.device_of(ctx, labels, p.x)
        z = _device.as_dev(p.z, torch.float32, dev)
        z = z[torch.isfinite(z)]
        z_max = max(float(z.max()), 0.0) if z.numel() else 0.0
    sp = SegmentPoints(labels, affine_transformation, dz, z_max, start_label=start_label, n_labels=n_labels, ctx=ctx)
    if p.is_torch:
        sp._tensor_in = True
    sp.add(p)
    res = sp.columns(min_height=min_height, beer_lambert_constant=beer_lambert_constant, pad=pad, as_array=as_array)
    res["profile"] = sp.profile(as_array=as_array)
    res["counters"] = sp.counters()
    return res


# ---------------------------------------------------------------------------------------------- height above ground (obia_ground.h)
def _raw_fields(pointcloud, names, optional=()):
    """``({name: values}, is_torch)`` of the named fields of a raw cloud (a dict, a structured array, or a list whose first element is
    one): all tensors or all arrays, one-dimensional and of one length; a CPU tensor is refused.  Touches no device."""
    if isinstance(pointcloud, (list, tuple)):
        if not pointcloud:
            raise ValueError("the point cloud list is empty")
        pointcloud = pointcloud[0]
    f = {name: _field(pointcloud, name) for name in tuple(names) + tuple(optional)}
    missing = [name for name in names if f[name] is None]
    if missing:
        raise ValueError(f"the point cloud has no {', '.join(missing)} field")
    f = {name: v for name, v in f.items() if v is not None}
    is_t = any(_device.is_torch(v) for v in f.values())
    if is_t and not all(_device.is_torch(v) for v in f.values()):
        raise ValueError("the fields of a point cloud must be all tensors or all arrays")
    if is_t:
        _device.device_of(None, *f.values())                                 # refuses CPU tensors
    else:
        f = {name: np.asarray(v) for name, v in f.items()}
    n = tuple(f[names[0]].shape)
    if len(n) != 1 or any(tuple(v.shape) != n for v in f.values()):
        raise ValueError("the fields of a point cloud must be one-dimensional and of one length")
    return f, is_t


def _check_query(count, max_distance):
    c = int(count)
    if c != count or not 1 <= c <= _lib.GROUND_MAX_COUNT:
        raise ValueError(f"count must be an integer in 1 .. {_lib.GROUND_MAX_COUNT}, got {count!r}")
    md = float(max_distance)
    if not md >= 0.0:
        raise ValueError(f"max_distance must not be negative (0: no limit), got {max_distance!r}")
    return c, md


def _ground_side(x0, x1, y0, y1, ng):
    """The cell side of the grid over ``ng`` ground points in [x0, x1] x [y0, y1]: about one point per cell.  With w, h the extent a
    side s gives at most (w / s + 2) (h / s + 2) = w h / s^2 + 2 (w + h) / s + 4 cells; s >= sqrt(w h / ng) and s >= 2 (w + h) / ng
    bound that by 2 ng + 4 for every extent and aspect ratio -- a single point, one (x, y), a line.  s is also at least 2^-29 of the
    largest coordinate, so that |v / s| <= 2^29 and cell indices fit (seeds._grid)."""
    w, h = x1 - x0, y1 - y0
    side = max(math.sqrt(w) * math.sqrt(h) / math.sqrt(ng), 2.0 * (w + h) / ng, max(abs(x0), abs(x1), abs(y0), abs(y1)) * 2.0 ** -29)
    if not math.isfinite(side):
        raise ValueError("the extent of the ground set is not finite")
    return side if side > 0.0 else 1.0


class GroundIndex:
    """The ground points of a cloud on a uniform grid, for any number of nearest-neighbour queries (include/obia_ground.h).

    ``ground``: a cloud with ``X``, ``Y``, ``Z`` (a dict of arrays or of CUDA tensors, or a structured array).  Points with a
    non-finite coordinate or elevation are dropped (``dropped`` counts them) and the index of a ground point is its position among
    the kept ones; no point left is a ``ValueError``.  ``n_ground``, ``side`` (the cell side) and ``shape`` = (ncy, ncx) describe
    the grid: ``ncy * ncx <= 4 * n_ground + 16`` for every extent, so memory is O(n_ground).

    The ground height of a query is the elevation of the nearest ground point (``count=1``) or the inverse-squared-distance mean of
    the ``count`` nearest, ties to the lower index, among those within ``max_distance`` (0: no limit); NaN when there is none or the
    query is not finite.  Every result is the same bits for every order and every cut of the queries."""

    def __init__(self, ground, *, ctx=None):
        _need_torch()
        f, is_t = _raw_fields(ground, ("X", "Y", "Z"))
        self._build(f["X"], f["Y"], f["Z"], is_t, ctx)

    @classmethod
    def from_cloud(cls, pointcloud, ground_class=2, *, ctx=None):
        """the index of the points of ``pointcloud`` whose ``Classification`` equals ``ground_class`` (2: ASPRS ground)"""
        _need_torch()
        f, is_t = _raw_fields(pointcloud, ("X", "Y", "Z"), optional=("Classification",))
        if "Classification" not in f:
            raise ValueError("the point cloud has no Classification field to take the ground from: pass the ground points")
        keep = f["Classification"] == int(ground_class)
        self = cls.__new__(cls)
        self._build(f["X"][keep], f["Y"][keep], f["Z"][keep], is_t, ctx)
        return self

    @staticmethod
    def _admit(ng):
        if ng == 0:
            raise ValueError("the ground set is empty: no point with finite X, Y and Z")
        if ng >= 2 ** 31:
            raise NotImplementedError("a ground set has fewer than 2^31 points")

    def _build(self, x, y, z, is_t, ctx):
        dev = _device.device_of(ctx, x, y, z)
        n_in = int(x.shape[0])
        if not is_t:                                                         # on the host: an empty set is refused before any device use
            x, y, z = (np.asarray(v).astype(np.float64, copy=False) for v in (x, y, z))
            keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
            if not keep.all():
                x, y, z = x[keep], y[keep], z[keep]
            self._admit(int(x.shape[0]))
        x, y, z = (_device.as_dev(v, torch.float64, dev) for v in (x, y, z))
        if is_t:
            keep = torch.isfinite(x) & torch.isfinite(y) & torch.isfinite(z)
            if not bool(keep.all()):
                x, y, z = x[keep], y[keep], z[keep]
        ng = int(x.shape[0])
        self._admit(ng)
        # the cell side: about one point per cell, (w / s + 2) (h / s + 2) <= 2 ng + 4 cells whatever the extent and the aspect, and
        # at least 2^-29 of the largest coordinate, so that |v / side| < 2^30 (seeds._grid)
        side = _ground_side(float(x.min()), float(x.max()), float(y.min()), float(y.max()), ng)
        lib, c = _device.begin(dev, ctx)
        cx = torch.empty(ng, dtype=torch.int32, device=x.device)
        cy = torch.empty(ng, dtype=torch.int32, device=x.device)
        while True:
            _lib.check(lib.obia_seedtab_cells_dev(c.handle, x.data_ptr(), y.data_ptr(), ng, side, cx.data_ptr(), cy.data_ptr()))
            cx0, cy0 = int(cx.min()), int(cy.min())
            ncx, ncy = int(cx.max()) - cx0 + 1, int(cy.max()) - cy0 + 1
            if ncx * ncy <= 4 * ng + 16:
                break
            side *= 2.0                                                      # not reached by the side above; the bound holds regardless
        key = (cy.to(torch.int64) - cy0) * ncx + (cx.to(torch.int64) - cx0)
        skey, order = torch.sort(key, stable=True)
        self._gx, self._gy, self._gz = x[order].contiguous(), y[order].contiguous(), z[order].contiguous()
        self._gidx = order.to(torch.int32).contiguous()
        self._cell_start = torch.searchsorted(skey, torch.arange(ncx * ncy + 1, dtype=torch.int64, device=x.device)).to(torch.int32).contiguous()
        self._cell0 = (cx0, cy0)
        self.ctx, self.dev, self._tensor_in = ctx, dev, is_t
        self.n_ground, self.side, self.shape, self.dropped = ng, side, (ncy, ncx), n_in - ng

    def _query(self, x, y, z, count, max_distance, with_m=False):
        """zg (n) float64, hag (n) float32 or None, m (n) uint8 or None of device tensors x, y float64 and z float64 or None"""
        n = int(x.shape[0])
        zg = torch.empty(n, dtype=torch.float64, device=x.device)
        hag = None if z is None else torch.empty(n, dtype=torch.float32, device=x.device)
        m = torch.empty(n, dtype=torch.uint8, device=x.device) if with_m else None
        if n:
            lib, c = _device.begin(self.dev, self.ctx)
            _lib.check(lib.obia_ground_query_dev(c.handle, self._gx.data_ptr(), self._gy.data_ptr(), self._gz.data_ptr(), self._gidx.data_ptr(),
                                                 self.n_ground, self._cell_start.data_ptr(), self.shape[1], self.shape[0], self._cell0[0],
                                                 self._cell0[1], self.side, x.data_ptr(), y.data_ptr(), None if z is None else z.data_ptr(), n,
                                                 count, max_distance, zg.data_ptr(), None if hag is None else hag.data_ptr(),
                                                 None if m is None else m.data_ptr()))
        return zg, hag, m

    def ground_z(self, x, y, count=1, max_distance=0.0):
        """(n) float64: the ground height under the points ``(x, y)``"""
        count, md = _check_query(count, max_distance)
        f, is_t = _raw_fields({"X": x, "Y": y}, ("X", "Y"))
        xd, yd = (_device.as_dev(f[k], torch.float64, self.dev) for k in ("X", "Y"))
        return _device.out(self._query(xd, yd, None, count, md)[0], is_t)

    def neighbours(self, x, y, count=1, max_distance=0.0):
        """(n) uint8: how many ground points the height of each query was formed from"""
        count, md = _check_query(count, max_distance)
        f, is_t = _raw_fields({"X": x, "Y": y}, ("X", "Y"))
        xd, yd = (_device.as_dev(f[k], torch.float64, self.dev) for k in ("X", "Y"))
        return _device.out(self._query(xd, yd, None, count, md, with_m=True)[2], is_t)

    def height_above_ground(self, pointcloud, count=1, max_distance=0.0):
        """(n) float32: ``Z`` -- the raw elevation, never ``HeightAboveGround`` -- minus the ground height under each point"""
        count, md = _check_query(count, max_distance)
        f, is_t = _raw_fields(pointcloud, ("X", "Y", "Z"))
        xd, yd, zd = (_device.as_dev(f[k], torch.float64, self.dev) for k in ("X", "Y", "Z"))
        return _device.out(self._query(xd, yd, zd, count, md)[1], is_t)

    def to_raster(self, shape, affine_transformation, count=1, max_distance=0.0):
        """The terrain model: (H, W) float32 of the ground height at the pixel centres of ``affine_transformation`` = [a, b, d, e,
        xoff, yoff], ``x = a (c + 0.5) + b (r + 0.5) + xoff`` and ``y`` likewise in float64.  NumPy unless the index was built from
        tensors."""
        count, md = _check_query(count, max_distance)
        H, W = _raster_shape(shape)
        t, _ = _forward(affine_transformation)
        if H * W >= 2 ** 31:
            raise NotImplementedError("a terrain raster has fewer than 2^31 pixels")
        d = self._gx.device
        cc = (torch.arange(W, dtype=torch.float64, device=d) + 0.5).reshape(1, W)
        rr = (torch.arange(H, dtype=torch.float64, device=d) + 0.5).reshape(H, 1)
        x = ((cc * t[0] + rr * t[1]) + t[4]).reshape(-1).contiguous()
        y = ((cc * t[2] + rr * t[3]) + t[5]).reshape(-1).contiguous()
        zg = self._query(x, y, None, count, md)[0]
        return _device.out(zg.to(torch.float32).reshape(H, W), self._tensor_in)


def _as_index(pointcloud, ground, ground_class, ctx):
    if isinstance(ground, GroundIndex):
        return ground
    if ground is None:
        return GroundIndex.from_cloud(pointcloud, ground_class=ground_class, ctx=ctx)
    return GroundIndex(ground, ctx=ctx)


def height_above_ground(pointcloud, ground=None, *, ground_class=2, count=1, max_distance=0.0, ctx=None):
    """(n) float32 heights of the points of ``pointcloud`` (``X``, ``Y``, raw ``Z``) above the ``count`` nearest ground points:
    ``ground=None`` takes the ground from the cloud's own ``Classification == ground_class``; otherwise ``ground`` is a
    :class:`GroundIndex` or a cloud of ground points.  A ground point comes out +-0 unless a lower-indexed ground point shares its
    ``(x, y)`` with another elevation."""
    _need_torch()
    _check_query(count, max_distance)
    _raw_fields(pointcloud, ("X", "Y", "Z"))
    return _as_index(pointcloud, ground, ground_class, ctx).height_above_ground(pointcloud, count=count, max_distance=max_distance)


def height_above_dtm(pointcloud, dtm, affine_transformation, ctx=None):
    """(n) float32 heights of the points of ``pointcloud`` above the terrain raster ``dtm`` (H, W) float32 with
    ``affine_transformation`` = [a, b, d, e, xoff, yoff]: raw ``Z`` minus the pixel that contains the point (the pixel rule of
    include/obia_points.h); NaN outside the raster and on a pixel that is not finite."""
    _need_torch()
    f, is_t = _raw_fields(pointcloud, ("X", "Y", "Z"))
    shape = tuple(dtm.shape)
    if len(shape) != 2 or 0 in shape:
        raise ValueError(f"dtm must be a non-empty (H, W) raster, got shape {shape}")
    H, W = _raster_shape(shape)
    _, inv = _forward(affine_transformation)
    dev = _device.device_of(ctx, f["X"], dtm)
    x, y, z = (_device.as_dev(f[k], torch.float64, dev) for k in ("X", "Y", "Z"))
    r = _device.as_dev(dtm, torch.float32, dev)
    n = int(x.shape[0])
    hag = torch.empty(n, dtype=torch.float32, device=x.device)
    if n:
        lib, c = _device.begin(dev, ctx)
        _lib.check(lib.obia_ground_dtm_dev(c.handle, x.data_ptr(), y.data_ptr(), z.data_ptr(), n, inv, r.data_ptr(), H, W, None, hag.data_ptr()))
    return _device.out(hag, is_t)


def normalize_heights(pointcloud, ground=None, *, dtm=None, affine_transformation=None, ground_class=2, count=1, max_distance=0.0, ctx=None):
    """A raw cloud as ``{"X", "Y", "HeightAboveGround"}`` (and ``"Intensity"`` when it has one), ready for ``points_to_rasters``,
    ``segment_point_stats`` and ``create_objects(pointcloud=)``: heights above ``dtm`` (with its ``affine_transformation``) when one
    is given, above the nearest ground points as in :func:`height_above_ground` otherwise."""
    _need_torch()
    f, _ = _raw_fields(pointcloud, ("X", "Y", "Z"), optional=("Intensity",))
    if dtm is not None:
        if ground is not None:
            raise ValueError("give the ground points or a dtm, not both")
        hag = height_above_dtm(pointcloud, dtm, affine_transformation, ctx=ctx)
    else:
        hag = height_above_ground(pointcloud, ground, ground_class=ground_class, count=count, max_distance=max_distance, ctx=ctx)
    out = {"X": f["X"], "Y": f["Y"], "HeightAboveGround": hag}
    if "Intensity" in f:
        out["Intensity"] = f["Intensity"]
    return out


# ------------------------------------------------------------------------------------------ ground filter (obia_groundfilter.h)
GROUND_COUNTERS = ("outside", "non_finite", "rejected", "ground")


def _check_radius(radius):
    r = int(radius)
    if r != radius or r < 1:
        raise ValueError(f"radius must be an integer of at least 1, got {radius!r}")
    if r > _lib.MORPH_MAX_RADIUS:
        raise NotImplementedError(f"radius must not exceed {_lib.MORPH_MAX_RADIUS}, got {r}")
    return r


def _grey(plane, radius, ops, ctx):
    _need_torch()
    r = _check_radius(radius)
    shape = tuple(plane.shape)
    if len(shape) != 2 or 0 in shape:
        raise ValueError(f"a plane must be a non-empty (H, W) raster, got shape {shape}")
    H, W = _raster_shape(shape)
    if H * W >= 2 ** 31:
        raise NotImplementedError("a plane has fewer than 2^31 cells")
    is_t = _device.is_torch(plane)
    dev = _device.device_of(ctx, plane)
    cur = _device.as_dev(plane, torch.float32, dev)
    tmp = torch.empty_like(cur)
    lib, c = _device.begin(dev, ctx)
    for op in ops:
        dst = torch.empty_like(cur)
        _lib.check(lib.obia_morph_filter_dev(c.handle, cur.data_ptr(), H, W, r, op, tmp.data_ptr(), dst.data_ptr()))
        cur = dst
    return _device.out(cur, is_t)


def grey_erosion(plane, radius, ctx=None):
    """(H, W) float32: the minimum over the ``(2 radius + 1)^2`` window around every cell, clipped to the raster.  NaN cells are empty:
    they are ignored, and the result is NaN where the window holds nothing else; infinities are data; ``1 <= radius <= 127``.  On
    planes without NaN this is ``scipy.ndimage.grey_erosion(size=(2 radius + 1,) * 2)`` bit for bit (include/obia_groundfilter.h).
    NumPy in, NumPy out; a CUDA tensor in, a CUDA tensor out."""
    return _grey(plane, radius, (0,), ctx)


def grey_dilation(plane, radius, ctx=None):
    """(H, W) float32: the maximum over the window, as :func:`grey_erosion` takes the minimum."""
    return _grey(plane, radius, (1,), ctx)


def grey_opening(plane, radius, ctx=None):
    """(H, W) float32: :func:`grey_erosion`, then :func:`grey_dilation` of the eroded plane: peaks narrower than the window are cut
    off, and an empty cell with neighbours that are not empty is filled."""
    return _grey(plane, radius, (0, 1), ctx)


def pmf_schedule(cell_size=1.0, slope=1.0, initial_distance=0.15, max_distance=2.5, max_window_size=33.0, exponential=True, base=2.0):
    """``(radii, dh)`` of a progressive morphological filter, two lists of one length (float64 arithmetic on the host): the
    half-widths ``r_k = round(base^k)`` (``exponential``) or ``round((k + 1) base)`` in cells for ``k = 0, 1, ...`` while the window
    ``w_k = 2 r_k + 1`` spans at most ``max_window_size`` (``w_k * cell_size <= max_window_size``), and the elevation thresholds
    ``dh_0 = initial_distance``, ``dh_k = min(slope (w_k - w_k-1) cell_size + initial_distance, max_distance)``.  The defaults give
    ``[1, 2, 4, 8, 16]`` and ``[0.15, 2.15, 2.5, 2.5, 2.5]``.  ``ValueError``: an empty schedule, more than 16 steps, a half-width
    that does not grow or exceeds 127, a ``cell_size`` that is not positive, a negative ``slope`` or distance, anything not finite."""
    v = dict(cell_size=float(cell_size), slope=float(slope), initial_distance=float(initial_distance), max_distance=float(max_distance),
             max_window_size=float(max_window_size), base=float(base))
    for name, x in v.items():
        if not math.isfinite(x):
            raise ValueError(f"{name} must be finite, got {x!r}")
    if v["cell_size"] <= 0.0:
        raise ValueError(f"cell_size must be positive, got {cell_size!r}")
    for name in ("slope", "initial_distance", "max_distance", "max_window_size"):
        if v[name] < 0.0:
            raise ValueError(f"{name} must not be negative, got {v[name]!r}")
    if v["base"] <= 0.0:
        raise ValueError(f"base must be positive, got {base!r}")
    radii, dh = [], []
    k, w_prev = 0, None
    while True:
        rf = round(v["base"] ** k) if exponential else round((k + 1) * v["base"])
        w = 2 * rf + 1
        if not w * v["cell_size"] <= v["max_window_size"]:
            break
        if rf < 1 or rf > _lib.MORPH_MAX_RADIUS or (radii and rf <= radii[-1]):
            raise ValueError(f"step {k}: the half-width must grow from step to step within 1 .. {_lib.MORPH_MAX_RADIUS} cells, got {rf}"
                             f" after {radii}")
        if len(radii) == _lib.GF_MAX_STEPS:
            raise ValueError(f"the schedule has more than {_lib.GF_MAX_STEPS} steps")
        radii.append(int(rf))
        dh.append(v["initial_distance"] if w_prev is None else min(v["slope"] * (w - w_prev) * v["cell_size"] + v["initial_distance"], v["max_distance"]))
        w_prev = w
        k += 1
    if not radii:
        raise ValueError(f"the schedule is empty: the first window, {3 * v['cell_size']!r}, exceeds max_window_size = {max_window_size!r}")
    return radii, dh


def _check_schedule(radii, dh):
    radii, dh = [int(r) for r in radii], [float(d) for d in dh]
    if not radii or len(radii) != len(dh) or len(radii) > _lib.GF_MAX_STEPS:
        raise ValueError(f"a schedule has 1 .. {_lib.GF_MAX_STEPS} steps, radii and dh of one length")
    if any(r < 1 or r > _lib.MORPH_MAX_RADIUS for r in radii) or any(not (math.isfinite(d) and d >= 0.0) for d in dh):
        raise ValueError(f"a schedule has radii within 1 .. {_lib.MORPH_MAX_RADIUS} and finite distances that are not negative")
    return radii, dh


class GroundFilter:
    """The ground points of an unclassified cloud by a progressive morphological filter on the grid of a raster
    (include/obia_groundfilter.h; modelled on Zhang et al. 2003 and PDAL's ``filters.pmf``, NOT compared with PDAL).

    ``add`` pieces of the cloud (``X``, ``Y``, raw ``Z``) in any number of calls -- the state is the minimum elevation of every
    cell, the same bits for every order and cut -- then ``finish``: ``zmin`` is opened with the growing windows of the schedule
    ``radii`` (cells), and ``threshold`` is the lowest ``surface_k + dh_k`` over the steps.  ``classify(piece)`` then gives the
    (n) bool ground flags: a point is ground iff it lies inside the raster, its ``Z`` is finite and ``Z <= threshold[cell]``.

    After ``finish``: ``zmin``, ``surface`` (the last opening), ``threshold`` (H, W) float32; ``counters`` sums what ``classify``
    saw; a one-shot :func:`ground_filter` also holds ``ground``.  ``shape``, ``affine_transformation``, ``cell_size``, ``radii`` and
    ``dh`` describe the grid and the schedule."""

    def __init__(self, shape, affine_transformation, radii, dh, ctx=None):
        _need_torch()
        self.shape = _raster_shape(shape)
        if self.shape[0] * self.shape[1] >= 2 ** 31:
            raise NotImplementedError("the grid of a ground filter has fewer than 2^31 cells")
        t, self._inv = _forward(affine_transformation)
        if t[1] != 0.0 or t[2] != 0.0 or abs(t[0]) != abs(t[3]):
            raise ValueError(f"the grid of a ground filter is axis-aligned with square pixels, got {t}")
        self.affine_transformation, self.cell_size = t, abs(t[0])
        self.radii, self.dh = _check_schedule(radii, dh)
        self.ctx = ctx
        self.dev = _device.device_of(ctx)
        self._tensor_in = False
        self._keys = self._zmin = self._surface = self._threshold = self._counters = None
        self.ground = None
        self.total = 0                                                       # points added, then points classified

    def _cloud(self, points):
        f, is_t = _raw_fields(points, ("X", "Y", "Z"))
        n = int(f["X"].shape[0])
        if n >= 2 ** 31:                                                     # (the state holds minima, not counts: any number of pieces)
            raise NotImplementedError("one piece holds fewer than 2^31 points: cut the cloud")
        if self._keys is None and self._counters is None and is_t and self.ctx is None:
            self.dev = _device.device_of(None, f["X"])
        self._tensor_in = self._tensor_in or is_t
        return tuple(_device.as_dev(f[k], torch.float64, self.dev) for k in ("X", "Y", "Z")), n, is_t

    def add(self, points):
        if self._threshold is not None:
            raise RuntimeError("the filter is finished: classify, or start another")
        (x, y, z), n, _ = self._cloud(points)
        if self._keys is None:
            self._keys = torch.zeros(self.shape, dtype=torch.int32, device=f"cuda:{self.dev}")
        lib, c = _device.begin(self.dev, self.ctx)
        _lib.check(lib.obia_gf_cell_min_dev(c.handle, x.data_ptr(), y.data_ptr(), z.data_ptr(), n, self._inv, self.shape[0], self.shape[1],
                                            self._keys.data_ptr()))
        self.total += n
        return self

    def finish(self):
        """``zmin`` from the state, then the 4 K line passes of the schedule: ``surface`` and ``threshold``"""
        if self._keys is None:
            self._keys = torch.zeros(self.shape, dtype=torch.int32, device=f"cuda:{self.dev}")
        H, W = self.shape
        d = self._keys.device
        zmin, tmp0, tmp1, surface, thresh = (torch.empty(self.shape, dtype=torch.float32, device=d) for _ in range(5))
        K = len(self.radii)
        lib, c = _device.begin(self.dev, self.ctx)
        _lib.check(lib.obia_gf_cell_min_finish_dev(c.handle, self._keys.data_ptr(), H, W, zmin.data_ptr()))
        _lib.check(lib.obia_gf_threshold_dev(c.handle, zmin.data_ptr(), H, W, (ctypes.c_int32 * K)(*self.radii), (ctypes.c_double * K)(*self.dh), K,
                                             tmp0.data_ptr(), tmp1.data_ptr(), surface.data_ptr(), thresh.data_ptr()))
        self._zmin, self._surface, self._threshold = zmin, surface, thresh
        self._counters = torch.zeros(4, dtype=torch.int64, device=d)
        self.total = 0                                                       # what classify counts starts here
        return self

    def classify(self, points):
        """(n) bool: the ground flags of a piece of the cloud; NumPy for arrays, a CUDA tensor for tensors"""
        if self._threshold is None:
            raise RuntimeError("finish the filter before it classifies")
        (x, y, z), n, is_t = self._cloud(points)
        flags = torch.empty(n, dtype=torch.uint8, device=x.device)
        if n:
            lib, c = _device.begin(self.dev, self.ctx)
            _lib.check(lib.obia_gf_classify_dev(c.handle, x.data_ptr(), y.data_ptr(), z.data_ptr(), n, self._inv, self._threshold.data_ptr(),
                                                self.shape[0], self.shape[1], flags.data_ptr(), self._counters.data_ptr()))
        self.total += n
        return _device.out(flags.to(torch.bool), is_t)

    def _plane(self, t):
        if t is None:
            raise RuntimeError("finish the filter first")
        return _device.out(t, self._tensor_in)

    zmin = property(lambda self: self._plane(self._zmin))
    surface = property(lambda self: self._plane(self._surface))
    threshold = property(lambda self: self._plane(self._threshold))

    @property
    def counters(self):
        """dict of Python ints over every ``classify`` so far: points ``outside`` the raster, inside with a ``non_finite`` Z,
        ``rejected`` and ``ground``"""
        if self._counters is None:
            raise RuntimeError("finish the filter first")
        return dict(zip(GROUND_COUNTERS, (int(v) for v in self._counters.cpu().tolist())))


def _north_up_grid(f, is_t, cell):
    """shape and transform of the north-up grid of ``cell`` over the points with finite X and Y, anchored at floor(min X / cell) cell and
    ceil(max Y / cell) cell; arrays are looked at on the host, tensors where they are"""
    x, y = f["X"], f["Y"]
    if is_t:
        x, y = x.to(torch.float64), y.to(torch.float64)
        keep = torch.isfinite(x) & torch.isfinite(y)
        x, y = x[keep], y[keep]
    else:
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        keep = np.isfinite(x) & np.isfinite(y)
        x, y = x[keep], y[keep]
    if int(x.shape[0]) == 0:
        raise ValueError("the point cloud has no point with finite X and Y to lay a grid over")
    x0, x1, y0, y1 = float(x.min()), float(x.max()), float(y.min()), float(y.max())
    left, top = math.floor(x0 / cell) * cell, math.ceil(y1 / cell) * cell
    t = [cell, 0.0, 0.0, -cell, left, top]
    inv = invert_affine(t)
    # the last column and row by the pixel rule's own arithmetic, so that no point falls off the far edges
    W = int(math.floor(inv[0] * x1 + inv[1] * y0 + inv[4])) + 1
    H = int(math.floor(inv[2] * x1 + inv[3] * y0 + inv[5])) + 1
    if not (1 <= H < 2 ** 31 and 1 <= W < 2 ** 31):
        raise ValueError(f"cell_size {cell!r} gives a grid of {H} x {W} cells over the cloud")
    return (H, W), t


def ground_filter(pointcloud, cell_size=1.0, slope=1.0, initial_distance=0.15, max_distance=2.5, max_window_size=33.0, exponential=True,
                  base=2.0, *, affine_transformation=None, shape=None, ctx=None):
    """The ground points of an unclassified cloud (``X``, ``Y``, raw ``Z``; a dict of arrays or of CUDA tensors, or a structured
    array): a finished :class:`GroundFilter` whose ``ground`` (n) bool marks them, with ``threshold``, ``surface``, ``zmin``,
    ``affine_transformation``, ``shape``, ``radii``, ``dh`` and ``counters``.

    Without ``affine_transformation`` the grid is north-up with cells of ``cell_size``, anchored at ``floor(min X / cell) cell`` and
    ``ceil(max Y / cell) cell`` over the points with finite coordinates (none: ``ValueError``).  With one -- [a, b, d, e, xoff, yoff]
    and ``shape`` = (H, W) -- the grid is the caller's: axis-aligned, square pixels (else ``ValueError``), and ``cell_size`` is taken
    from it.  The other parameters are :func:`pmf_schedule`'s.  Selecting last returns is the caller's step."""
    _need_torch()
    f, is_t = _raw_fields(pointcloud, ("X", "Y", "Z"))
    if affine_transformation is not None:
        if shape is None:
            raise ValueError("affine_transformation comes with the shape (H, W) of its raster")
        t, _ = _forward(affine_transformation)
        if t[1] != 0.0 or t[2] != 0.0 or abs(t[0]) != abs(t[3]):
            raise ValueError(f"the grid of a ground filter is axis-aligned with square pixels, got {t}")
        cell = abs(t[0])
        radii, dh = pmf_schedule(cell, slope, initial_distance, max_distance, max_window_size, exponential, base)
    else:
        if shape is not None:
            raise ValueError("shape comes with the affine_transformation of its raster")
        cell = float(cell_size)
        radii, dh = pmf_schedule(cell, slope, initial_distance, max_distance, max_window_size, exponential, base)
        shape, t = _north_up_grid(f, is_t, cell)
    gf = GroundFilter(shape, t, radii, dh, ctx=ctx)
    gf.add(pointcloud).finish()
    gf.ground = gf.classify(pointcloud)
    return gf


def classify_ground(pointcloud, cell_size=1.0, slope=1.0, initial_distance=0.15, max_distance=2.5, max_window_size=33.0, exponential=True,
                    base=2.0, *, affine_transformation=None, shape=None, ground_class=2, other_class=1, ctx=None):
    """The fields of ``pointcloud`` as a dict plus ``Classification`` (uint8): ``ground_class`` where :func:`ground_filter` finds
    ground, ``other_class`` elsewhere.  ``GroundIndex.from_cloud``, ``height_above_ground`` and ``normalize_heights`` take the result
    as it is: ``normalize_heights(classify_ground(raw))`` is the chain from a raw cloud to heights above ground."""
    for name, v in (("ground_class", ground_class), ("other_class", other_class)):
        if int(v) != v or not 0 <= int(v) <= 255:
            raise ValueError(f"{name} must be an integer in 0 .. 255, got {v!r}")
    gf = ground_filter(pointcloud, cell_size, slope, initial_distance, max_distance, max_window_size, exponential, base,
                       affine_transformation=affine_transformation, shape=shape, ctx=ctx)
    if isinstance(pointcloud, (list, tuple)):
        pointcloud = pointcloud[0]
    if isinstance(pointcloud, dict):
        out = dict(pointcloud)
    else:
        out = {name: pointcloud[name] for name in pointcloud.dtype.names}
    g = gf.ground
    if _device.is_torch(g):
        out["Classification"] = torch.where(g, int(ground_class), int(other_class)).to(torch.uint8)
    else:
        out["Classification"] = np.where(g, np.uint8(ground_class), np.uint8(other_class)).astype(np.uint8)
    return out
