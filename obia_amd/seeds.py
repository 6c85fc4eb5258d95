"""The seed points of obia/utils/seeds.py on the GPU: ``make_chm_seeds``, ``make_density_seeds`` and ``make_canonical_seeds``.

Peaks (seeds.py:11-102) are a Gaussian smooth, a (2d+1)^2 maximum filter, a threshold and the row-major list of the surviving
pixels; the merge (seeds.py:139-165, 215-231) evaluates the cost-aware distance of every pair of seeds and takes the connected
components of ``D <= merge_radius`` -- what ``DBSCAN(min_samples=1, metric="precomputed")`` returns -- without ever storing the
matrix.  Both run in libobia_hip.so (seeds.hip).  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out; there is no CPU
path.  Seed tables are plain dicts of arrays (the reference's GeoDataFrame columns); a ``.gpkg`` path is written / read with
obia_amd.geopackage.

Not built: the host-side table options of ``make_canonical_seeds`` (``keep_all_stage1=False``, ``z_thresh``,
``dz_merge``, ``max_per_cluster``, ``nms_base`` / ``nms_scale``) and the CHM resampling of seeds without heights."""
import ctypes
import os
import sqlite3
import struct

import numpy as np

from . import _device, _lib
from .cost import _as_dev, _is_path, _need_torch, _plane, _shape

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

SAMPLES = 12                       # make_canonical_seeds calls _build_distance_matrix(..., samples=12)
_CHUNK = 4096                      # pixels per compaction block (seeds.hip)
MAX_MIN_DIST_PX = 32


def line_samples(samples):
    """The interior float32 values of np.linspace(0, 1, samples + 2, dtype=float32) as float64 (seeds.py:156): what
    ``xi + ts * dx`` multiplies once ``dx`` (an np.float64 scalar) has promoted them."""
    return np.linspace(0.0, 1.0, int(samples) + 2, dtype=np.float32)[1:-1].astype(np.float64)


def invert_affine(affine_transformation):
    """``~Affine(a, b, xoff, d, e, yoff)`` as the affine package computes it, for ``image.affine_transformation`` =
    [a, b, d, e, xoff, yoff]: (ra, rb, rc, rd, re, rf) with col = ra x + rb y + rc, row = rd x + re y + rf."""
    sa, sb, sd, se, sc, sf = [float(v) for v in affine_transformation]
    det = sa * se - sb * sd
    if det == 0.0:
        raise ValueError("singular affine transformation")
    idet = 1.0 / det
    ra, rb, rd, re = se * idet, -sb * idet, -sd * idet, sa * idet
    return [ra, rb, -sc * ra - sf * rb, rd, re, -sc * rd - sf * re]


def _check_peak_args(name, shape, min_dist_px, gauss_sigma):
    if len(shape) != 2:
        raise ValueError(f"{name} must be (H, W), got shape {shape}")
    if 0 in shape:
        raise ValueError(f"{name} is empty")
    if int(min_dist_px) != min_dist_px or not 0 <= int(min_dist_px) <= MAX_MIN_DIST_PX:
        raise ValueError(f"min_dist_px must be an integer in 0..{MAX_MIN_DIST_PX}, got {min_dist_px!r}")
    if not float(gauss_sigma) >= 0.0:
        raise ValueError(f"gauss_sigma must be >= 0, got {gauss_sigma!r}")
    if shape[0] * shape[1] > 2 ** 31 - 1 - _CHUNK:
        raise ValueError(f"{name} has more than 2^31 pixels")


def detect_peaks(arr, v_min, min_dist_px, sigma=0, ctx=None, _smooth=False):
    """_detect_chm_peaks / _detect_den_peaks (seeds.py:11-35) on a float32 (H, W) plane: (row, col, smoothed value, raw value)
    of the pixels with g == maximum_filter(g, 2 * min_dist_px + 1) and g >= v_min, g = gaussian_filter(arr, sigma) when
    sigma > 0, in np.where order (int32, int32, float32, float32).  A NaN never wins the maximum and is never a peak.
    ``_smooth=True`` appends the smoothed plane (test hook)."""
    _need_torch()
    _check_peak_args("arr", _shape(arr), min_dist_px, sigma)
    is_t = _device.is_torch(arr)
    dev = _device.device_of(ctx, arr)
    x = _as_dev(arr, torch.float32, dev)
    H, W = x.shape
    n = H * W
    nchunks = -(-n // _CHUNK)
    sigma = float(sigma)
    lib, c = _device.begin(dev, ctx)
    smooth = torch.empty((H, W), dtype=torch.float32, device=x.device) if sigma > 0 else x
    flags = torch.empty(nchunks * _CHUNK, dtype=torch.uint8, device=x.device)
    offsets = torch.empty(nchunks + 1, dtype=torch.int32, device=x.device)
    count = ctypes.c_int64(0)
    _lib.check(lib.obia_seeds_peaks_dev(c.handle, x.data_ptr(), H, W, sigma, int(min_dist_px), float(np.float32(v_min)),
                                        smooth.data_ptr() if sigma > 0 else None, flags.data_ptr(), offsets.data_ptr(),
                                        ctypes.byref(count)))
    k = int(count.value)
    rows = torch.empty(k, dtype=torch.int32, device=x.device)
    cols = torch.empty(k, dtype=torch.int32, device=x.device)
    gval = torch.empty(k, dtype=torch.float32, device=x.device)
    rval = torch.empty(k, dtype=torch.float32, device=x.device)
    _lib.check(lib.obia_seeds_peaks_gather_dev(c.handle, x.data_ptr(), smooth.data_ptr(), flags.data_ptr(), offsets.data_ptr(), H, W, k,
                                               rows.data_ptr(), cols.data_ptr(), gval.data_ptr(), rval.data_ptr()))
    _device.end(lib, c)
    out = (rows, cols, gval, rval) + ((smooth,) if _smooth else ())
    return _device.out(out, is_t)


def _table_name(path):
    return os.path.splitext(os.path.basename(os.fspath(path)))[0]


def _point_wkb(x, y):
    return struct.pack("<BI2d", 1, 1, float(x), float(y))


def write_seed_points(path, seeds, table=None, srs_epsg=None):
    """One point layer: every key of ``seeds`` other than x / y / row / col becomes a column."""
    from .geopackage import write_geopackage
    host = {k: (v.cpu().numpy() if _device.is_torch(v) else np.asarray(v)) for k, v in seeds.items()}
    wkbs = [_point_wkb(x, y) for x, y in zip(host["x"], host["y"])]
    cols = {k: v for k, v in host.items() if k not in ("x", "y", "row", "col")}
    d = os.path.dirname(os.path.abspath(os.fspath(path)))
    os.makedirs(d, exist_ok=True)
    return write_geopackage(os.fspath(path), wkbs, cols, table=table or _table_name(path), srs_epsg=srs_epsg)


def read_seed_points(path):
    """The first feature table of a seed GeoPackage as a dict of NumPy arrays (x, y from the point geometries)."""
    from .geopackage import read_geopackage
    con = sqlite3.connect(os.fspath(path))
    try:
        row = con.execute("SELECT table_name FROM gpkg_contents WHERE data_type = 'features' ORDER BY table_name").fetchone()
    finally:
        con.close()
    if not row:
        raise ValueError(f"{path}: no feature table")
    wkbs, cols, _ = read_geopackage(os.fspath(path), table=row[0])
    xy = np.empty((len(wkbs), 2), np.float64)
    for i, w in enumerate(wkbs):
        if struct.unpack_from("<I", w, 1)[0] != 1:
            raise ValueError(f"{path}: seed geometries must be points")
        xy[i] = struct.unpack_from("<2d", w, 5)
    out = {k: np.asarray(v) for k, v in cols.items()}
    out["x"], out["y"] = xy[:, 0].copy(), xy[:, 1].copy()
    return out


def _make_seeds(raster, seeds_gpkg, v_min, min_dist_px, gauss_sigma, affine_transformation, ctx, name, column, empty_message):
    _need_torch()
    raster = _plane(raster, None, name)
    is_t = _device.is_torch(raster)
    rows, cols, _, raw = detect_peaks(raster if is_t else np.asarray(raster), v_min, min_dist_px, gauss_sigma, ctx=ctx)
    if len(rows) == 0:
        raise SystemExit(empty_message)
    a, b, d, e, xoff, yoff = [float(v) for v in (affine_transformation if affine_transformation is not None else (1, 0, 0, 1, 0, 0))]
    f64 = torch.float64 if is_t else np.float64
    cc = (cols.to(f64) if is_t else cols.astype(f64)) + 0.5
    rr = (rows.to(f64) if is_t else rows.astype(f64)) + 0.5
    ids = torch.arange(len(rows), dtype=torch.int64, device=rows.device) if is_t else np.arange(len(rows), dtype=np.int64)
    out = {"id": ids, "row": rows, "col": cols, "x": a * cc + b * rr + xoff, "y": d * cc + e * rr + yoff, column: raw}
    if seeds_gpkg is not None:
        write_seed_points(seeds_gpkg, out)
    return out


def make_chm_seeds(chm, seeds_gpkg=None, h_min_m=2.5, min_dist_px=3, gauss_sigma=1, affine_transformation=None, ctx=None):
    """make_chm_seeds (seeds.py:72-102): local maxima of the (smoothed) canopy height model that reach ``h_min_m``.

    chm : (H, W) array or CUDA tensor (taken as float32, NaN = nodata) or a raster path (GDAL).
    affine_transformation : ``image.affine_transformation`` [a, b, d, e, xoff, yoff]; None = pixel coordinates.
    Returns a dict: id, row, col (np.where order), x, y (pixel centres: a (col + 0.5) + b (row + 0.5) + xoff, float64) and
    ch_max = chm[row, col] of the unsmoothed raster.  ``seeds_gpkg``: also write them as a point layer.
    No peak raises SystemExit as the reference does."""
    return _make_seeds(chm, seeds_gpkg, h_min_m, min_dist_px, gauss_sigma, affine_transformation, ctx, "chm", "ch_max",
                       "No peaks found – adjust H_MIN_M or check CHM.")


def make_density_seeds(density, seeds_gpkg=None, d_min=4.5, min_dist_px=4, gauss_sigma=2, affine_transformation=None, ctx=None):
    """make_density_seeds (seeds.py:38-69): the same on a point-density raster; the value column is ``den_max``."""
    return _make_seeds(density, seeds_gpkg, d_min, min_dist_px, gauss_sigma, affine_transformation, ctx, "density", "den_max",
                       "No density peaks found — lower D_MIN or check raster.")


# ---------------------------------------------------------------------------------------------------------------- merge
def _pair_call(fn, c, xs, ys, cost, inv6, weight, xy_thresh, samples, *rest):
    ts = np.ascontiguousarray(line_samples(samples))
    H, W = cost.shape
    return fn(c.handle, xs.data_ptr(), ys.data_ptr(), xs.numel(), cost.data_ptr(), H, W, (ctypes.c_double * 6)(*inv6), float(weight),
              float(xy_thresh), int(samples), ts.ctypes.data_as(ctypes.c_void_p), *rest)


def _check_pair_args(xs, ys, cost, inv6):
    if len(_shape(xs)) != 1 or _shape(xs) != _shape(ys):
        raise ValueError(f"xs and ys must be 1-D and of one length, got {_shape(xs)} and {_shape(ys)}")
    if _shape(xs)[0] == 0:
        raise ValueError("no seeds")
    if len(_shape(cost)) != 2 or 0 in _shape(cost):
        raise ValueError(f"cost must be a non-empty (H, W) raster, got shape {_shape(cost)}")
    if len(inv6) != 6:
        raise ValueError("the inverse geotransform has six values (a, b, c, d, e, f)")


def pair_distances(xs, ys, cost, inv6, weight, xy_thresh, samples=SAMPLES, ctx=None):
    """_build_distance_matrix (seeds.py:139-165) as a full float32 (n, n) matrix, n <= 512: a test hook of the pair function."""
    _need_torch()
    _check_pair_args(xs, ys, cost, inv6)
    is_t = _device.is_torch(xs)
    dev = _device.device_of(ctx, xs, ys, cost)
    x, y, cst = _as_dev(xs, torch.float64, dev), _as_dev(ys, torch.float64, dev), _as_dev(cost, torch.float32, dev)
    lib, c = _device.begin(dev, ctx)
    D = torch.empty((x.numel(), x.numel()), dtype=torch.float32, device=x.device)
    _lib.check(_pair_call(lib.obia_seeds_pair_matrix_dev, c, x, y, cst, inv6, weight, xy_thresh, samples, D.data_ptr()))
    _device.end(lib, c)
    return _device.out(D, is_t)


def merge_clusters(xs, ys, cost, inv6, weight, xy_thresh, eps, samples=SAMPLES, prune=None, ctx=None):
    """Labels of DBSCAN(eps, min_samples=1, metric="precomputed") on the distance matrix of the seeds: connected components
    of D <= float32(eps), numbered by smallest member (int32).  ``prune``: None = skip the gathers of pairs that cannot link
    when weight >= 0 and the cost has no negative value; False = evaluate every pair (same result)."""
    _need_torch()
    _check_pair_args(xs, ys, cost, inv6)
    is_t = _device.is_torch(xs)
    dev = _device.device_of(ctx, xs, ys, cost)
    x, y, cst = _as_dev(xs, torch.float64, dev), _as_dev(ys, torch.float64, dev), _as_dev(cost, torch.float32, dev)
    nonneg = False if prune is False else bool(float(weight) >= 0 and bool((cst >= 0).all()))
    lib, c = _device.begin(dev, ctx)
    cl = torch.empty(x.numel(), dtype=torch.int32, device=x.device)
    ncl = ctypes.c_int(0)
    _lib.check(_pair_call(lib.obia_seeds_pair_link_dev, c, x, y, cst, inv6, weight, xy_thresh, samples, float(eps), int(nonneg),
                          cl.data_ptr(), ctypes.byref(ncl)))
    _device.end(lib, c)
    return _device.out(cl, is_t)


def pair_stats(xs, ys, cost, inv6, weight, xy_thresh, samples=SAMPLES, ctx=None):
    """(min, np.median, max) of the upper triangle of the distance matrix as float32, without the matrix; all NaN when any
    distance is NaN.  Fewer than two seeds raise ValueError (the reference's ``dvals.min()`` of an empty array does)."""
    _need_torch()
    _check_pair_args(xs, ys, cost, inv6)
    if _shape(xs)[0] < 2:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")
    dev = _device.device_of(ctx, xs, ys, cost)
    x, y, cst = _as_dev(xs, torch.float64, dev), _as_dev(ys, torch.float64, dev), _as_dev(cost, torch.float32, dev)
    lib, c = _device.begin(dev, ctx)
    st = (ctypes.c_float * 4)()
    n_nan = ctypes.c_int64(0)
    _lib.check(_pair_call(lib.obia_seeds_pair_stats_dev, c, x, y, cst, inv6, weight, xy_thresh, samples, st, ctypes.byref(n_nan)))
    _device.end(lib, c)
    v = np.array(list(st), np.float32)
    return v[0], np.mean(v[1:3]), v[3]


_NOT_BUILT = "is a host-side table option of the reference that obia_amd does not build (DESIGN.md, section 6)"


def _seed_table(s, origin):
    if _is_path(s):
        s = read_seed_points(s)
    if not isinstance(s, dict) or "x" not in s or "y" not in s:
        raise ValueError(f"{origin} seeds must be a dict with x and y (what make_{'chm' if origin == 'chm' else 'density'}_seeds returns) or a "
                         ".gpkg path")
    col = "ch_max" if origin == "chm" else "den_max"
    h = s.get(col, s.get("height"))
    if h is None:
        raise NotImplementedError(f"{origin} seeds without a {col} / height column: sampling the CHM at the seed points "
                                  "(_add_chm_height) is not built")
    return s["x"], s["y"], h


def make_canonical_seeds(chm_seeds, den_seeds, cost_surface, out_path=None, merge_radius=1.5, cost_weight=0.5, xy_thresh=0.8,
                         debug_dist=True, nodata_cost=1, cost_nodata=None, cost_affine=None, ctx=None, z_thresh=-1, dz_merge=0,
                         keep_all_stage1=True, max_per_cluster=0, nms_base=0, nms_scale=0):
    """make_canonical_seeds (seeds.py:168-262) at its defaults: CHM seeds then density seeds, the cost-aware distance between
    every two of them (12 samples of the cost surface along the line), clusters = connected components of D <= merge_radius.

    chm_seeds, den_seeds : the dicts make_chm_seeds / make_density_seeds return, or .gpkg paths of such layers.
    cost_surface : (H, W) array / CUDA tensor (what make_cost_surface returns) or a raster path (GDAL).
    cost_nodata  : value replaced by ``nodata_cost`` (the raster's nodata value; None = nothing is replaced).
    cost_affine  : [a, b, d, e, xoff, yoff] of the cost raster; None = pixel coordinates.
    Returns a dict id, cluster (int32), ch_max (float32), origin ("chm" / "density"), x, y; arrays are CUDA tensors when the cost
    surface is one (origin stays a NumPy array of str).  ``out_path``: also write the layer "canonical_seeds".
    Stage 1 (``cluster1``) does not reach the output at the defaults and is not computed; the options that would use it raise
    NotImplementedError, as do seeds without heights."""
    if not keep_all_stage1:
        raise NotImplementedError(f"keep_all_stage1=False {_NOT_BUILT}")
    if z_thresh >= 0:
        raise NotImplementedError(f"z_thresh >= 0 {_NOT_BUILT}")
    if dz_merge > 0:
        raise NotImplementedError(f"dz_merge > 0 {_NOT_BUILT}")
    if max_per_cluster > 0:
        raise NotImplementedError(f"max_per_cluster > 0 {_NOT_BUILT}")
    if nms_base > 0 or nms_scale > 0:
        raise NotImplementedError(f"nms_base / nms_scale > 0 {_NOT_BUILT}")
    cx, cy, ch = _seed_table(chm_seeds, "chm")
    dx, dy, dh = _seed_table(den_seeds, "density")
    inv6 = invert_affine(cost_affine if cost_affine is not None else (1, 0, 0, 1, 0, 0))
    _need_torch()
    cost_surface = _plane(cost_surface, None, "cost_surface")
    if 0 in _shape(cost_surface):
        raise ValueError("cost_surface is empty")
    is_t = _device.is_torch(cost_surface)
    dev = _device.device_of(ctx, cost_surface, cx, dx)
    xs = torch.cat([_as_dev(cx, torch.float64, dev), _as_dev(dx, torch.float64, dev)])
    ys = torch.cat([_as_dev(cy, torch.float64, dev), _as_dev(dy, torch.float64, dev)])
    hs = torch.cat([_as_dev(ch, torch.float32, dev), _as_dev(dh, torch.float32, dev)])
    n_chm = int(_shape(cx)[0])
    n = int(xs.numel())
    if n == 0:
        raise SystemExit("No seeds after CHM sampling.")
    cost = _as_dev(cost_surface, torch.float32, dev)
    if cost_nodata is not None:
        # cost_arr[cost_arr == nodata] = nodata_cost on a float32 array: the comparison promotes a Python nodata weakly
        cost = torch.where(cost == float(np.float32(cost_nodata)), torch.full_like(cost, float(np.float32(nodata_cost))), cost)
    if debug_dist:
        lo, med, hi = pair_stats(xs, ys, cost, inv6, cost_weight, xy_thresh, SAMPLES, ctx=ctx)
        print(f"d_eff  min/median/max = {lo:.2f} / {med:.2f} / {hi:.2f}")
    cl = merge_clusters(xs, ys, cost, inv6, cost_weight, xy_thresh, merge_radius, SAMPLES, ctx=ctx)
    origin = np.array(["chm"] * n_chm + ["density"] * (n - n_chm))
    out = {"id": torch.arange(n, dtype=torch.int64, device=xs.device), "cluster": cl, "ch_max": hs, "origin": origin, "x": xs, "y": ys}
    out = _device.out(out, is_t)
    if out_path is not None:
        write_seed_points(out_path, out, table="canonical_seeds")
        print(f"✓ canonical seeds: {n:,}  →  {out_path}")
    return out
