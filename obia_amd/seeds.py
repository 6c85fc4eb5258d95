"""The seed points of obia/utils/seeds.py on the GPU: ``make_chm_seeds``, ``make_density_seeds`` and ``make_canonical_seeds``.

Peaks (seeds.py:11-102) are a Gaussian smooth, a (2d+1)^2 maximum filter, a threshold and the row-major list of the surviving
pixels; the merge (seeds.py:139-165, 215-231) evaluates the cost-aware distance of every pair of seeds and takes the connected
components of ``D <= merge_radius`` -- what ``DBSCAN(min_samples=1, metric="precomputed")`` returns -- without ever storing the
matrix.  Both run in libobia_hip.so (seeds.hip).  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out; there is no CPU
path.  Seed tables are plain dicts of arrays (the reference's GeoDataFrame columns); a ``.gpkg`` path is written / read with
obia_amd.geopackage.

``make_canonical_seeds`` is the reference's function at its defaults and refuses the table options (``keep_all_stage1=False``,
``z_thresh``, ``dz_merge``, ``max_per_cluster``, ``nms_base`` / ``nms_scale``) and seeds without heights.  ``canonical_seeds`` is the
complete function: it builds every one of them on the device (seed_table.hip), stage by stage through
``sample_heights``, ``stage1_clusters``, ``reduce_stage1``, ``split_clusters_by_height``, ``trim_clusters`` and ``nms_per_crown``."""
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
    NotImplementedError here, as do seeds without heights: ``canonical_seeds`` is the function that takes them."""
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


# ------------------------------------------------------------------------------------------------------- the table options
# What make_canonical_seeds refuses, on the device (include/obia_seed_table.h).  A stage that selects or reorders rows
# returns an int64 selection into its input table; canonical_seeds applies it to every column with a gather.
_MAX_ROWS = 2 ** 31 - 1


def _columns(names, *cols):
    """Number of rows of 1-D columns of one length."""
    shapes = [_shape(c) for c in cols]
    if any(len(s) != 1 for s in shapes) or len(set(shapes)) != 1:
        raise ValueError(f"{names} must be 1-D and of one length, got {' and '.join(str(s) for s in shapes)}")
    if shapes[0][0] > _MAX_ROWS:
        raise ValueError(f"a seed table has fewer than 2^31 rows, got {shapes[0][0]}")
    return int(shapes[0][0])


def _rows(names, *cols):
    n = _columns(names, *cols)
    if n == 0:
        raise ValueError("no seeds")
    return n


def _host_nan_check(h):
    if not _device.is_torch(h) and np.isnan(np.asarray(h, dtype=np.float32)).any():
        raise ValueError("heights contain NaN")


def _heights(h, dev):
    """float32 heights on the device; NaN is refused (on the host for host input, so before the device is used)."""
    _host_nan_check(h)
    t = _as_dev(h, torch.float32, dev)
    if _device.is_torch(h) and bool(torch.isnan(t).any()):
        raise ValueError("heights contain NaN")
    return t


def _check_stage1(eps_scale, min_eps, max_eps, z_thresh, min_samples):
    """(eps_scale, min_eps, max_eps, z_thresh) as the float32 values the reference's arithmetic makes of them (a Python scalar next to
    a float32 height is weak under NumPy 2), z_thresh -1 when it is off, and min_samples."""
    es, lo, hi = np.float32(eps_scale), np.float32(min_eps), np.float32(max_eps)
    if not lo >= 0:
        raise ValueError(f"min_eps must not be negative, got {min_eps!r}")
    if not hi >= lo:
        raise ValueError(f"min_eps must not exceed max_eps, got min_eps {min_eps!r} and max_eps {max_eps!r}")
    if not np.isfinite(es):
        raise ValueError(f"eps_scale must be finite, got {eps_scale!r}")
    if z_thresh != z_thresh:
        raise ValueError("z_thresh is NaN")
    if int(min_samples) != min_samples or min_samples < 1:
        raise ValueError(f"min_samples must be an integer >= 1, got {min_samples!r}")
    return float(es), float(lo), float(hi), (float(np.float32(z_thresh)) if z_thresh >= 0 else -1.0), int(min_samples)


def _check_dz(dz_merge):
    if dz_merge != dz_merge:
        raise ValueError("dz_merge is NaN")
    if not dz_merge > 0:
        return 0.0
    d = float(np.float32(dz_merge))
    if d == 0.0:
        raise ValueError(f"dz_merge {dz_merge!r} is zero as a float32, the precision it is compared in")
    return d


def _check_trim(max_per_cluster):
    if int(max_per_cluster) != max_per_cluster:
        raise ValueError(f"max_per_cluster must be an integer, got {max_per_cluster!r}")
    return max(0, int(max_per_cluster))


def _check_nms(nms_base, nms_scale):
    base, scale = float(nms_base), float(nms_scale)
    if base != base or scale != scale or abs(base) == float("inf") or abs(scale) == float("inf"):
        raise ValueError(f"nms_base and nms_scale must be finite, got {nms_base!r} and {nms_scale!r}")
    return base, scale


def _sync(dev):
    torch.cuda.current_stream(dev).synchronize()     # what torch wrote is complete before the context's stream reads it


def _arange(n, like):
    return torch.arange(n, dtype=torch.int64, device=like.device)


def _grid(lib, c, dev, x, y, radius):
    """The seeds binned on a uniform grid whose cell side is not smaller than ``radius``: (order, sorted keys, ncx), memory O(n).

    The side is radius (1 + 2^-20), and at least 2^-29 of the largest coordinate: the cell indices then fit 31 bits, and two seeds
    the float64 predicate puts within ``radius`` of each other lie in neighbouring cells whatever the rounding of x / side (the
    quotients differ by at most radius (1 + 4u) / side + 2u max|x| / side < 1, u = 2^-53)."""
    if not bool(torch.isfinite(x).all() & torch.isfinite(y).all()):
        raise ValueError("seed coordinates must be finite")
    n = x.numel()
    biggest = float(torch.maximum(x.abs().max(), y.abs().max()))
    side = max(float(radius) * (1.0 + 2.0 ** -20), biggest * 2.0 ** -29)
    if not side > 0.0:
        side = 1.0
    cx = torch.empty(n, dtype=torch.int32, device=x.device)
    cy = torch.empty(n, dtype=torch.int32, device=x.device)
    _sync(dev)
    _lib.check(lib.obia_seedtab_cells_dev(c.handle, x.data_ptr(), y.data_ptr(), n, side, cx.data_ptr(), cy.data_ptr()))
    cx, cy = cx.to(torch.int64), cy.to(torch.int64)
    cx0, cy0 = cx.min(), cy.min()
    ncx = int(cx.max() - cx0) + 3
    key = (cy - cy0 + 1) * ncx + (cx - cx0 + 1)
    skey, order = torch.sort(key, stable=True)
    return order, skey.contiguous(), ncx


def sample_heights(xs, ys, chm, chm_affine=None, ctx=None):
    """_add_chm_height (seeds.py:105-112): the CHM at the pixel that contains each point -- floor of the inverse-affine column and
    row -- as ``(heights, keep)``: float32 heights of all n points (NaN where the point lies outside the raster or on a NaN pixel)
    and the int64 rows that survive, ascending.  ``chm_affine``: [a, b, d, e, xoff, yoff]; None = pixel coordinates."""
    _need_torch()
    n = _rows("xs and ys", xs, ys)
    if len(_shape(chm)) != 2 or 0 in _shape(chm):
        raise ValueError(f"chm must be a non-empty (H, W) raster, got shape {_shape(chm)}")
    inv6 = invert_affine(chm_affine if chm_affine is not None else (1, 0, 0, 1, 0, 0))
    is_t = _device.is_torch(xs)
    dev = _device.device_of(ctx, xs, ys, chm)
    x, y, r = _as_dev(xs, torch.float64, dev), _as_dev(ys, torch.float64, dev), _as_dev(chm, torch.float32, dev)
    H, W = r.shape
    lib, c = _device.begin(dev, ctx)
    h = torch.empty(n, dtype=torch.float32, device=x.device)
    valid = torch.empty(n, dtype=torch.uint8, device=x.device)
    _lib.check(lib.obia_seedtab_sample_dev(c.handle, x.data_ptr(), y.data_ptr(), n, r.data_ptr(), H, W, (ctypes.c_double * 6)(*inv6),
                                           h.data_ptr(), valid.data_ptr()))
    return _device.out((h, torch.nonzero(valid).reshape(-1)), is_t)


def stage1_clusters(xs, ys, heights, eps_scale=0.4, min_eps=2, max_eps=8, z_thresh=-1, min_samples=2, ctx=None):
    """The adaptive-radius pre-clustering (seeds.py:193-203): ``cluster1`` (int32, -1 = none) of every seed.

    In table order a seed without a pre-cluster draws the ball of eps = clip(eps_scale * h, min_eps, max_eps) (float32) around
    itself; when the ball has ``min_samples`` members and (``z_thresh`` >= 0) their heights spread no further than ``z_thresh``, ALL
    its members take the next id, those that had one included.  Computed from the closed form (include/obia_seed_table.h) in rounds;
    ``stage1_rounds`` reports how many the last call took."""
    _need_torch()
    n = _rows("xs, ys and heights", xs, ys, heights)
    es, lo, hi, zt, ms = _check_stage1(eps_scale, min_eps, max_eps, z_thresh, min_samples)
    _host_nan_check(heights)
    is_t = _device.is_torch(xs)
    dev = _device.device_of(ctx, xs, ys, heights)
    x, y, h = _as_dev(xs, torch.float64, dev), _as_dev(ys, torch.float64, dev), _heights(heights, dev)
    lib, c = _device.begin(dev, ctx)
    order, skey, ncx = _grid(lib, c, dev, x, y, hi)
    xs_s, ys_s, hs_s, orig = x[order].contiguous(), y[order].contiguous(), h[order].contiguous(), order.to(torch.int32).contiguous()
    fired_s = torch.empty(n, dtype=torch.uint8, device=x.device)
    owner_s = torch.empty(n, dtype=torch.int32, device=x.device)
    _sync(dev)
    _lib.check(lib.obia_seedtab_stage1_dev(c.handle, xs_s.data_ptr(), ys_s.data_ptr(), hs_s.data_ptr(), orig.data_ptr(), skey.data_ptr(), n,
                                           ncx, es, lo, hi, zt, ms, fired_s.data_ptr(), owner_s.data_ptr(), None))
    fired = torch.empty(n, dtype=torch.int64, device=x.device)
    owner = torch.empty(n, dtype=torch.int64, device=x.device)
    fired[order] = fired_s.to(torch.int64)
    owner[order] = owner_s.to(torch.int64)
    rank = torch.cumsum(fired, 0) - 1                                        # a fired seed's rank among the fired ones
    cl1 = torch.where(owner >= 0, rank[owner.clamp(min=0)], torch.full_like(owner, -1)).to(torch.int32)
    return _device.out(cl1, is_t)


def stage1_rounds(ctx=None, device=0):
    """(rounds, seeds) of this thread's last ``stage1_clusters``: a chain of seeds that each cover the next costs a round per link."""
    lib = _lib.load()
    c = ctx or _lib.default_context(device)
    w = (ctypes.c_int64 * 2)()
    _lib.check(lib.obia_seedtab_last_work(c.handle, w))
    return int(w[0]), int(w[1])


def _cluster_order(cl, h):
    """Rows by (cluster ascending, height descending, row ascending): two stable sorts."""
    i1 = torch.sort(h, descending=True, stable=True).indices
    return i1[torch.sort(cl[i1], stable=True).indices]


def _segments(lib, c, dev, cl, h, dz):
    """The table in cluster order and, per sorted row, its rank in the cluster, the cluster's size and the side of the median."""
    n = cl.numel()
    p = _cluster_order(cl, h)
    cs, hs = cl[p].contiguous(), h[p].contiguous()
    rank = torch.empty(n, dtype=torch.int32, device=cl.device)
    size = torch.empty(n, dtype=torch.int32, device=cl.device)
    part = torch.empty(n, dtype=torch.uint8, device=cl.device)
    _sync(dev)
    _lib.check(lib.obia_seedtab_segments_dev(c.handle, cs.data_ptr(), hs.data_ptr(), n, dz, rank.data_ptr(), size.data_ptr(), part.data_ptr()))
    return p, cs, rank.to(torch.int64), size.to(torch.int64), part.to(torch.int64)


def _cluster_args(cluster, heights, ctx):
    _need_torch()
    n = _rows("cluster and heights", cluster, heights)
    _host_nan_check(heights)
    is_t = _device.is_torch(cluster)
    dev = _device.device_of(ctx, cluster, heights)
    return n, is_t, dev, _as_dev(cluster, torch.int32, dev), _heights(heights, dev)


def reduce_stage1(cluster1, heights, stage1_top=1, ctx=None):
    """The reduction of ``keep_all_stage1=False`` (seeds.py:205-213) as an int64 selection: for every non-empty pre-cluster in
    ascending id its max(1, stage1_top) tallest rows, tallest first and ties to the earlier row, then the rows without a pre-cluster
    (-1) in table order."""
    top = max(1, int(stage1_top))
    n, is_t, dev, cl, h = _cluster_args(cluster1, heights, ctx)
    lib, c = _device.begin(dev, ctx)
    p, cs, rank, _, _ = _segments(lib, c, dev, cl, h, 0.0)
    sel = torch.cat([p[(cs >= 0) & (rank < top)], torch.nonzero(cl == -1).reshape(-1)])
    return _device.out(sel, is_t)


def split_clusters_by_height(cluster, heights, dz_merge, ctx=None):
    """The height split of ``dz_merge > 0`` (seeds.py:233-243) as ``(perm, cluster)``: a cluster whose heights spread further than
    float32(dz_merge) becomes its rows at or below its median and those above it; the parts are numbered consecutively in ascending
    id of the cluster, lower part first.  ``perm`` (int64) groups the rows by the new id, in table order inside a part; ``cluster``
    (int32) is the new column in that order.  dz_merge <= 0: the identity and the column as it is."""
    dz = _check_dz(dz_merge)
    n, is_t, dev, cl, h = _cluster_args(cluster, heights, ctx)
    if dz == 0.0:
        return _device.out((_arange(n, cl), cl), is_t)
    lib, c = _device.begin(dev, ctx)
    p, _, rank, _, part = _segments(lib, c, dev, cl, h, dz)
    nparts = torch.where(rank == 0, 1 + part, torch.zeros_like(part))         # at a cluster's first row, its tallest: 2 when it is above the median
    base = torch.cumsum(nparts, 0) - nparts
    new = torch.empty(n, dtype=torch.int64, device=cl.device)
    new[p] = base[_arange(n, cl) - rank] + part
    snew, perm = torch.sort(new, stable=True)
    return _device.out((perm, snew.to(torch.int32)), is_t)


def trim_clusters(cluster, heights, max_per_cluster, ctx=None):
    """The trim of ``max_per_cluster > 0`` (seeds.py:245-251) as an int64 selection: a cluster of more than m rows keeps its m
    tallest, tallest first and ties to the earlier row.  Row order is what pandas' groupby-apply leaves: the table's when no cluster is
    trimmed; otherwise grouped by cluster in ascending id, the untrimmed ones in table order."""
    m = _check_trim(max_per_cluster)
    n, is_t, dev, cl, h = _cluster_args(cluster, heights, ctx)
    if m == 0:
        return _device.out(_arange(n, cl), is_t)
    lib, c = _device.begin(dev, ctx)
    p, cs, rank, size, _ = _segments(lib, c, dev, cl, h, 0.0)
    trimmed = size > m
    if not bool(trimmed.any()):
        return _device.out(_arange(n, cl), is_t)
    keep = rank < m
    rows, cl_k = p[keep], cs[keep]
    second = torch.where(trimmed[keep], rank[keep], rows)
    i1 = torch.sort(second, stable=True).indices
    return _device.out(rows[i1[torch.sort(cl_k[i1], stable=True).indices]], is_t)


def nms_per_crown(xs, ys, heights, cluster, nms_base, nms_scale, ctx=None):
    """_nms_per_crown (seeds.py:115-136) as an int64 selection.  Per cluster in ascending id the rows are ordered by height
    descending (stable: ties to the earlier row; the reference's sort is not); row i of that order clears every other row of its
    cluster within r_i = max(nms_base, nms_scale * h_i) (float64, inclusive) and is set itself.  The reference's loop never skips a
    cleared row, so a LATER, LOWER row clears an earlier, taller one: a row survives when no row after it in that order has it within
    its radius.  The survivors, cluster by cluster in that order.  Both parameters <= 0: the identity."""
    base, scale = _check_nms(nms_base, nms_scale)
    _need_torch()
    n = _rows("xs, ys, heights and cluster", xs, ys, heights, cluster)
    _host_nan_check(heights)
    is_t = _device.is_torch(xs)
    dev = _device.device_of(ctx, xs, ys, heights, cluster)
    x, y, h = _as_dev(xs, torch.float64, dev), _as_dev(ys, torch.float64, dev), _heights(heights, dev)
    cl = _as_dev(cluster, torch.int32, dev)
    if not (base > 0 or scale > 0):
        return _device.out(_arange(n, cl), is_t)
    lib, c = _device.begin(dev, ctx)
    p = _cluster_order(cl, h)
    pos = torch.empty(n, dtype=torch.int64, device=cl.device)
    pos[p] = _arange(n, cl)
    # the largest radius: r is monotone in h, and the predicate squares it
    radius = max(abs(max(base, scale * float(h.max()))), abs(max(base, scale * float(h.min()))))
    order, skey, ncx = _grid(lib, c, dev, x, y, radius)
    xs_s, ys_s, hs_s = x[order].contiguous(), y[order].contiguous(), h[order].contiguous()
    cl_s, pos_s = cl[order].contiguous(), pos[order].to(torch.int32).contiguous()
    keep_s = torch.empty(n, dtype=torch.uint8, device=cl.device)
    _sync(dev)
    _lib.check(lib.obia_seedtab_nms_dev(c.handle, xs_s.data_ptr(), ys_s.data_ptr(), hs_s.data_ptr(), cl_s.data_ptr(), pos_s.data_ptr(),
                                        skey.data_ptr(), n, ncx, base, scale, keep_s.data_ptr()))
    keep = torch.empty(n, dtype=torch.bool, device=cl.device)
    keep[order] = keep_s != 0
    return _device.out(p[keep[p]], is_t)


def _any_seed_table(s, origin):
    """(x, y, heights or None) of a seed table; the height column may be missing."""
    if _is_path(s):
        s = read_seed_points(s)
    if not isinstance(s, dict) or "x" not in s or "y" not in s:
        raise ValueError(f"{origin} seeds must be a dict with x and y (what make_{'chm' if origin == 'chm' else 'density'}_seeds returns) or a "
                         ".gpkg path")
    h = s.get("ch_max" if origin == "chm" else "den_max", s.get("height"))
    cols = (s["x"], s["y"]) + (() if h is None else (h,))
    _columns(f"x, y and the height column of the {origin} seeds", *cols)
    return s["x"], s["y"], h


def canonical_seeds(chm_seeds, den_seeds, cost_surface, out_path=None, *, chm=None, chm_affine=None, eps_scale=0.4, min_eps=2, max_eps=8,
                    z_thresh=-1, min_samples=2, merge_radius=1.5, cost_weight=0.5, xy_thresh=0.8, dz_merge=0, keep_all_stage1=True,
                    stage1_top=1, max_per_cluster=0, nms_base=0, nms_scale=0, debug_dist=True, nodata_cost=1, cost_nodata=None,
                    cost_affine=None, ctx=None):
    """make_canonical_seeds (seeds.py:168-262) with every option, under the reference's keyword names and defaults.

    What ``make_canonical_seeds`` takes, and:
    chm, chm_affine : the canopy height model (array / CUDA tensor / raster path) and its [a, b, d, e, xoff, yoff]; a seed table
        without a ch_max / den_max / height column takes its heights from it (``sample_heights``) and loses the points outside the
        raster or on NaN.  A given height column that holds NaN raises ValueError.
    keep_all_stage1=False, stage1_top, eps_scale, min_eps, max_eps, z_thresh, min_samples : ``stage1_clusters`` and
        ``reduce_stage1``: only the tallest seeds of every pre-cluster go on to the merge.
    dz_merge > 0 : ``split_clusters_by_height``.   max_per_cluster > 0 : ``trim_clusters``.
    nms_base / nms_scale > 0 : ``nms_per_crown``.
    Returns the dict of ``make_canonical_seeds`` (id, cluster, ch_max, origin, x, y) -- at the defaults exactly what it returns --
    which ``grow_crowns`` takes as it is.  The stages run in the reference's order, each on the rows the one before it left."""
    tabs = [_any_seed_table(chm_seeds, "chm"), _any_seed_table(den_seeds, "density")]
    if chm is None and any(t[2] is None for t in tabs):
        raise ValueError("chm is needed: a seed table has no ch_max / den_max / height column to take its heights from")
    s1 = _check_stage1(eps_scale, min_eps, max_eps, z_thresh, min_samples)
    dz, m = _check_dz(dz_merge), _check_trim(max_per_cluster)
    base, scale = _check_nms(nms_base, nms_scale)
    for t in tabs:
        if t[2] is not None:
            _host_nan_check(t[2])
    inv6 = invert_affine(cost_affine if cost_affine is not None else (1, 0, 0, 1, 0, 0))
    _need_torch()
    cost_surface = _plane(cost_surface, None, "cost_surface")
    if 0 in _shape(cost_surface):
        raise ValueError("cost_surface is empty")
    if chm is not None:
        chm = _plane(chm, None, "chm")
    is_t = _device.is_torch(cost_surface)
    dev = _device.device_of(ctx, cost_surface, *[v for t in tabs for v in t if v is not None], chm)
    cols, n_chm = [], 0
    for k, (tx, ty, th) in enumerate(tabs):
        x, y = _as_dev(tx, torch.float64, dev), _as_dev(ty, torch.float64, dev)
        if th is not None:
            h = _heights(th, dev)
        elif x.numel():
            chm = _as_dev(chm, torch.float32, dev)
            h, keep = sample_heights(x, y, chm, chm_affine, ctx=ctx)
            x, y, h = x[keep], y[keep], h[keep]
        else:
            h = torch.empty(0, dtype=torch.float32, device=x.device)
        cols.append((x, y, h, torch.full((x.numel(),), k, dtype=torch.int64, device=x.device)))
    xs, ys, hs, org = [torch.cat([a[i] for a in cols]) for i in range(4)]
    n = int(xs.numel())
    if n == 0:
        raise SystemExit("No seeds after CHM sampling.")
    if not keep_all_stage1:
        cl1 = stage1_clusters(xs, ys, hs, s1[0], s1[1], s1[2], z_thresh, s1[4], ctx=ctx)
        sel = reduce_stage1(cl1, hs, stage1_top, ctx=ctx)
        xs, ys, hs, org = xs[sel], ys[sel], hs[sel], org[sel]
    cost = _as_dev(cost_surface, torch.float32, dev)
    if cost_nodata is not None:
        cost = torch.where(cost == float(np.float32(cost_nodata)), torch.full_like(cost, float(np.float32(nodata_cost))), cost)
    if debug_dist:
        lo, med, hi = pair_stats(xs, ys, cost, inv6, cost_weight, xy_thresh, SAMPLES, ctx=ctx)
        print(f"d_eff  min/median/max = {lo:.2f} / {med:.2f} / {hi:.2f}")
    cl = merge_clusters(xs, ys, cost, inv6, cost_weight, xy_thresh, merge_radius, SAMPLES, ctx=ctx)
    if dz > 0:
        sel, cl = split_clusters_by_height(cl, hs, dz, ctx=ctx)
        xs, ys, hs, org = xs[sel], ys[sel], hs[sel], org[sel]
    if m > 0:
        sel = trim_clusters(cl, hs, m, ctx=ctx)
        xs, ys, hs, org, cl = xs[sel], ys[sel], hs[sel], org[sel], cl[sel]
    if base > 0 or scale > 0:
        sel = nms_per_crown(xs, ys, hs, cl, base, scale, ctx=ctx)
        xs, ys, hs, org, cl = xs[sel], ys[sel], hs[sel], org[sel], cl[sel]
    n = int(xs.numel())
    origin = np.array([("chm", "density")[k] for k in org.cpu().tolist()])
    out = {"id": torch.arange(n, dtype=torch.int64, device=xs.device), "cluster": cl, "ch_max": hs, "origin": origin, "x": xs, "y": ys}
    out = _device.out(out, is_t)
    if out_path is not None:
        write_seed_points(out_path, out, table="canonical_seeds")
        print(f"✓ canonical seeds: {n:,}  →  {out_path}")
    return out
