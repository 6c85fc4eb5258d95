"""The cost surface of obia/utils/cost.py on the GPU: ``normalise``, ``chm_gradient``, ``ndvi``, ``texture_entropy`` and
``make_cost_surface``, with the reference's dtypes and values under NumPy >= 2 promotion (every normalised layer is
float64, the surface float32).  The layers run in libobia_hip.so (cost.hip); the host only interpolates the percentiles
from the order statistics the device selects (np.nanpercentile's linear method, restated operation for operation) and
builds the entropy term table with libm ``log``.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out.

``make_cost_surface`` takes the label raster; ``rasterise_slic_gpkg`` (cost.py:51-86) makes that raster from a stored
``segments.gpkg`` on the GPU (obia_amd.polygons.rasterize).  The nodata mask of the reference's masked WorldView-3 read is
not built ("Cost surface")."""
import ctypes
import math
import os
import warnings

import numpy as np

from . import _device, _lib, _percentile

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

N_BANDS = 8                        # C, B, G, Y, R, RE, N1, N2 (the reference unpacks exactly these)
BAND_C, BAND_R, BAND_N1 = 0, 4, 6
_Q = np.true_divide((2, 98), 100.0)
_LN2 = 0.6931471805599453
_TCOLS = 32


def _need_torch():
    _device.need_torch("obia_amd.cost")


def _is_path(x):
    return isinstance(x, (str, bytes, os.PathLike))


def _shape(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def _as_dev(x, dtype, dev):
    """Contiguous, 16-byte aligned device tensor of ``dtype`` (NumPy's astype for other dtypes)."""
    return _device.as_dev(x, dtype, dev, align16=True)


def _lerp(n, a, b, dtype):
    """np.nanpercentile(x, (2, 98)) from the four order statistics (obia_amd._percentile.lerp at q = 0.02, 0.98)."""
    return _percentile.lerp(n, a, b, dtype, _Q)


def _select(lib, c, plane):
    """(lo, hi) = np.nanpercentile(plane, (2, 98)) of a float32 / float64 device plane, and the number of valid values."""
    return _percentile.select(lib, c, plane, _Q)


def _edge_lohi(lib, c, lab, H, W):
    """np.nanpercentile of the 0/1 float32 edge image of a label raster: its order statistics follow from the edge count."""
    n_edge = ctypes.c_int64(0)
    _lib.check(lib.obia_cost_edge_count_dev(c.handle, lab.data_ptr(), H, W, ctypes.byref(n_edge)))
    n, z = H * W, H * W - int(n_edge.value)
    v = (n - 1) * _Q
    ia = np.where(v >= n - 1, n - 1, np.floor(v)).astype(np.int64)
    ib = np.where(v >= n - 1, n - 1, ia + 1)
    lohi = _lerp(n, (ia >= z).astype(np.float32), (ib >= z).astype(np.float32), np.float32)
    return float(lohi[0]), float(lohi[1])


_TABLE = {}


def entropy_table():
    """T[pop][c] = (c / pop) * log(c / pop) / ln 2 for pop, c in 1..29 (libm log, float64), column 0 = 0: the terms skimage's
    rank entropy subtracts, one per grey level present, in ascending grey-level order."""
    t = np.zeros((30, _TCOLS), np.float64)
    for pop in range(1, 30):
        for cnt in range(1, pop + 1):
            p = cnt / pop
            t[pop, cnt] = p * math.log(p) / _LN2
    return t


def _table_dev(dev):
    t = _TABLE.get(dev)
    if t is None:
        t = _TABLE[dev] = torch.as_tensor(entropy_table(), device=f"cuda:{dev}")
    return t


def _plane(x, dev, name):
    if _is_path(x):
        x = _read_band(x)
    if len(_shape(x)) != 2:
        raise ValueError(f"{name} must be (H, W), got shape {_shape(x)}")
    return x


def _float_plane(x, dev):
    """float32 / float64 planes are kept as they are; any other dtype is cast to float32."""
    if _device.is_torch(x):
        dt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    else:
        dt = torch.float64 if np.asarray(x).dtype == np.float64 else torch.float32
    return _as_dev(x, dt, dev)


def _normalise_dev(lib, c, plane):
    lo, hi, n = _select(lib, c, plane)
    out = torch.empty(plane.shape, dtype=torch.float64, device=plane.device)
    _lib.check(lib.obia_cost_normalise_dev(c.handle, plane.data_ptr(), int(plane.dtype == torch.float64), plane.numel(), lo, hi,
                                           out.data_ptr()))
    if n == 0 and plane.dtype == torch.float32:
        out = out.to(torch.float32)      # all NaN: the percentiles are float32 NaN, so nothing promotes (zeros either way)
    return out


def normalise(arr, ctx=None):
    """np.nan_to_num((np.clip(arr, lo, hi) - lo) / (hi - lo)) with lo, hi = np.nanpercentile(arr, (2, 98)): float64 out for
    a float32 or float64 plane (other dtypes are taken as float32).  Constant or all-NaN input gives zeros."""
    _need_torch()
    is_t = _device.is_torch(arr)
    dev = _device.device_of(ctx, arr)
    x = _float_plane(arr, dev)
    if x.numel() == 0:
        raise ValueError("normalise of an empty array")
    lib, c = _device.begin(dev, ctx)
    out = _normalise_dev(lib, c, x)
    _device.end(lib, c)
    return _device.out(out.reshape(_shape(arr)), is_t)


def _sobel_dev(lib, c, chm):
    H, W = chm.shape
    g = torch.empty((H, W), dtype=torch.float32, device=chm.device)
    _lib.check(lib.obia_cost_sobel_f32_dev(c.handle, chm.data_ptr(), H, W, g.data_ptr()))
    return g


def chm_gradient(chm, ctx=None, _raw=False):
    """normalise(np.hypot(sobel(chm, axis=1), sobel(chm, axis=0))), mode "nearest": float64 (H, W).  NaN pixels of the CHM
    spoil their 3 x 3 neighbourhood and end as 0.  ``_raw=True`` returns the float32 hypot plane before normalise."""
    _need_torch()
    chm = _plane(chm, None, "chm")
    is_t = _device.is_torch(chm)
    if 0 in _shape(chm):
        raise ValueError("chm is empty")
    dev = _device.device_of(ctx, chm)
    x = _as_dev(chm, torch.float32, dev)
    lib, c = _device.begin(dev, ctx)
    g = _sobel_dev(lib, c, x)
    out = g if _raw else _normalise_dev(lib, c, g)
    _device.end(lib, c)
    return _device.out(out, is_t)


def ndvi(red, nir, ctx=None):
    """np.clip((nir - red) / (nir + red + 1e-9), -1, 1) in float32."""
    _need_torch()
    if _shape(red) != _shape(nir):
        raise ValueError(f"red and nir differ in shape: {_shape(red)} vs {_shape(nir)}")
    is_t = _device.is_torch(red) or _device.is_torch(nir)
    dev = _device.device_of(ctx, red, nir)
    r, n = _as_dev(red, torch.float32, dev), _as_dev(nir, torch.float32, dev)
    out = torch.empty(r.shape, dtype=torch.float32, device=r.device)
    lib, c = _device.begin(dev, ctx)
    if r.numel():
        _lib.check(lib.obia_cost_ndvi_f32_dev(c.handle, r.data_ptr(), n.data_ptr(), r.numel(), out.data_ptr()))
    _device.end(lib, c)
    return _device.out(out, is_t)


def _entropy_dev(lib, c, pan, lo, hi):
    H, W = pan.shape
    e = torch.empty((H, W), dtype=torch.float64, device=pan.device)
    _lib.check(lib.obia_cost_entropy_f32_dev(c.handle, pan.data_ptr(), H, W, lo, hi, _table_dev(pan.device.index or 0).data_ptr(),
                                             e.data_ptr()))
    return e


def texture_entropy(pan, ctx=None, _raw=False):
    """normalise(entropy((normalise(pan) * 255).astype(uint8), disk(3))): skimage's rank entropy (bits) over the 29-pixel
    disk, taps outside the raster not counted; float64 (H, W).  ``_raw=True`` returns the entropy before the last
    normalise."""
    _need_torch()
    pan = _plane(pan, None, "pan")
    is_t = _device.is_torch(pan)
    if 0 in _shape(pan):
        raise ValueError("pan is empty")
    dev = _device.device_of(ctx, pan)
    x = _as_dev(pan, torch.float32, dev)
    lib, c = _device.begin(dev, ctx)
    lo, hi, _ = _select(lib, c, x)
    e = _entropy_dev(lib, c, x, lo, hi)
    out = e if _raw else _normalise_dev(lib, c, e)
    _device.end(lib, c)
    return _device.out(out, is_t)


# ------------------------------------------------------------------------------------------- segments.gpkg -> label raster
def _profile_transform(t):
    """rasterio's ``profile["transform"]`` -- six numbers (a, b, xoff, d, e, yoff) or an object with attributes a..f -- as this
    package's [a, b, d, e, xoff, yoff]."""
    if all(hasattr(t, k) for k in "abcdef"):
        t = (t.a, t.b, t.c, t.d, t.e, t.f)
    try:
        a, b, xoff, d, e, yoff = [float(v) for v in t][:6]
    except Exception:
        raise ValueError("tgt_profile['transform'] must be six numbers (a, b, xoff, d, e, yoff) or an Affine") from None
    return [a, b, d, e, xoff, yoff]


def _wkb_is_empty(wkb):
    import struct
    if wkb is None or len(wkb) < 9:
        return True
    kind, n = struct.unpack_from("<II", wkb, 1)
    if kind == 3:
        return n == 0 or struct.unpack_from("<I", wkb, 9)[0] == 0
    return n == 0


def rasterise_slic_gpkg(gpkg_path, tgt_profile, ctx=None, as_tensor=False):
    """Rasterise the polygons of a ``segments.gpkg`` (column ``segment_id``) onto the target grid: obia/utils/cost.py:51-86
    without geopandas / rasterio -- the file is read with obia_amd.geopackage, the polygons are burned on the GPU
    (obia_amd.polygons.rasterize: fill 0, pixel centres, later rows over earlier ones).

    ``tgt_profile``: mapping with ``height``, ``width`` and ``transform`` (rasterio order (a, b, xoff, d, e, yoff), or an object
    with attributes a..f); optional ``bounds`` (west, south, east, north): only shapes whose envelope meets them are burned (a
    superset of the reference's bbox read -- shapes outside burn nothing); optional ``crs``: must name the layer's EPSG code,
    reprojection is not built (NotImplementedError).  Rows whose ``segment_id`` ``int()`` cannot convert and empty geometries
    are skipped.  Returns the (H, W) int32 label raster ``make_cost_surface(slic=...)`` takes (a CUDA tensor with
    ``as_tensor=True``)."""
    from .geopackage import read_geopackage, _wkb_envelope
    from .segmentation import _epsg_of
    try:
        H, W = int(tgt_profile["height"]), int(tgt_profile["width"])
        transform = tgt_profile["transform"]
    except (KeyError, TypeError):
        raise ValueError("tgt_profile must be a mapping with height, width and transform") from None
    if H <= 0 or W <= 0:
        raise ValueError(f"tgt_profile height and width must be positive, got {H} x {W}")
    aff = _profile_transform(transform)
    bounds = tgt_profile.get("bounds")
    if bounds is not None:
        try:
            west, south, east, north = [float(v) for v in bounds]
        except Exception:
            raise ValueError("tgt_profile['bounds'] must be (west, south, east, north)") from None
    wkbs, cols, srs_id = read_geopackage(os.fspath(gpkg_path), table="segments")
    if "segment_id" not in cols:
        raise ValueError("the segments table has no 'segment_id' column")
    rows = list(zip(wkbs, cols["segment_id"]))
    if bounds is not None:
        kept = []
        for w, seg in rows:
            if _wkb_is_empty(w):
                continue
            minx, maxx, miny, maxy = _wkb_envelope(w)
            if maxx >= west and minx <= east and maxy >= south and miny <= north:
                kept.append((w, seg))
        rows = kept
    if not rows:
        raise SystemExit("SLIC GPKG has no polygons over this tile.")
    crs = tgt_profile.get("crs")
    if crs is not None:
        want = _epsg_of(getattr(crs, "to_epsg", lambda: crs)())
        if want is None or want != srs_id:
            raise NotImplementedError(f"the layer's srs_id is {srs_id} and the target crs is {crs!r}: reprojection is not built")
    shapes, ids = [], []
    for w, seg in rows:
        try:
            seg_id = int(seg)
        except Exception:
            continue
        if not _wkb_is_empty(w):
            shapes.append(w)
            ids.append(seg_id)
    if not shapes:
        raise SystemExit("No valid SLIC polygons with 'segment_id' found.")
    from .polygons import rasterize
    return rasterize(shapes, (H, W), aff, values=np.asarray(ids, np.int64), fill=0, ctx=ctx, as_tensor=as_tensor)


# ------------------------------------------------------------------------------------------------------ the cost surface
def _read_band(path, idx=1):
    """read_band (cost.py:14-18) through GDAL: band ``idx`` as float32, nodata -> NaN."""
    try:
        from osgeo import gdal
    except Exception as e:  # pragma: no cover
        raise ImportError("reading a raster path needs GDAL (osgeo); pass the (H, W) array instead") from e
    ds = gdal.Open(os.fspath(path))
    if not ds:
        raise ValueError(f"Unable to open {path}")
    band = ds.GetRasterBand(idx)
    arr = band.ReadAsArray().astype(np.float32)
    nd = band.GetNoDataValue()
    if nd is not None:
        arr[arr == np.float32(nd)] = np.nan
    return arr


def _write_cost(path, cost, like):  # pragma: no cover - needs GDAL
    try:
        from osgeo import gdal
    except Exception as e:
        raise ImportError("writing the cost surface needs GDAL (osgeo); pass out=None to get the array") from e
    os.makedirs(os.path.dirname(os.path.abspath(os.fspath(path))), exist_ok=True)
    H, W = cost.shape
    ds = gdal.GetDriverByName("GTiff").Create(os.fspath(path), W, H, 1, gdal.GDT_Float32, options=["COMPRESS=DEFLATE"])
    if like is not None:
        src = gdal.Open(os.fspath(like))
        ds.SetGeoTransform(src.GetGeoTransform())
        ds.SetProjection(src.GetProjection())
    band = ds.GetRasterBand(1)
    band.SetNoDataValue(-9999.0)
    band.WriteArray(cost)
    ds.FlushCache()


def _weights(weights, have_slic):
    w_grad, w_gap, w_tex, w_slic = weights
    if abs(sum(weights) - 1) > 1e-6:
        raise SystemExit("Weights must sum to 1.")
    if not have_slic:
        s = w_grad + w_gap + w_tex
        w_grad, w_gap, w_tex, w_slic = (w_grad / s, w_gap / s, w_tex / s, 0.0)
    return [float(w_grad), float(w_gap), float(w_tex), float(w_slic)]


def make_cost_surface(wv3, chm, out=None, slic=None, weights=(0.5, 0.25, 0.25, 0), ctx=None, _layers=None):
    """Cost surface of obia/utils/cost.py:89-140, float32 (H, W) in [0, 1]:
    clip(w_grad * chm_gradient + w_gap * normalise(1 - ndvi(R, N1)) + w_tex * texture_entropy(C) + w_slic * edge, 0, 1).

    wv3  : (H, W, 8) array or CUDA tensor (C, B, G, Y, R, RE, N1, N2), an object with ``img_data``, or a path (GDAL).
    chm  : (H, W) canopy height model, NaN = nodata; array, tensor or path.
    slic : (H, W) label raster (the rasterised ``segments.gpkg``), a path to one, or None: then the first three weights are
           renormalised, the edge term is 0 and a warning says so.  A .gpkg path raises NotImplementedError: to use a
           GeoPackage, pass ``slic=rasterise_slic_gpkg(path, profile)``.
    out  : GeoTIFF path (GDAL) or None.  The surface is returned either way (a CUDA tensor when wv3 is one).
    ``_layers``: a dict that receives the (lo, hi) each layer was stretched with (test hook).
    """
    _need_torch()
    if _is_path(slic) and os.fsdecode(slic).lower().endswith(".gpkg"):
        raise NotImplementedError("slic as a .gpkg is not supported: pass the (H, W) label raster of segment_id "
                                  "(the raster the polygons were made from) instead")
    w = _weights(weights, slic is not None)
    like = wv3 if _is_path(wv3) else None
    if _is_path(wv3):
        from .tiling import _open_raster
        wv3 = _open_raster(os.fspath(wv3))[0]
    elif hasattr(wv3, "img_data"):
        wv3 = wv3.img_data
    chm = _plane(chm, None, "chm")
    if slic is not None:
        slic = _plane(slic, None, "slic")
    shp = _shape(wv3)
    if len(shp) != 3 or shp[2] != N_BANDS:
        raise ValueError(f"wv3 must be (H, W, {N_BANDS}) (C, B, G, Y, R, RE, N1, N2), got shape {shp}")
    H, W = shp[0], shp[1]
    if H == 0 or W == 0:
        raise ValueError("wv3 is empty")
    if _shape(chm) != (H, W):
        raise ValueError(f"chm shape {_shape(chm)} does not match the raster's {(H, W)}")
    if slic is not None and _shape(slic) != (H, W):
        raise ValueError(f"slic shape {_shape(slic)} does not match the raster's {(H, W)}")
    if slic is None:
        warnings.warn("No SLIC provided – cost built from 3 terms only.")
    is_t = _device.is_torch(wv3)
    dev = _device.device_of(ctx, wv3, chm, slic)

    img = _as_dev(wv3, torch.float32, dev)
    chm_d = _as_dev(chm, torch.float32, dev)
    lab = _as_dev(slic, torch.int32, dev) if slic is not None else None
    lib, c = _device.begin(dev, ctx)
    pan = torch.empty((H, W), dtype=torch.float32, device=img.device)
    gap = torch.empty((H, W), dtype=torch.float32, device=img.device)
    _lib.check(lib.obia_cost_bands_f32_dev(c.handle, img.data_ptr(), H * W, pan.data_ptr(), gap.data_ptr()))
    grad = _sobel_dev(lib, c, chm_d)
    lo_c, hi_c, _ = _select(lib, c, pan)
    tex = _entropy_dev(lib, c, pan, lo_c, hi_c)
    del pan
    lohi = [_select(lib, c, grad)[:2], _select(lib, c, gap)[:2], _select(lib, c, tex)[:2]]
    lohi.append(_edge_lohi(lib, c, lab, H, W) if lab is not None else (0.0, 0.0))
    cost = torch.empty((H, W), dtype=torch.float32, device=img.device)
    d4 = ctypes.c_double * 4
    _lib.check(lib.obia_cost_combine_dev(c.handle, grad.data_ptr(), gap.data_ptr(), tex.data_ptr(),
                                         lab.data_ptr() if lab is not None else None, H, W, d4(*[p[0] for p in lohi]),
                                         d4(*[p[1] for p in lohi]), d4(*w), cost.data_ptr()))
    _device.end(lib, c)
    if _layers is not None:
        _layers.update(pan=(lo_c, hi_c), grad=lohi[0], gap=lohi[1], tex=lohi[2], edge=lohi[3] if lab is not None else None,
                       weights=tuple(w))
    if out is not None:
        _write_cost(out, cost.cpu().numpy(), like)
    return _device.out(cost, is_t)
