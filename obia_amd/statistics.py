"""Host-side mirror of the reference's per-segment statistics interface.

Mirrors ``obia.segmentation.segment_statistics.create_objects`` / ``calculate_spectral_stats`` /
``_create_empty_stats_columns`` (segment_statistics.py:392-511, :113-176, :12-110) for the statistics on
the hot path: mean, variance (ddof 0), min, max per band per segment, batched over all segments in one
GPU pass (libobia_hip.so: obia_zonal_stats_f32), plus skewness / kurtosis from a second pass
(obia_zonal_moments_f32).
"""
import ctypes

import numpy as np

from . import _device, _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def _band_list(bands, C):
    bl = list(range(C)) if bands is None else [int(b) for b in bands]
    for b in bl:
        if b < 0 or b >= C:
            raise IndexError(f"Band index {b} out of range. Available bands indices: 0 to {C - 1}.")
    return bl


def _n_labels(n_labels, lab, start_label):
    """``n_labels`` as given, or what the largest label of ``lab`` implies; never negative."""
    if n_labels is None:
        empty = isinstance(lab, np.ndarray) and lab.size == 0      # (an empty tensor is refused by its own max())
        n_labels = 0 if empty else int(lab.max()) - start_label + 1
    return max(int(n_labels), 0)


def _buffer(like, shape, dtype, fill=None):
    """An output beside ``like``.  A tensor is left unwritten unless ``fill`` is given (the device kernels write every entry);
    an array for the host entry points starts at ``fill``, or at 0 / NaN."""
    if _device.is_torch(like):
        dt = getattr(torch, np.dtype(dtype).name)
        return torch.empty(shape, dtype=dt, device=like.device) if fill is None else torch.full(shape, fill, dtype=dt, device=like.device)
    return np.full(shape, fill if fill is not None else (0 if np.dtype(dtype).kind == "i" else np.nan), dtype)


def zonal_stats(raw, labels, bands=None, start_label=1, n_labels=None, ctx=None, moments=False):
    """Per-label statistics of ``raw`` (H,W,C) under the label raster ``labels`` (H,W).

    Returns a dict: ``count`` (N,), ``mean``/``variance`` (N,B) float64, ``min``/``max`` (N,B) float32, with
    N = n_labels (default: max label - start_label + 1) and B = len(bands).  Labels outside
    [start_label, start_label+N) -- e.g. the -1 / 0 of masked pixels -- are ignored; NaN pixels are dropped
    per band; empty segments give NaN (segment_statistics.py:145-162).  NumPy in -> NumPy out (the host entry points:
    torch is not needed); CUDA tensors in -> CUDA tensors out.

    ``moments=True`` adds ``skewness`` and ``kurtosis`` (N,B) float64: scipy.stats.skew / kurtosis with their defaults
    (segment_statistics.py:173-175), computed by a second pass with the per-label means as pivots
    (obia_zonal_moments_f32_dev); ``variance`` is then that pass's central m2.  The first pass alone sums about a pivot
    pixel of each segment (zonal.hip), so both stay accurate on bright, nearly flat segments.
    """
    is_t = _device.is_torch(raw)
    dev = _device.device_of(ctx, raw, labels)
    if is_t:
        r, lab = _device.as_dev(raw, torch.float32, dev), _device.as_dev(labels, torch.int32, dev)
        ptr = torch.Tensor.data_ptr
    else:
        r, lab = np.ascontiguousarray(raw, dtype=np.float32), np.ascontiguousarray(labels, dtype=np.int32)
        ptr = _lib.np_ptr
    if r.ndim != 3:
        raise ValueError("raw must be (H,W,C)")
    H, W, C = r.shape
    if tuple(lab.shape) != (H, W):
        raise ValueError("labels must have the raster's (H,W) shape")
    n_labels = _n_labels(n_labels, lab, start_label)
    bl = _band_list(bands, C)
    B = len(bl)
    barr = np.ascontiguousarray(bl, np.int32)
    cnt = _buffer(r, (n_labels,), np.int64)
    mean, var = _buffer(r, (n_labels, B), np.float64), _buffer(r, (n_labels, B), np.float64)
    mn, mx = _buffer(r, (n_labels, B), np.float32), _buffer(r, (n_labels, B), np.float32)
    if moments:
        # filled on torch's stream before `begin` waits for it: a fill queued between the two calls could land on the second call's result
        skew, kurt = _buffer(r, (n_labels, B), np.float64, float("nan")), _buffer(r, (n_labels, B), np.float64, float("nan"))
    lib, c = _device.begin(dev, ctx, host=not is_t)
    stats = lib.obia_zonal_stats_f32_dev if is_t else lib.obia_zonal_stats_f32
    _lib.check(stats(c.handle, ptr(r), ptr(lab), H, W, C, _lib.np_ptr(barr), B, n_labels, int(start_label), ptr(cnt), ptr(mean),
                     ptr(var), ptr(mn), ptr(mx)))
    out = {"count": cnt, "mean": mean, "variance": var, "min": mn, "max": mx, "bands": bl}
    if moments:
        pivots = (ptr(mean),) if is_t else ()              # (the host entry point keeps the means of its own first pass)
        second = lib.obia_zonal_moments_f32_dev if is_t else lib.obia_zonal_moments_f32
        _lib.check(second(c.handle, ptr(r), ptr(lab), H, W, C, _lib.np_ptr(barr), B, n_labels, int(start_label), *pivots, ptr(skew),
                          ptr(kurt), ptr(var)))
        out["skewness"], out["kurtosis"] = skew, kurt
    return out


TEXTURE_PROPS = ("contrast", "dissimilarity", "homogeneity", "ASM", "energy", "correlation")


def texture_stats(raw, labels, bands=None, start_label=1, n_labels=None, ctx=None):
    """GLCM texture statistics per (label, band): dict prop -> (N, B) float64 for contrast, dissimilarity, homogeneity,
    ASM, energy, correlation (calculate_textural_stats, segment_statistics.py:179-298, on the band plane -- see
    oracle/glcm.py for the one place where this departs from the reference's indexing).  NumPy in -> NumPy out, CUDA
    tensors in -> CUDA tensors out (libobia_hip.so: obia_texture_stats_f32_dev)."""
    _device.need_torch("obia_amd.statistics.texture_stats")
    is_t = _device.is_torch(raw)
    dev = _device.device_of(ctx, raw, labels)
    r = _device.as_dev(raw, torch.float32, dev)
    if r.dim() != 3:
        raise ValueError("raw must be (H,W,C)")
    H, W, C = r.shape
    lab = _device.as_dev(labels, torch.int32, dev)
    if tuple(lab.shape) != (H, W):
        raise ValueError("labels must have the raster's (H,W) shape")
    n_labels = _n_labels(n_labels, lab, start_label)
    bl = _band_list(bands, C)
    B = len(bl)
    barr = np.ascontiguousarray(bl, np.int32)
    out = torch.full((6, n_labels, B), float("nan"), dtype=torch.float64, device=r.device)
    lib, c = _device.begin(dev, ctx)
    if n_labels > 0 and B > 0:
        _lib.check(lib.obia_texture_stats_f32_dev(c.handle, r.data_ptr(), lab.data_ptr(), H, W, C, _lib.np_ptr(barr), B,
                                                  n_labels, int(start_label), out.data_ptr()))
    res = {p: _device.out(out[i], is_t) for i, p in enumerate(TEXTURE_PROPS)}
    res["bands"] = bl
    return res


POINTCLOUD_STATS = ("pai", "fhd", "ch", "mean_intensity", "variance_intensity")


def stats_columns(spectral_bands, textural_bands=(), calc_mean=True, calc_variance=True, calc_min=True, calc_max=True,
                  calc_skewness=True, calc_kurtosis=True, calc_contrast=True, calc_dissimilarity=True,
                  calc_homogeneity=True, calc_ASM=True, calc_energy=True, calc_correlation=True,
                  calc_pai=False, calc_fhd=False, calc_ch=False, calc_mean_intensity=False, calc_variance_intensity=False,
                  geometry=False):
    """Column names and order of the objects table: segment_id, then per spectral band
    mean/variance/min/max/skewness/kurtosis, then per textural band the six GLCM properties, then the point-cloud
    statistics whose flags are set, then ``geometry`` (obia _create_empty_stats_columns, segment_statistics.py:12-110).
    create_objects passes the reference's defaults (all five point-cloud flags True, geometry last)."""
    cols = ["segment_id"]
    spec = [("mean", calc_mean), ("variance", calc_variance), ("min", calc_min), ("max", calc_max),
            ("skewness", calc_skewness), ("kurtosis", calc_kurtosis)]
    for b in spectral_bands:
        cols += [f"b{b}_{name}" for name, on in spec if on]
    tex = [("contrast", calc_contrast), ("dissimilarity", calc_dissimilarity), ("homogeneity", calc_homogeneity),
           ("ASM", calc_ASM), ("energy", calc_energy), ("correlation", calc_correlation)]
    for b in textural_bands:
        cols += [f"b{b}_{name}" for name, on in tex if on]
    cols += [name for name, on in zip(POINTCLOUD_STATS, (calc_pai, calc_fhd, calc_ch, calc_mean_intensity,
                                                         calc_variance_intensity)) if on]
    if geometry:
        cols.append("geometry")
    return cols


def _labels_of(segments):
    """The label raster behind ``segments``: the raster itself, or the table create_segments(as_table=True) returned
    (its ``attrs["labels"]``)."""
    if hasattr(segments, "attrs") and "labels" in getattr(segments, "attrs", {}):
        return segments.attrs["labels"], segments
    return segments, None


def create_objects(segments, image, ept=None, ept_srs=None, spectral_bands=None, textural_bands=None, voxel_resolution=None,
                   calculate_spectral=True, calculate_textural=True, calculate_structural=False, calculate_radiometric=False,
                   calc_mean=True, calc_variance=True, calc_min=True, calc_max=True, calc_skewness=True, calc_kurtosis=True,
                   calc_contrast=True, calc_dissimilarity=True, calc_homogeneity=True, calc_ASM=True, calc_energy=True,
                   calc_correlation=True, calc_pai=True, calc_fhd=True, calc_ch=True, calc_mean_intensity=True,
                   calc_variance_intensity=True, *, start_label=1, pointcloud=None, geometry=True, ctx=None):
    """Mirror of obia create_objects (segment_statistics.py:392-511): same positional order, same defaults, same column
    set and order -- ``calculate_textural`` defaults to True, the five point-cloud columns are present and NaN (their flags
    default to True while the point-cloud workflow itself raises, :435-439), ``geometry`` comes last.

    ``pointcloud``: what :func:`obia_amd.pointcloud.as_points` accepts (a structured array or a dict with ``X``, ``Y``,
    ``HeightAboveGround`` and optionally ``Intensity``).  With it ``calculate_structural=True`` fills ``pai``, ``fhd`` and ``ch``
    and ``calculate_radiometric=True`` fills ``mean_intensity`` and ``variance_intensity``, each where its ``calc_*`` flag is
    set; it needs ``voxel_resolution`` (dx, dy, dz) -- only dz is used: the segment footprint is the voxel column -- and the
    image's ``affine_transformation``.  Without it both flags raise as the reference does, and so does ``ept``.

    ``segments``: the label raster from create_segments (one 4-connected component per label, so "pixels inside polygon p"
    are "pixels carrying label p") or the table create_segments(as_table=True) returned.  ``image``: object
    with ``img_data`` (and optionally ``affine_transformation`` / ``crs``) or the raw (H,W,C) array.  Labels below
    ``start_label`` (the -1 / 0 of masked pixels) get no row; ``segment_id`` = 1..N in ascending label order
    (segment_boundaries.py:76).
    ``geometry``: True -> one polygon per segment from the GPU polygoniser (WKB bytes; shapely geometries in a
    GeoDataFrame when geopandas is installed); False -> the column holds None (skips the polygon pass).
    Spectral statistics are always computed, like the reference's loop (:487-491 does not test ``calculate_spectral``).
    """
    import pandas as pd
    if not (calculate_spectral or calculate_textural or calculate_structural or calculate_radiometric):
        raise ValueError("At least one of 'calculate_spectral', 'calculate_textural', 'calculate_structural', or "
                         "'calculate_radiometric' must be True.")
    if ept is not None or ((calculate_structural or calculate_radiometric) and pointcloud is None):
        raise NotImplementedError("Point-cloud workflows are temporarily disabled. "
                                  "Use spectral/textural statistics only for now.")
    if pointcloud is not None:
        try:
            voxel = [float(v) for v in voxel_resolution]
        except TypeError:
            voxel = []
        if len(voxel) != 3 or not all(np.isfinite(v) and v > 0.0 for v in voxel):
            raise ValueError(f"pointcloud needs voxel_resolution = (dx, dy, dz), three positive numbers, got {voxel_resolution!r}")
        if getattr(image, "affine_transformation", None) is None:
            raise ValueError("pointcloud needs the image's affine_transformation to place the points on the raster")
    labels, seg_table = _labels_of(segments)
    img_data = image.img_data if hasattr(image, "img_data") else image
    C = img_data.shape[2]
    if spectral_bands is None:
        spectral_bands = list(range(C))
    if textural_bands is None:
        textural_bands = list(range(C))
    spectral_bands, textural_bands = list(spectral_bands), list(textural_bands)
    st = zonal_stats(img_data, labels, bands=spectral_bands, start_label=start_label, ctx=ctx,
                     moments=bool(calc_skewness or calc_kurtosis))
    st = _device.out(st, False)
    n = st["count"].shape[0]
    present = st["count"] > 0                      # ids of the table: the labels that exist (np.unique order)
    cols = stats_columns(spectral_bands, textural_bands, calc_mean, calc_variance, calc_min, calc_max, calc_skewness,
                         calc_kurtosis, calc_contrast, calc_dissimilarity, calc_homogeneity, calc_ASM, calc_energy,
                         calc_correlation, calc_pai, calc_fhd, calc_ch, calc_mean_intensity, calc_variance_intensity,
                         geometry=True)
    n_rows = int(present.sum())
    data = {"segment_id": np.arange(1, n_rows + 1)}
    for j, b in enumerate(spectral_bands):
        for name, on in (("mean", calc_mean), ("variance", calc_variance), ("min", calc_min), ("max", calc_max),
                         ("skewness", calc_skewness), ("kurtosis", calc_kurtosis)):
            if on:
                data[f"b{b}_{name}"] = st[name][present, j]
    tex_names = [(name, on) for name, on in (("contrast", calc_contrast), ("dissimilarity", calc_dissimilarity),
                                             ("homogeneity", calc_homogeneity), ("ASM", calc_ASM), ("energy", calc_energy),
                                             ("correlation", calc_correlation)) if on]
    if calculate_textural and textural_bands and tex_names:
        tx = texture_stats(img_data, labels, bands=textural_bands, start_label=start_label, n_labels=n, ctx=ctx)
        tx = _device.out(tx, False)
        for j, b in enumerate(textural_bands):
            for name, _ in tex_names:
                data[f"b{b}_{name}"] = tx[name][present, j]
    if pointcloud is not None and (calculate_structural or calculate_radiometric):
        from .pointcloud import segment_point_stats
        pc = segment_point_stats(pointcloud, labels, image.affine_transformation, voxel[2], start_label=start_label, n_labels=n, ctx=ctx)
        pc = _device.out(pc, False)
        wanted = [(name, on and calculate_structural) for name, on in (("pai", calc_pai), ("fhd", calc_fhd), ("ch", calc_ch))]
        wanted += [(name, on and calculate_radiometric) for name, on in (("mean_intensity", calc_mean_intensity),
                                                                        ("variance_intensity", calc_variance_intensity))]
        for name, on in wanted:
            if on:
                data[name] = pc[name][present]
    for c in cols:                                 # textural columns when calculate_textural=False, point-cloud columns not asked for: NaN
        if c not in data and c != "geometry":
            data[c] = np.full(n_rows, np.nan)
    geoms = [None] * n_rows
    crs = getattr(image, "crs", None)
    if geometry:
        if seg_table is not None and "geometry" in seg_table and len(seg_table) == n_rows:
            geoms = list(seg_table["geometry"])
        else:
            from .polygons import polygonize
            pt = polygonize(labels, affine_transformation=getattr(image, "affine_transformation", None),
                            start_label=start_label, ctx=ctx)
            if len(pt) != n_rows:
                raise RuntimeError(f"polygoniser returned {len(pt)} polygons for {n_rows} labels")
            geoms = pt.wkb()
    data["geometry"] = geoms
    df = pd.DataFrame(data, columns=cols)
    if geometry:
        try:                                       # the reference returns a GeoDataFrame; without its geo stack: WKB bytes
            import geopandas as gpd
            import shapely
            df = gpd.GeoDataFrame(df.drop(columns="geometry"), geometry=list(shapely.from_wkb(geoms)), crs=crs)[cols]
        except ImportError:
            pass
    df.attrs["crs"] = crs
    return df
