"""The preview path of the reference on the GPU: ``Image.to_image`` (obia/handlers/geotif.py:46-75) with its stretches
``rescale_to_8bit``, ``apply_histogram_equalization`` and ``apply_clahe`` (obia/utils/image.py:8-94), and the boundary overlay behind
``Segments.to_segmented_image`` (obia/segmentation/segment.py:41-53): ``find_boundaries`` and ``mark_boundaries_u8``.  The passes run
in libobia_hip.so (csrc/image.hip, include/obia_image.h); the host interpolates the two percentiles from the order statistics the
device selects and builds the 256-entry equalisation table from the histogram the device counts.  NumPy in -> NumPy out, CUDA tensor
in -> CUDA tensor out.

The sharpness raster of the same module of the reference (obia/utils/image.py:97-136) is here too: ``rgb_to_gray``, ``box_filter``
(``scipy.ndimage.uniform_filter``), ``variance_of_laplacian`` and ``laplacian`` (csrc/sharpness.hip, include/obia_sharpness.h).

What the results are pinned to:
  * ``rescale_to_8bit``: the reference's three NumPy expressions, evaluated literally;
  * ``find_boundaries`` / ``mark_boundaries_u8``: scikit-image 0.18.3, through committed goldens;
  * ``apply_histogram_equalization`` / ``apply_clahe``: OpenCV's algorithms (cvtColor RGB2GRAY, equalizeHist, CLAHE) RESTATED in
    tests/image_restatement.py.  They are NOT compared with ``cv2`` anywhere: OpenCV is not installed where the tests run.
  * ``box_filter``: SciPy 1.15.3's ``uniform_filter`` bit for bit, through committed goldens -- a serial running sum in double along
    every line, which the kernels walk in SciPy's order;
  * ``rgb_to_gray`` and the stretch of ``laplacian``: the reference's NumPy expressions, evaluated literally;
  * the 3 x 3 Laplacian of ``variance_of_laplacian``: ``cv2.Laplacian(gray, CV_32F, ksize=3)`` RESTATED in
    tests/sharpness_restatement.py (filter2D with [[2, 0, 2], [0, -8, 0], [2, 0, 2]], BORDER_REFLECT_101, float32 accumulation over the
    taps in row-major order).  It is NOT compared with ``cv2`` anywhere either.
"""
import ctypes
import os

import numpy as np

from . import _device, _lib, _percentile

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

_STRETCHES = (None, "histogram_equalization", "clahe")
_MAX_SELECT = 2 ** 32 - 2          # obia_cost_select_dev takes 1 <= n < 2^32 - 1
_I32_MAX = 2 ** 31 - 1


def _need_torch():
    _device.need_torch("obia_amd.image")


def _shape(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def _dtype_name(x):
    """'float32', 'uint8', ...: of a tensor, an array or anything NumPy accepts"""
    if _device.is_torch(x):
        return str(x.dtype).replace("torch.", "")
    return np.asarray(x).dtype.name


def _u8_dev(x, dev):
    """contiguous uint8 tensor on cuda:dev (the caller has checked the dtype)"""
    if _device.is_torch(x):
        return x.to(device=f"cuda:{dev}").contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x)), device=f"cuda:{dev}")


def _check_u8(image, who, three_only=False):
    name = _dtype_name(image)
    if name != "uint8":
        raise TypeError(f"{who} takes a uint8 image, got {name}")
    shp = _shape(image)
    ok = (len(shp) == 3 and shp[2] == 3) or (len(shp) == 2 and not three_only)
    if not ok or 0 in shp:
        raise ValueError(f"{who} takes a non-empty (H, W, 3){'' if three_only else ' or (H, W)'} image, got shape {shp}")
    return shp


# ------------------------------------------------------------------------------------------------------------ the stretch
_FLOAT_IN = {"float32": "float32", "float64": "float64", "uint8": "float32", "uint16": "float32", "int16": "float32"}


def _stretch_input(image, who):
    name = _dtype_name(image)
    if name not in _FLOAT_IN:
        raise TypeError(f"{who} takes float32, float64, uint8, uint16 or int16, got {name}")
    n = int(np.prod(_shape(image), dtype=np.int64))
    if n > _MAX_SELECT:
        raise NotImplementedError(f"{who}: {n} elements; the percentile select takes fewer than 2^32 - 1")
    return getattr(torch, _FLOAT_IN[name]), n


def _rescale_dev(lib, c, x, p_lo, p_hi):
    """uint8 tensor of x's shape from a float32 / float64 device tensor (contiguous, 16-byte aligned, not empty)"""
    q = _percentile.quantiles(p_lo, p_hi)
    lo, hi, n_valid = _percentile.select(lib, c, x, q)
    if n_valid < x.numel():
        raise ValueError(f"rescale_to_8bit: {x.numel() - n_valid} NaN in the image (the reference's cast of NaN to uint8 is undefined)")
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _lib.check(lib.obia_image_stretch_u8_dev(c.handle, x.data_ptr(), int(x.dtype == torch.float64), x.numel(), lo, hi, out.data_ptr()))
    return out


def rescale_to_8bit(image, min=2, max=98, ctx=None):
    """obia.utils.image.rescale_to_8bit: ``p_min, p_max = np.percentile(image, (min, max))`` over ALL elements (float64 for float32
    input under NumPy >= 2), zeros when they are equal, else ``np.clip(255 * (image - p_min) / (p_max - p_min), 0, 255)`` in float64,
    truncated to uint8.  Any shape; float32, float64, uint8, uint16 or int16 (the integers are taken as float32, which holds them
    exactly).  Deviation: a NaN anywhere raises ValueError (the reference casts NaN to uint8, which is undefined)."""
    _need_torch()
    is_t = _device.is_torch(image)
    dev = _device.device_of(ctx, image)
    dt, n = _stretch_input(image, "rescale_to_8bit")
    shp = _shape(image)
    if n == 0:
        empty = torch.empty(shp, dtype=torch.uint8, device=f"cuda:{dev}") if is_t else np.zeros(shp, np.uint8)
        return empty
    x = _device.as_dev(image if is_t else np.asarray(image), dt, dev, align16=True)
    lib, c = _device.begin(dev, ctx)
    out = _rescale_dev(lib, c, x, min, max)
    _device.end(lib, c)
    return _device.out(out.reshape(shp), is_t)


# ----------------------------------------------------------------------------------------------------------- equalisation
def equalization_table(hist):
    """cv::equalizeHist's table from the 256-bin histogram, or None when one bin holds every pixel (the output is the input):
    scale = 255.f / (total - hist[first]) and lut[j] = saturate(round_half_even(sum * scale)) in float32, lut[first] = 0."""
    hist = np.asarray(hist, np.int64)
    total = int(hist.sum())
    first = int(np.flatnonzero(hist)[0])
    if hist[first] == total:
        return None
    scale = np.float32(255.0) / np.float32(total - int(hist[first]))
    sums = np.cumsum(hist[first + 1:]).astype(np.float32)           # int -> float32, as the C cast rounds
    lut = np.zeros(256, np.uint8)
    lut[first + 1:] = np.clip(np.rint(sums * scale), 0, 255).astype(np.uint8)
    return lut


def _equalize_dev(lib, c, x):
    """(H, W, 3) uint8 tensor: the equalised grey plane of the (H, W) or (H, W, 3) uint8 device tensor x, three times"""
    H, W = x.shape[:2]
    n = H * W
    if n > _I32_MAX:
        raise NotImplementedError(f"apply_histogram_equalization: {n} pixels; OpenCV counts them in an int")
    nch = 3 if x.dim() == 3 else 1
    hist = torch.empty(256, dtype=torch.int64, device=x.device)
    gray = torch.empty((H, W), dtype=torch.uint8, device=x.device) if nch == 3 else x
    _lib.check(lib.obia_image_gray_hist_dev(c.handle, x.data_ptr(), nch, n, gray.data_ptr() if nch == 3 else None, hist.data_ptr()))
    _device.end(lib, c)
    lut = equalization_table(hist.cpu().numpy())
    if lut is None:
        lut = np.arange(256, dtype=np.uint8)
    lut_d = torch.as_tensor(lut, device=x.device)
    torch.cuda.current_stream(x.device).synchronize()
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device)
    _lib.check(lib.obia_image_lut_u8_dev(c.handle, gray.data_ptr(), n, lut_d.data_ptr(), 3, out.data_ptr()))
    _device.end(lib, c)              # lut_d and gray are still alive here
    return out


def apply_histogram_equalization(image, ctx=None):
    """obia.utils.image.apply_histogram_equalization: uint8 (H, W) or (H, W, 3) -> uint8 (H, W, 3), the equalised grey plane stacked
    three times.  OpenCV's ``cvtColor(RGB2GRAY)`` ((9798 R + 19235 G + 3735 B + 16384) >> 15) and ``equalizeHist`` restated; NOT
    compared with cv2 anywhere (module docstring)."""
    _need_torch()
    _check_u8(image, "apply_histogram_equalization")
    is_t = _device.is_torch(image)
    dev = _device.device_of(ctx, image)
    x = _u8_dev(image, dev)
    lib, c = _device.begin(dev, ctx)
    return _device.out(_equalize_dev(lib, c, x), is_t)


# ------------------------------------------------------------------------------------------------------------------ CLAHE
def _clahe_dev(lib, c, x):
    H, W = x.shape[:2]
    nch = x.shape[2] if x.dim() == 3 else 1
    out = torch.empty_like(x)
    for ch in range(nch):
        _lib.check(lib.obia_image_clahe_u8_dev(c.handle, x.data_ptr(), H, W, nch, ch, out.data_ptr()))
    return out


def apply_clahe(image, ctx=None):
    """obia.utils.image.apply_clahe: ``cv2.createCLAHE(clipLimit=2.0, tileGridSize=(8, 8)).apply`` on each channel of a uint8 (H, W) or
    (H, W, 3) image; same shape out.  OpenCV's algorithm restated; NOT compared with cv2 anywhere (module docstring).  Deviation:
    H < 8 or W < 8 raises ValueError (a tile grid wider than the image)."""
    _need_torch()
    shp = _check_u8(image, "apply_clahe")
    if shp[0] < 8 or shp[1] < 8:
        raise ValueError(f"apply_clahe needs at least 8 x 8 pixels for its 8 x 8 tiles, got {shp[0]} x {shp[1]}")
    is_t = _device.is_torch(image)
    dev = _device.device_of(ctx, image)
    x = _u8_dev(image, dev)
    lib, c = _device.begin(dev, ctx)
    out = _clahe_dev(lib, c, x)
    _device.end(lib, c)
    return _device.out(out, is_t)


# --------------------------------------------------------------------------------------------------------------- to_image
def _check_bands(bands, num_bands, stretch_type):
    if not isinstance(bands, (list, tuple)) or len(bands) != 3:
        raise ValueError("'bands' should be a list or tuple of exactly three elements")
    for band in bands:
        if band >= num_bands or band < 0:
            raise IndexError(f"Band index {band} out of range. Available bands indices: 0 to {num_bands - 1}.")
    if stretch_type not in _STRETCHES:
        raise ValueError(f"Unknown stretch_type: {stretch_type}")


def to_image(image, bands, p_min=2, p_max=98, stretch_type=None, *, as_array=False, ctx=None):
    """Image.to_image (geotif.py:46-75): the three ``bands`` of an (H, W, C) raster (or of ``image.img_data``) as float32, stretched
    between the ``p_min`` and ``p_max`` percentiles taken over the three bands TOGETHER (rescale_to_8bit), then ``stretch_type``
    None, "histogram_equalization" or "clahe".  Returns a PIL image (mode RGB) as the reference does; ``as_array=True`` returns the
    uint8 (H, W, 3) array instead -- a CUDA tensor, with no host copy, when the raster is one."""
    _need_torch()
    img = image.img_data if hasattr(image, "img_data") else image
    shp = _shape(img)
    if not isinstance(bands, (list, tuple)) or len(bands) != 3:
        raise ValueError("'bands' should be a list or tuple of exactly three elements")
    if len(shp) != 3:
        raise ValueError(f"to_image takes an (H, W, C) raster, got shape {shp}")
    _check_bands(bands, shp[2], stretch_type)
    if stretch_type == "clahe" and (shp[0] < 8 or shp[1] < 8):
        raise ValueError(f"apply_clahe needs at least 8 x 8 pixels for its 8 x 8 tiles, got {shp[0]} x {shp[1]}")
    if 0 in shp:
        raise ValueError("to_image of an empty raster")
    if 3 * shp[0] * shp[1] > _MAX_SELECT:
        raise NotImplementedError(f"to_image: {3 * shp[0] * shp[1]} values; the percentile select takes fewer than 2^32 - 1")
    is_t = _device.is_torch(img)
    dev = _device.device_of(ctx, img)
    idx = [int(b) for b in bands]
    if is_t:
        rgb = img.to(device=f"cuda:{dev}")[:, :, idx].to(torch.float32).contiguous()
    else:
        rgb = torch.as_tensor(np.ascontiguousarray(np.asarray(img)[:, :, idx], dtype=np.float32), device=f"cuda:{dev}")
    if rgb.data_ptr() % 16:
        rgb = rgb.clone()
    lib, c = _device.begin(dev, ctx)
    out = _rescale_dev(lib, c, rgb, p_min, p_max)
    del rgb
    if stretch_type == "histogram_equalization":
        out = _equalize_dev(lib, c, out)
    elif stretch_type == "clahe":
        out = _clahe_dev(lib, c, out)
    _device.end(lib, c)
    if as_array:
        return _device.out(out, is_t)
    from PIL.Image import fromarray
    return fromarray(out.cpu().numpy())


class Image:
    """The reference's raster holder (obia/handlers/geotif.py:8-44): ``img_data`` (H, W, C) -- an array or a CUDA tensor --, ``crs``,
    ``affine_transformation``, ``transform``, ``rasterio_obj``."""

    def __init__(self, img_data, crs=None, affine_transformation=None, transform=None, rasterio_obj=None):
        self.img_data = img_data
        self.crs = crs
        self.affine_transformation = affine_transformation
        self.transform = transform
        self.rasterio_obj = rasterio_obj

    def to_image(self, bands, p_min=2, p_max=98, stretch_type=None, *, as_array=False, ctx=None):
        """:func:`to_image` of this raster."""
        return to_image(self, bands, p_min=p_min, p_max=p_max, stretch_type=stretch_type, as_array=as_array, ctx=ctx)

    def laplacian(self, win, out_path=None, *, bands=(1, 2, 4), ctx=None):
        """:func:`laplacian` of this raster."""
        return laplacian(self, out_path, win, bands=bands, ctx=ctx)


# -------------------------------------------------------------------------------------------------------- sharpness raster
_GRAY_COEFFS = (0.299, 0.587, 0.114)


def _check_win(win, who):
    if isinstance(win, bool) or not isinstance(win, (int, np.integer)) or win < 1:
        raise ValueError(f"{who}: win must be an integer >= 1, got {win!r}")
    if win > _lib.SHARP_MAX_WIN:
        raise NotImplementedError(f"{who}: win {win} is larger than {_lib.SHARP_MAX_WIN}")
    return int(win)


def _check_plane(x, who, what):
    """shape of a non-empty (H, W) plane of a dtype the module takes as float32"""
    name = _dtype_name(x)
    if name not in _FLOAT_IN:
        raise TypeError(f"{who} takes float32, float64, uint8, uint16 or int16, got {name}")
    shp = _shape(x)
    if len(shp) != 2 or 0 in shp:
        raise ValueError(f"{who} takes a non-empty (H, W) {what}, got shape {shp}")
    if shp[0] * shp[1] > _MAX_SELECT:
        raise NotImplementedError(f"{who}: {shp[0] * shp[1]} pixels; the percentile select takes fewer than 2^32 - 1")
    return shp


def _raise_nonfinite(lib, c, counter, who, what):
    """the one counter a sharpness call reads back"""
    _device.end(lib, c)
    bad = int(counter.item())
    if bad:
        raise ValueError(f"{who}: {bad} NaN or infinite values in {what} (the reference would write an all-NaN raster)")


def rgb_to_gray(rgb):
    """obia.utils.image.rgb_to_gray: ``(rgb * float32([0.299, 0.587, 0.114])).sum(axis=-1)`` of an (H, W, 3) raster taken as float32,
    which for three elements is ``(r * 0.299f + g * 0.587f) + b * 0.114f`` with every product and sum rounded to float32.  Plain
    elementwise torch on the device (one rounding per operation, nothing fused): bit-equal to the NumPy expression."""
    _need_torch()
    shp = _shape(rgb)
    if len(shp) != 3 or shp[2] != 3:
        raise ValueError(f"rgb_to_gray takes an (H, W, 3) raster, got shape {shp}")
    name = _dtype_name(rgb)
    if name not in _FLOAT_IN:
        raise TypeError(f"rgb_to_gray takes float32, float64, uint8, uint16 or int16, got {name}")
    is_t = _device.is_torch(rgb)
    dev = _device.device_of(None, rgb)
    x = _device.as_dev(rgb, torch.float32, dev)
    c0, c1, c2 = (float(np.float32(v)) for v in _GRAY_COEFFS)
    gray = (x[..., 0] * c0 + x[..., 1] * c1) + x[..., 2] * c2
    return _device.out(gray, is_t)


def box_filter(plane, win, ctx=None):
    """``scipy.ndimage.uniform_filter(plane.astype(float32), size=win)`` (mode "reflect") of an (H, W) plane, bit for bit with SciPy
    1.15.3: the running sum in double along every column, then along every row of that float32 result, each line walked by one lane
    in SciPy's order.  Deviation: a NaN or an infinity in the plane raises ValueError."""
    _need_torch()
    win = _check_win(win, "box_filter")
    H, W = _check_plane(plane, "box_filter", "plane")
    is_t = _device.is_torch(plane)
    dev = _device.device_of(ctx, plane)
    x = _device.as_dev(plane, torch.float32, dev)
    work = torch.empty((H, W), dtype=torch.float32, device=x.device)
    out = torch.empty((H, W), dtype=torch.float32, device=x.device)
    bad = torch.empty(1, dtype=torch.int64, device=x.device)
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_sharp_box_dev(c.handle, x.data_ptr(), H, W, win, work.data_ptr(), out.data_ptr(), bad.data_ptr()))
    _raise_nonfinite(lib, c, bad, "box_filter", "the plane")
    return _device.out(out, is_t)


def _variance_dev(lib, c, lap, win):
    """variance of the Laplacian from the device plane ``lap``"""
    H, W = lap.shape
    work = torch.empty((2, H, W), dtype=torch.float32, device=lap.device)
    out = torch.empty((H, W), dtype=torch.float32, device=lap.device)
    _lib.check(lib.obia_sharp_variance_dev(c.handle, lap.data_ptr(), H, W, win, work.data_ptr(), out.data_ptr()))
    _device.end(lib, c)              # work is still alive here
    return out


def variance_of_laplacian(gray, win, ctx=None):
    """obia.utils.image.variance_of_laplacian: ``lap = cv2.Laplacian(gray, CV_32F, ksize=3)``, ``mean = uniform_filter(lap, win)``,
    ``mean2 = uniform_filter(lap * lap, win)``, ``mean2 - mean ** 2`` in float32, of an (H, W) plane taken as float32.  The Laplacian
    is OpenCV's restated and NOT compared with cv2 anywhere (module docstring).  Deviation: a NaN or an infinity in ``gray`` raises
    ValueError.  A ``gray`` whose squared Laplacian overflows float32 is not specified."""
    _need_torch()
    win = _check_win(win, "variance_of_laplacian")
    H, W = _check_plane(gray, "variance_of_laplacian", "grey plane")
    is_t = _device.is_torch(gray)
    dev = _device.device_of(ctx, gray)
    x = _device.as_dev(gray, torch.float32, dev)
    lap = torch.empty((H, W), dtype=torch.float32, device=x.device)
    bad = torch.empty(1, dtype=torch.int64, device=x.device)
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_sharp_laplacian_dev(c.handle, x.data_ptr(), H, W, lap.data_ptr(), bad.data_ptr()))
    _raise_nonfinite(lib, c, bad, "variance_of_laplacian", "the grey plane")
    return _device.out(_variance_dev(lib, c, lap, win), is_t)


def laplacian(image, out_path, win, *, bands=(1, 2, 4), ctx=None):
    """obia.utils.image.laplacian(in_path, out_path, win) at array level: the three ``bands`` (0-based; the default is the reference's
    1-based [2, 3, 5]) of an (H, W, C) raster -- an array, a CUDA tensor or an :class:`Image` -- as float32, each normalised by
    ``(x - min) / ((max - min) + 1e-8)``, :func:`rgb_to_gray`, :func:`variance_of_laplacian` with window ``win``, then
    ``np.clip((sharp - lo) / (hi - lo), 0, 1)`` in float64 between the 2nd and 98th percentiles of ``sharp``, as float32 (H, W).
    ``hi == lo`` is taken literally: NaN where ``sharp == lo``, 0 below, 1 above (a constant raster gives all NaN).

    ``out_path`` must be None and ``image`` must not be a path: GeoTIFF I/O stays with the caller.  Deviation: a NaN or
    an infinity in one of the three bands raises ValueError (the reference writes an all-NaN raster)."""
    _need_torch()
    if out_path is not None:
        raise NotImplementedError("laplacian: out_path must be None -- GeoTIFF I/O stays with the caller (DESIGN.md 6); write the "
                                  "returned raster with rasterio")
    if isinstance(image, (str, bytes, os.PathLike)):
        raise NotImplementedError("laplacian takes the raster itself, not a path -- GeoTIFF I/O stays with the caller (DESIGN.md 6); "
                                  "read it with rasterio and move the bands last")
    win = _check_win(win, "laplacian")
    img = image.img_data if hasattr(image, "img_data") else image
    shp = _shape(img)
    if not isinstance(bands, (list, tuple)) or len(bands) != 3:
        raise ValueError("'bands' should be a list or tuple of exactly three elements")
    if len(shp) != 3:
        raise ValueError(f"laplacian takes an (H, W, C) raster, got shape {shp}")
    _check_bands(bands, shp[2], None)
    if 0 in shp:
        raise ValueError("laplacian of an empty raster")
    name = _dtype_name(img)
    if name not in _FLOAT_IN:
        raise TypeError(f"laplacian takes float32, float64, uint8, uint16 or int16, got {name}")
    H, W, C = shp
    if H * W > _MAX_SELECT:
        raise NotImplementedError(f"laplacian: {H * W} pixels; the percentile select takes fewer than 2^32 - 1")
    is_t = _device.is_torch(img)
    dev = _device.device_of(ctx, img)
    idx = [int(b) for b in bands]
    if is_t and img.dtype == torch.float32:
        x = img.to(device=f"cuda:{dev}").contiguous()         # the kernels pick the bands out of the raster as it is
    elif is_t:
        x, idx = img.to(device=f"cuda:{dev}")[:, :, idx].to(torch.float32).contiguous(), [0, 1, 2]
    else:
        x = torch.as_tensor(np.ascontiguousarray(np.asarray(img)[:, :, idx], dtype=np.float32), device=f"cuda:{dev}")
        idx = [0, 1, 2]
    lap = torch.empty((H, W), dtype=torch.float32, device=x.device)
    bad = torch.empty(1, dtype=torch.int64, device=x.device)
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_sharp_gray_lap_dev(c.handle, x.data_ptr(), H, W, x.shape[2], (ctypes.c_int32 * 3)(*idx), lap.data_ptr(),
                                           bad.data_ptr()))
    _raise_nonfinite(lib, c, bad, "laplacian", f"bands {tuple(int(b) for b in bands)}")
    del x
    sharp = _variance_dev(lib, c, lap, win)
    del lap
    lo, hi, _ = _percentile.select(lib, c, sharp, _percentile.quantiles(2, 98))
    out = torch.empty((H, W), dtype=torch.float32, device=sharp.device)
    _lib.check(lib.obia_sharp_stretch_f32_dev(c.handle, sharp.data_ptr(), H * W, lo, hi, out.data_ptr()))
    _device.end(lib, c)
    return _device.out(out, is_t)


# ------------------------------------------------------------------------------------------------------------- boundaries
def mark_table():
    """What ``(mark_boundaries(img, ...) * 255).astype(uint8)`` leaves of a uint8 value v away from the boundaries:
    ``img_as_float`` multiplies by 1 / 255 in float64, the caller by 255, the cast truncates -- not the identity for every v."""
    v = np.multiply(np.arange(256, dtype=np.uint8), 1.0 / 255, dtype=np.float64)
    return (v * 255).astype(np.uint8)


def _labels_dev(labels, dev, shape=None):
    shp = _shape(labels)
    if len(shp) != 2 or 0 in shp:
        raise ValueError(f"labels must be a non-empty (H, W) raster, got shape {shp}")
    if shape is not None and shp != tuple(shape):
        raise ValueError(f"the label raster is {shp[0]} x {shp[1]}, the image {shape[0]} x {shape[1]}")
    lab = _device.as_dev(labels, torch.int32, dev)
    if int(lab.max()) == _I32_MAX:
        raise ValueError("2^31 - 1 cannot be a label: find_boundaries uses it for the background")
    return lab


def find_boundaries(labels, mode="outer", background=0, ctx=None):
    """skimage.segmentation.find_boundaries(labels, connectivity=1, mode="outer", background=0) as a uint8 0 / 1 (H, W) raster; labels
    are taken as int32 and may be negative (only 0 is background).  Other modes and backgrounds raise NotImplementedError."""
    _need_torch()
    if mode != "outer":
        raise NotImplementedError(f"find_boundaries: only mode='outer' is built, got {mode!r}")
    if background != 0:
        raise NotImplementedError(f"find_boundaries: only background=0 is built, got {background!r}")
    is_t = _device.is_torch(labels)
    dev = _device.device_of(ctx, labels)
    lab = _labels_dev(labels, dev)
    H, W = lab.shape
    out = torch.empty((H, W), dtype=torch.uint8, device=lab.device)
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_image_boundaries_dev(c.handle, lab.data_ptr(), H, W, out.data_ptr()))
    _device.end(lib, c)
    return _device.out(out, is_t)


def mark_boundaries_u8(rgb_u8, labels, color=(255, 255, 0), ctx=None):
    """``(skimage.segmentation.mark_boundaries(rgb_u8, labels, color=color / 255) * 255).astype(uint8)`` with scikit-image's
    defaults (mode "outer", background 0): ``color`` at the boundary pixels, :func:`mark_table` of the image elsewhere.  uint8
    (H, W, 3) or (H, W) (grey, replicated) in, uint8 (H, W, 3) out."""
    _need_torch()
    shp = _check_u8(rgb_u8, "mark_boundaries_u8")
    rgb = [int(v) for v in color]
    if len(rgb) != 3 or any(v < 0 or v > 255 for v in rgb):
        raise ValueError(f"color must be three values in 0..255, got {color!r}")
    is_t = _device.is_torch(rgb_u8) or _device.is_torch(labels)
    dev = _device.device_of(ctx, rgb_u8, labels)
    lab = _labels_dev(labels, dev, shp[:2])
    x = _u8_dev(rgb_u8, dev)
    H, W = shp[:2]
    table = torch.as_tensor(mark_table(), device=x.device)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device)
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_image_mark_u8_dev(c.handle, x.data_ptr(), 3 if len(shp) == 3 else 1, lab.data_ptr(), H, W, table.data_ptr(),
                                          (ctypes.c_uint8 * 3)(*rgb), out.data_ptr()))
    _device.end(lib, c)
    return _device.out(out, is_t)
