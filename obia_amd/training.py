"""Training tiles of the reference on the GPU: ``obia.utils.training.tile_and_process`` (obia/utils/training.py:16-338) at array level.

A raster is cut into overlapping tiles and every tile becomes the 8-bit image a detector is trained on: the percentile stretch
(``obia_amd.image.rescale_to_8bit``) or the min-max scaling, CLAHE per channel (``apply_clahe``), and -- with a canopy mask -- a
Gaussian blur of the result, darkened, as the background of a hard or feathered blend.  Beside the images come the per-tile
geotransforms (``transforms.json``) and, from polygon bounds, the bounding-box annotations (``annotations.json``).  The new passes run
in libobia_hip.so (csrc/training.hip, include/obia_training.h); GeoTIFF and GeoPackage I/O stays with the caller.
NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out.

What the results are pinned to:
  * ``gaussian_blur_u8``: ``cv2.GaussianBlur(src, (kx, ky), 0)`` for uint8 RESTATED as integer arithmetic (8.8 fixed-point weights per
    axis, one rounding at the end, BORDER_REFLECT_101) in tests/training_restatement.py;
  * ``chamfer_distance``: ``cv2.distanceTransform(src, DIST_L2, 3)`` RESTATED there as OpenCV's two-pass 3 x 3 sweep; the kernels
    evaluate the closed form the sweep has on a grid;
  * both are NOT compared with ``cv2`` anywhere: OpenCV is not installed where the tests run.  The weights for ksize <= 7 are OpenCV's
    small-kernel table; those for ksize >= 9 follow the rule in :func:`gaussian_weights`, and their agreement with OpenCV's own table is
    unverified;
  * darkening, the two blends and the min-max scaling: the reference's NumPy expressions, evaluated literally.
"""
import json
import math
import os

import numpy as np

from . import _device, _lib
from . import image as _image
from .seeds import invert_affine

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

_SMALL_WEIGHTS = {1: (256,), 3: (64, 128, 64), 5: (16, 64, 96, 64, 16), 7: (8, 28, 56, 72, 56, 28, 8)}
CHAMFER_HV = 62587            # round(0.955 * 65536)
CHAMFER_DG = 89738            # round(1.3693 * 65536)
CHAMFER_MAX = (2 ** 31 - 1) >> 2
_KEEP_BYTES = 256 << 20       # temporaries of a tile_and_process call held between two waits for the stream


def _need_torch():
    _device.need_torch("obia_amd.training")


# ------------------------------------------------------------------------------------------------------------------ blur
def gaussian_weights(k):
    """The integer weights of one axis of ``cv2.GaussianBlur(..., (k, k), 0)`` on uint8: ``k`` values that sum to 256 (int32).

    k = 1, 3, 5, 7: OpenCV's small-kernel table ({256}, {64, 128, 64}, {16, 64, 96, 64, 16}, {8, 28, 56, 72, 56, 28, 8}), exact in
    8.8 fixed point.  Odd k from 9 to 31: sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8, g_i = exp(-x_i^2 / (2 sigma^2)) normalised in
    float64, quantised from the ends inward with error diffusion (v = 256 g_i + err, q = floor(v + 0.5), err = v - q, w_i = w_(k-1-i)
    = q for i < k // 2); the centre tap is 256 minus the others.  The agreement of these with OpenCV's own table is unverified."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k > _lib.TRAIN_MAX_KSIZE or k % 2 == 0:
        raise ValueError(f"a blur kernel size must be an odd integer in 1..{_lib.TRAIN_MAX_KSIZE}, got {k!r}")
    k = int(k)
    if k in _SMALL_WEIGHTS:
        return np.array(_SMALL_WEIGHTS[k], np.int32)
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) * 0.5
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    g = g / g.sum()
    w = np.zeros(k, np.int64)
    err = 0.0
    for i in range(k // 2):
        v = 256.0 * g[i] + err
        q = math.floor(v + 0.5)
        err = v - q
        w[i] = w[k - 1 - i] = q
    w[k // 2] = 256 - int(w.sum())
    return w.astype(np.int32)


def _ksize(ksize):
    """(kx, ky) of an int or a pair, as cv2 takes it; (0, 0) for "no blur" """
    if isinstance(ksize, (int, np.integer)) and not isinstance(ksize, bool):
        pair = (int(ksize), int(ksize))
    elif isinstance(ksize, (tuple, list)) and len(ksize) == 2 and all(
            isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in ksize):
        pair = (int(ksize[0]), int(ksize[1]))
    else:
        raise ValueError(f"blur kernel must be an int or a (kx, ky) pair of ints, got {ksize!r}")
    if pair == (0, 0):
        return pair
    for v in pair:
        if v < 1 or v > _lib.TRAIN_MAX_KSIZE or v % 2 == 0:
            raise ValueError(f"a blur kernel size must be an odd integer in 1..{_lib.TRAIN_MAX_KSIZE} (or 0 for none), got {ksize!r}")
    return pair


def _weights_dev(pair, device):
    """(wx, wy) int32 device tensors of a kernel pair; None for (0, 0)"""
    if pair == (0, 0):
        return None
    return (torch.as_tensor(gaussian_weights(pair[0]), device=device), torch.as_tensor(gaussian_weights(pair[1]), device=device))


def _blur_dev(lib, c, x, pair, weights):
    H, W = x.shape[:2]
    out = torch.empty_like(x)
    _lib.check(lib.obia_train_blur_u8_dev(c.handle, x.data_ptr(), H, W, 3 if x.dim() == 3 else 1, pair[0], pair[1],
                                          weights[0].data_ptr(), weights[1].data_ptr(), out.data_ptr()))
    return out


def gaussian_blur_u8(image, ksize, ctx=None):
    """``cv2.GaussianBlur(image, ksize, 0)`` of a uint8 (H, W) or (H, W, 3) image, restated as integer arithmetic: per axis the weights
    of :func:`gaussian_weights`, S = sum wy * wx * p, out = (S + 32768) >> 16, BORDER_REFLECT_101 (applied repeatedly for a side shorter
    than half the kernel).  ``ksize``: an odd int or a ``(kx, ky)`` pair, as cv2 takes it, each at most 31; ``0`` or ``(0, 0)`` returns
    the input, as the reference's branch does.  NOT compared with cv2 anywhere (module docstring)."""
    _need_torch()
    _image._check_u8(image, "gaussian_blur_u8")
    pair = _ksize(ksize)
    if pair == (0, 0):
        return image
    is_t = _device.is_torch(image)
    dev = _device.device_of(ctx, image)
    x = _image._u8_dev(image, dev)
    weights = _weights_dev(pair, x.device)
    lib, c = _device.begin(dev, ctx)
    out = _blur_dev(lib, c, x, pair, weights)
    _device.end(lib, c)
    return _device.out(out, is_t)


# -------------------------------------------------------------------------------------------------------------- distance
def _distance_dev(lib, c, x, R):
    H, W = x.shape
    work = torch.empty((H, W), dtype=torch.int32, device=x.device)
    out = torch.empty((H, W), dtype=torch.float32, device=x.device)
    _lib.check(lib.obia_train_distance_dev(c.handle, x.data_ptr(), H, W, int(R), work.data_ptr(), out.data_ptr()))
    return out, work


def chamfer_distance(image_u8, radius=None, ctx=None):
    """``cv2.distanceTransform(image_u8, cv2.DIST_L2, 3)`` of a uint8 (H, W) image as float32 (H, W): the fixed-point 3 x 3 chamfer
    distance of every pixel to the nearest zero pixel, min over them of (62587 * (max - min) + 89738 * min) / 65536 with max / min of the
    offset's |dx|, |dy| -- what OpenCV's forward / backward sweep gives on a grid.  ``radius`` R: only zero pixels within Chebyshev
    distance R count; a pixel with none gets 8192.0 (as does every pixel of an image without a zero).  None: the full transform.
    A side may be 4096 at the most.  NOT compared with cv2 anywhere (module docstring)."""
    _need_torch()
    shp = _image._check_u8(image_u8, "chamfer_distance")
    if len(shp) != 2:
        raise ValueError(f"chamfer_distance takes a non-empty (H, W) image, got shape {shp}")
    if max(shp) > _lib.TRAIN_MAX_SIDE:
        raise NotImplementedError(f"chamfer_distance: {shp[0]} x {shp[1]}; a side may be {_lib.TRAIN_MAX_SIDE} at the most")
    if radius is None:
        R = max(shp) - 1
    elif isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or radius < 0:
        raise ValueError(f"chamfer_distance: radius must be None or an integer >= 0, got {radius!r}")
    else:
        R = min(int(radius), _lib.TRAIN_MAX_SIDE)
    is_t = _device.is_torch(image_u8)
    dev = _device.device_of(ctx, image_u8)
    x = _image._u8_dev(image_u8, dev)
    lib, c = _device.begin(dev, ctx)
    out, work = _distance_dev(lib, c, x, R)
    _device.end(lib, c)              # work is still alive here
    return _device.out(out, is_t)


# ---------------------------------------------------------------------------------------------------------------- tiling
def generate_tiles(bounds, step, tile_size):
    """The reference's generator (training.py:16-33): boxes ``(minx, miny, maxx, maxy)`` stepping through ``bounds`` from the bottom row
    up and from left to right, clipped at the right and top edges."""
    minx, miny, maxx, maxy = bounds
    y = miny
    while y < maxy:
        x = minx
        tile_top = y + tile_size
        while x < maxx:
            tile_right = x + tile_size
            cur_maxx = min(tile_right, maxx)
            cur_maxy = min(tile_top, maxy)
            yield (x, y, cur_maxx, cur_maxy)
            x += step
        y += step


def _whole(value, what):
    n = round(value)
    if n < 1 or abs(value - n) > 1e-9 * max(abs(value), 1.0):
        raise ValueError(f"{what} must be a whole number of pixels, got {value!r} (rasterio's rounding of fractional windows is not restated)")
    return int(n)


def tile_windows(shape, affine_transformation, tile_size, overlap):
    """The tiles of :func:`generate_tiles` over a raster of ``shape`` (H, W, ...) as integer pixel windows.

    ``affine_transformation`` is ``[a, b, d, e, xoff, yoff]`` as everywhere in this package.  Returns ``(windows, transforms)``:
    ``windows[i] = (row_off, col_off, h, w)`` and ``transforms[i] = [a, b, c, d, e, f]`` (rasterio's order) of tile ``i`` in the
    reference's order: the bottom tile row first, left to right, tiles clipped at the top and right edges.

    ValueError unless the transform is north-up (b = d = 0, a > 0, e < 0), ``overlap < tile_size`` (a non-positive step makes the
    reference loop for ever) and ``tile_size`` and ``tile_size - overlap`` are whole numbers of pixels on both axes to within 1e-9
    relative (rasterio's rounding of fractional windows is not restated)."""
    H, W = int(shape[0]), int(shape[1])
    if H < 1 or W < 1:
        raise ValueError(f"tile_windows of an empty raster, shape {tuple(shape)}")
    a, b, d, e, xoff, yoff = [float(v) for v in affine_transformation]
    if b != 0.0 or d != 0.0 or not a > 0.0 or not e < 0.0:
        raise ValueError(f"tile_windows takes a north-up transform (b = d = 0, a > 0, e < 0), got {list(affine_transformation)!r}")
    tile_size, overlap = float(tile_size), float(overlap)
    if not tile_size > 0.0 or not overlap < tile_size:
        raise ValueError(f"overlap must be smaller than tile_size and tile_size positive, got tile_size {tile_size!r}, overlap {overlap!r}")
    step = tile_size - overlap
    tw, th = _whole(tile_size / a, "tile_size / pixel width"), _whole(tile_size / -e, "tile_size / pixel height")
    sw, sh = _whole(step / a, "(tile_size - overlap) / pixel width"), _whole(step / -e, "(tile_size - overlap) / pixel height")
    windows, transforms = [], []
    for from_bottom in range(0, H, sh):
        h = min(th, H - from_bottom)
        row_off = H - from_bottom - h
        for col_off in range(0, W, sw):
            w = min(tw, W - col_off)
            windows.append((row_off, col_off, h, w))
            transforms.append([a, b, a * col_off + b * row_off + xoff, d, e, d * col_off + e * row_off + yoff])
    return windows, transforms


def _bounds_table(boxes):
    if boxes is None:
        return None
    t = np.asarray(boxes.bounds if hasattr(boxes, "bounds") else boxes, dtype=np.float64)
    if t.ndim != 2 or t.shape[1] != 4:
        raise ValueError(f"boxes must be an (N, 4) table of polygon bounds (minx, miny, maxx, maxy), got shape {t.shape}")
    return t


def tile_annotations(bounds, affine_transformation, windows, names):
    """The reference's bounding boxes (training.py:139-145, 267-318) from polygon ``bounds`` (N, 4): per tile the polygons whose bounds
    lie within the tile's box, as ``[x_min, y_min, x_max, y_max]`` pixels of the tile -- floor of the inverse transform of (minx, maxy)
    and (maxx, miny), minus the window's offsets, clamped to the tile, degenerate boxes skipped, ``labels`` all 1.  A key exists only
    for a tile that contains a polygon."""
    a, b, d, e, xoff, yoff = [float(v) for v in affine_transformation]
    ra, rb, rc, rd, re, rf = invert_affine(affine_transformation)
    out = {}
    for (row_off, col_off, h, w), name in zip(windows, names):
        minx, maxx = a * col_off + xoff, a * (col_off + w) + xoff
        maxy, miny = e * row_off + yoff, e * (row_off + h) + yoff
        inside = (bounds[:, 0] >= minx) & (bounds[:, 1] >= miny) & (bounds[:, 2] <= maxx) & (bounds[:, 3] <= maxy)
        if not inside.any():
            continue
        boxes, labels = [], []
        for pxmin, pymin, pxmax, pymax in bounds[inside]:
            col_tl, row_tl = math.floor(ra * pxmin + rb * pymax + rc), math.floor(rd * pxmin + re * pymax + rf)
            col_br, row_br = math.floor(ra * pxmax + rb * pymin + rc), math.floor(rd * pxmax + re * pymin + rf)
            x_min, x_max = (max(0, min(v - col_off, w - 1)) for v in (col_tl, col_br))
            y_min, y_max = (max(0, min(v - row_off, h - 1)) for v in (row_tl, row_br))
            if x_min >= x_max or y_min >= y_max:
                continue
            boxes.append([x_min, y_min, x_max, y_max])
            labels.append(1)
        out[os.path.splitext(name)[0]] = {"file_name": name, "boxes": boxes, "labels": labels}
    return out


# ------------------------------------------------------------------------------------------------------------------ tiles
class _Settings:
    """the checked arguments of process_tile / tile_and_process; touches no device"""

    def __init__(self, feather_radius, blur_kernel, darken_factor, apply_clahe_flag, rescale):
        self.feather = float(feather_radius)
        if not self.feather >= 0.0 or math.isinf(self.feather):
            raise ValueError(f"feather_radius must be a finite number >= 0, got {feather_radius!r}")
        self.ksize = _ksize(blur_kernel)
        self.darken = float(darken_factor)
        if not 0.0 <= self.darken <= 1.0:
            raise ValueError(f"darken_factor must lie in 0..1, got {darken_factor!r}")
        self.clahe = bool(apply_clahe_flag)
        self.rescale = bool(rescale)
        self.radius = int(math.ceil(self.feather / 0.955)) + 1 if self.feather > 0.0 else 0   # anything farther has alpha == 0

    def darken_lut(self):
        """the reference's ``(blurred * darken_factor).astype(uint8)`` as a table; it skips darkening for 0"""
        if self.darken == 0.0:
            return np.arange(256, dtype=np.uint8)
        return (np.arange(256, dtype=np.uint8) * self.darken).astype(np.uint8)

    def check_tile(self, h, w, name, masked):
        if self.clahe and (h < 8 or w < 8):
            raise ValueError(f"{name}: apply_clahe needs at least 8 x 8 pixels for its 8 x 8 tiles, got {h} x {w}")
        if masked and self.feather > 0.0 and max(h, w) > _lib.TRAIN_MAX_SIDE:
            raise NotImplementedError(f"{name}: {h} x {w}; a feathered tile's side may be {_lib.TRAIN_MAX_SIDE} at the most")


class _Tables:
    """what every tile of a call reads: the darkening table and the blur weights on the device (uploaded once)"""

    def __init__(self, s, device, masked):
        self.lut = torch.as_tensor(s.darken_lut(), device=device) if masked else None
        self.weights = _weights_dev(s.ksize, device) if masked else None


def _tile_dev(lib, c, s, tables, x, m, inv, counters, keep):
    """One tile on the context's stream: ``x`` (h, w, 3) float32, ``m`` (h, w) uint8 mask or None, ``inv`` = 255 - 255 m when the
    blend is feathered; ``counters``: two int64 (bad mask bytes, non-finite values).  Temporaries go to ``keep``."""
    h, w = x.shape[:2]
    if s.rescale:
        u8 = _image._rescale_dev(lib, c, x, 2, 98)
    else:
        work = torch.empty(_lib.TRAIN_MINMAX_WORK, dtype=torch.float32, device=x.device)
        u8 = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        _lib.check(lib.obia_train_minmax_u8_dev(c.handle, x.data_ptr(), x.numel(), work.data_ptr(), u8.data_ptr(),
                                                counters[1:].data_ptr()))
        keep.append(work)
    final = _image._clahe_dev(lib, c, u8) if s.clahe else u8
    keep += [x, u8, final]
    if m is None:
        return final
    blurred = final if s.ksize == (0, 0) else _blur_dev(lib, c, final, s.ksize, tables.weights)
    dist = None
    if s.feather > 0.0:
        dist, work = _distance_dev(lib, c, inv, s.radius)
        keep += [work, dist, inv]
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=x.device)
    _lib.check(lib.obia_train_compose_u8_dev(c.handle, final.data_ptr(), blurred.data_ptr(), m.data_ptr(),
                                             dist.data_ptr() if dist is not None else None, h, w, tables.lut.data_ptr(), s.feather,
                                             out.data_ptr(), counters[:1].data_ptr()))
    keep += [blurred, m]
    return out


def _raise_counters(counts, names):
    """ValueError for the first tile whose counters are not zero; ``counts`` (n, 2) on the host"""
    for (bad_mask, nonfinite), name in zip(counts.tolist(), names):
        if nonfinite:
            raise ValueError(f"{name}: {nonfinite} NaN or infinite values in the tile (the reference's cast of NaN to uint8 is undefined)")
        if bad_mask:
            raise ValueError(f"{name}: {bad_mask} mask values other than 0 and 1")


def _mask_u8(mask, dev):
    """(H, W) uint8 device tensor of a mask given as bool or any integer / float type (cast as ``astype(uint8)`` casts)"""
    if _device.is_torch(mask):
        m = mask.to(device=f"cuda:{dev}")
        return (m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)).contiguous()
    m = np.asarray(mask)
    return torch.as_tensor(np.ascontiguousarray(m.astype(np.uint8, copy=False)), device=f"cuda:{dev}")


def process_tile(tile, mask=None, *, feather_radius=0.0, blur_kernel=5, darken_factor=0.8, apply_clahe_flag=True, rescale=True, ctx=None):
    """Steps (2) and (3) of the reference's loop (training.py:154-230) on one (h, w, 3) float32 tile; returns the (h, w, 3) uint8 tile.

    1. ``rescale``: :func:`obia_amd.image.rescale_to_8bit` over the three bands together; else the min-max branch, in float32:
       zeros when min == max, else ``clip(255 * (x - min) / (max - min), 0, 255)`` truncated.
    2. ``apply_clahe_flag``: CLAHE on each channel (the tile must be at least 8 x 8).
    3. With a ``mask`` ((h, w), values 0 and 1): the result of 2 blurred with ``blur_kernel`` (:func:`gaussian_blur_u8`; 0 = none) and
       darkened, ``(blurred * darken_factor).astype(uint8)`` (``darken_factor == 0`` skips it, as the reference does), is the
       background.  ``feather_radius == 0``: the unblurred result where the mask is 1, the background elsewhere.  Otherwise
       ``alpha = clip(1 - dist / feather_radius, 0, 1)`` with ``dist`` = :func:`chamfer_distance` of ``255 - 255 * mask`` (within a
       window of ceil(feather_radius / 0.955) + 1 pixels; anything farther has alpha == 0) and ``alpha * tile + (1 - alpha) *
       background`` in float32, clipped and truncated.  Without a mask nothing is blurred, exactly as in the reference.

    ValueError: ``darken_factor`` outside 0..1, ``feather_radius < 0``, a mask value other than 0 and 1 (counted on the device, read
    once per call), a NaN or an infinity in the tile."""
    _need_torch()
    s = _Settings(feather_radius, blur_kernel, darken_factor, apply_clahe_flag, rescale)
    shp = _image._shape(tile)
    if len(shp) != 3 or shp[2] != 3 or 0 in shp:
        raise ValueError(f"process_tile takes a non-empty (h, w, 3) tile, got shape {shp}")
    name = _image._dtype_name(tile)
    if name != "float32":
        raise TypeError(f"process_tile takes a float32 tile, got {name}")
    if mask is not None and _image._shape(mask) != shp[:2]:
        raise ValueError(f"the mask is {_image._shape(mask)}, the tile {shp[0]} x {shp[1]}")
    s.check_tile(shp[0], shp[1], "process_tile", mask is not None)
    is_t = _device.is_torch(tile)
    dev = _device.device_of(ctx, tile, mask)
    x = _device.as_dev(tile, torch.float32, dev, align16=True)
    m = _mask_u8(mask, dev) if mask is not None else None
    inv = (255 - m * 255) if m is not None and s.feather > 0.0 else None
    tables = _Tables(s, x.device, m is not None)
    counters = torch.zeros(2, dtype=torch.int64, device=x.device)
    keep = []
    lib, c = _device.begin(dev, ctx)
    out = _tile_dev(lib, c, s, tables, x, m, inv, counters, keep)
    _device.end(lib, c)
    _raise_counters(counters.cpu().numpy().reshape(1, 2), ["process_tile"])
    return _device.out(out, is_t)


class TrainingTiles:
    """What :func:`tile_and_process` returns: ``names`` (``img_001.jpg`` ...), ``images`` (uint8 (h, w, 3) each), ``transforms``
    (``{name: {"transform": [a, b, c, d, e, f], "crs": str}}``), ``annotations`` (``{"img_001": {"file_name", "boxes", "labels"}}``;
    None when no boxes were given) and ``windows`` (``(row_off, col_off, h, w)`` of each tile)."""

    def __init__(self, names, images, transforms, annotations, windows):
        self.names, self.images, self.transforms, self.annotations, self.windows = names, images, transforms, annotations, windows

    def __len__(self):
        return len(self.names)


def tile_and_process(raster, affine_transformation, crs, mask=None, boxes=None, output_dir=None, tile_size=150.0, overlap=50.0,
                     selected_bands=(4, 2, 1), feather_radius=0.0, blur_kernel=5, darken_factor=0.8, apply_clahe_flag=True, rescale=True,
                     *, as_array=False, ctx=None):
    """obia.utils.training.tile_and_process with arrays in place of paths; GeoTIFF and GeoPackage I/O stays with the caller.

    ``raster``: (H, W, C) float32, a NumPy array or a CUDA tensor, with ``affine_transformation`` = [a, b, d, e, xoff, yoff] and
    ``crs``; ``selected_bands``: three zero-based band indices; ``mask``: (H, W) canopy mask of 0 and 1, or None; ``boxes``: an (N, 4)
    array of polygon bounds (minx, miny, maxx, maxy), or anything with a ``.bounds`` table (a GeoDataFrame), or None.  A polygon lies
    within a tile exactly when its bounds do, so the reference's geometry filter reduces to comparisons of bounds.  The tiles are those
    of :func:`tile_windows`, each processed as :func:`process_tile` describes; the other parameters are the reference's.

    Returns a :class:`TrainingTiles`.  ``as_array=True`` leaves ``images`` as CUDA tensors; otherwise they are NumPy arrays.  With
    ``output_dir``: the tiles are written there as JPEG (through PIL -- the bytes are PIL's encoder's, not GDAL's as in the reference),
    ``transforms.json`` and, when ``boxes`` was given, ``annotations.json`` with ``json.dump(..., indent=2)``.

    All tiles of a call are queued on one stream; the library does not wait between tiles beyond what the percentile stretch does
    (it reads its two order statistics back), and the mask and NaN counters of all tiles are read once at the end.  Temporaries are held
    until the stream has been waited for, which a call does whenever they exceed 256 MiB."""
    _need_torch()
    s = _Settings(feather_radius, blur_kernel, darken_factor, apply_clahe_flag, rescale)
    shp = _image._shape(raster)
    if len(shp) != 3 or 0 in shp:
        raise ValueError(f"tile_and_process takes a non-empty (H, W, C) raster, got shape {shp}")
    name = _image._dtype_name(raster)
    if name != "float32":
        raise TypeError(f"tile_and_process takes a float32 raster, got {name}")
    if not isinstance(selected_bands, (list, tuple)) or len(selected_bands) != 3:
        raise ValueError("'selected_bands' should be a list or tuple of exactly three elements")
    idx = [int(b) for b in selected_bands]
    for band in idx:
        if band >= shp[2] or band < 0:
            raise IndexError(f"Band index {band} out of range. Available bands indices: 0 to {shp[2] - 1}.")
    if mask is not None and _image._shape(mask) != shp[:2]:
        raise ValueError(f"the mask is {_image._shape(mask)}, the raster {shp[0]} x {shp[1]}")
    windows, tile_transforms = tile_windows(shp, affine_transformation, tile_size, overlap)
    names = [f"img_{i + 1:03d}.jpg" for i in range(len(windows))]
    for (_, _, h, w), tile_name in zip(windows, names):
        s.check_tile(h, w, tile_name, mask is not None)
    bounds = _bounds_table(boxes)
    transforms = {n: {"transform": t, "crs": str(crs)} for n, t in zip(names, tile_transforms)}
    annotations = tile_annotations(bounds, affine_transformation, windows, names) if bounds is not None else None

    dev = _device.device_of(ctx, raster, mask)
    if _device.is_torch(raster):
        src = raster.to(device=f"cuda:{dev}")
    else:
        src, idx = torch.as_tensor(np.ascontiguousarray(np.asarray(raster)[:, :, idx]), device=f"cuda:{dev}"), [0, 1, 2]
    m_all = _mask_u8(mask, dev) if mask is not None else None
    tables = _Tables(s, src.device, m_all is not None)
    counters = torch.zeros((len(windows), 2), dtype=torch.int64, device=src.device)
    lib, c = _device.begin(dev, ctx)
    stream = torch.cuda.current_stream(dev)
    images, keep, held = [], [], 0
    for i, (r0, c0, h, w) in enumerate(windows):
        x = src[r0:r0 + h, c0:c0 + w][:, :, idx].contiguous()
        m = inv = None
        if m_all is not None:
            m = m_all[r0:r0 + h, c0:c0 + w].contiguous()
            inv = (255 - m * 255) if s.feather > 0.0 else None
        stream.synchronize()         # the tile torch has just cut out is complete before the context's stream reads it
        try:
            images.append(_tile_dev(lib, c, s, tables, x, m, inv, counters[i], keep))
        except ValueError as e:
            _device.end(lib, c)
            raise ValueError(f"{names[i]}: {e}") from None
        held += 40 * h * w           # bytes of a tile's temporaries, roughly
        if held > _KEEP_BYTES:
            _device.end(lib, c)
            keep, held = [], 0
    _device.end(lib, c)
    del keep
    _raise_counters(counters.cpu().numpy(), names)
    if not as_array:
        images = [t.cpu().numpy() for t in images]
    if output_dir is not None:
        from PIL.Image import fromarray
        os.makedirs(output_dir, exist_ok=True)
        for tile_name, img in zip(names, images):
            fromarray(img.cpu().numpy() if _device.is_torch(img) else img).save(os.path.join(output_dir, tile_name), format="JPEG")
        if annotations is not None:
            with open(os.path.join(output_dir, "annotations.json"), "w") as f:
                json.dump(annotations, f, indent=2)
        with open(os.path.join(output_dir, "transforms.json"), "w") as f:
            json.dump(transforms, f, indent=2)
    return TrainingTiles(names, images, transforms, annotations, windows)
