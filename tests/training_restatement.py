"""obia.utils.training.tile_and_process (training.py:16-338) restated in NumPy, written plainly rather than fast (test helper, not a
conftest): what tests/test_training_restatement_cpu.py pins on things outside it and tests/test_gpu_training.py compares the kernels
with, bit for bit.

  * blur_u8: cv2.GaussianBlur(src, (kx, ky), 0) on uint8 as integer arithmetic -- 8.8 fixed-point weights per axis, the horizontal pass
    kept exact, one rounding after the vertical pass -- with BORDER_REFLECT_101 applied index by index, repeatedly;
  * chamfer_sweep: cv2.distanceTransform(src, DIST_L2, 3) as OpenCV's two-pass 3 x 3 sweep over a plane with a border of DIST_MAX --
    deliberately NOT the closed form the kernels evaluate; chamfer_closed_form is that closed form by brute force over the zero pixels,
    with or without a window;
  * darken, blend_hard, blend_feather, minmax_u8: the reference's NumPy expressions;
  * generate_tiles, windows, annotations: the reference's loops, the float window rounded to integers;
  * process_tile / tile_and_process composed from these and tests/image_restatement.py's rescale_to_8bit and apply_clahe.

OpenCV's operators are restated from its algorithm and NOT compared with cv2 anywhere: it is not installed where the tests run."""
import functools
import math

import numpy as np

from tests import image_restatement as IR

HV, DG, DIST_MAX = 62587, 89738, (2 ** 31 - 1) >> 2
SMALL = {1: [256], 3: [64, 128, 64], 5: [16, 64, 96, 64, 16], 7: [8, 28, 56, 72, 56, 28, 8]}


# ---- blur ------------------------------------------------------------------------------------------------------------------------
def gaussian_weights(k):
    if k in SMALL:
        return np.array(SMALL[k], np.int64)
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    g = np.array([math.exp(-((i - (k - 1) * 0.5) ** 2) / (2 * sigma * sigma)) for i in range(k)], np.float64)
    g = g / g.sum()
    w = [0] * k
    err = 0.0
    for i in range(k // 2):
        v = 256 * g[i] + err
        q = math.floor(v + 0.5)
        err = v - q
        w[i] = w[k - 1 - i] = int(q)
    w[k // 2] = 256 - sum(w)
    return np.array(w, np.int64)


def reflect101(p, n):
    """BORDER_REFLECT_101, applied until the index lies in the line; a line of one reads index 0"""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def blur_u8(img, ksize):
    kx, ky = (ksize, ksize) if isinstance(ksize, int) else ksize
    if (kx, ky) == (0, 0):
        return img
    wx, wy = gaussian_weights(kx), gaussian_weights(ky)
    p = img.astype(np.int64)
    H, W = p.shape[:2]
    hor = np.zeros_like(p)
    for t in range(kx):
        cols = [reflect101(x + t - kx // 2, W) for x in range(W)]
        hor += wx[t] * p[:, cols]
    assert hor.max() <= 255 * 256
    tot = np.zeros_like(p)
    for t in range(ky):
        rows = [reflect101(y + t - ky // 2, H) for y in range(H)]
        tot += wy[t] * hor[rows]
    return ((tot + 32768) >> 16).astype(np.uint8)


# ---- distance --------------------------------------------------------------------------------------------------------------------
def chamfer_sweep_fixed(src):
    """the integers of OpenCV's distanceTransform_3x3 before the scaling: forward pass, backward pass, the cap"""
    H, W = src.shape
    tmp = [[DIST_MAX] * (W + 2) for _ in range(H + 2)]               # a border of one pixel on every side
    for i in range(1, H + 1):
        row, up = tmp[i], tmp[i - 1]
        for j in range(1, W + 1):
            if src[i - 1, j - 1] == 0:
                row[j] = 0
            else:
                row[j] = min(up[j - 1] + DG, up[j] + HV, up[j + 1] + DG, row[j - 1] + HV)
    out = np.zeros((H, W), np.int64)
    for i in range(H, 0, -1):
        row, down = tmp[i], tmp[i + 1]
        for j in range(W, 0, -1):
            t0 = row[j]
            if t0 > HV:
                t0 = min(t0, down[j + 1] + DG, down[j] + HV, down[j - 1] + DG, row[j + 1] + HV)
                row[j] = t0
            out[i - 1, j - 1] = min(t0, DIST_MAX)
    return out


def to_float(t):
    """OpenCV's (float)t * (1.f / 65536)"""
    return t.astype(np.float32) * np.float32(1.0 / 65536.0)


def chamfer_sweep(src):
    return to_float(chamfer_sweep_fixed(src))


def chamfer_closed_form_fixed(src, R=None):
    """min over the zero pixels (within Chebyshev distance R, when given) of HV * (max - min) + DG * min of |dx|, |dy|; DIST_MAX when
    there is none"""
    H, W = src.shape
    zy, zx = np.nonzero(src == 0)
    out = np.full((H, W), DIST_MAX, np.int64)
    for y in range(H):
        for x in range(W):
            ady, adx = np.abs(zy - y), np.abs(zx - x)
            if R is not None:
                near = np.maximum(ady, adx) <= R
                ady, adx = ady[near], adx[near]
            if len(ady):
                mx, mn = np.maximum(ady, adx), np.minimum(ady, adx)
                out[y, x] = int((HV * (mx - mn) + DG * mn).min())
    return out


def chamfer_windowed(src, R):
    return to_float(chamfer_closed_form_fixed(src, R))


# ---- darkening, blends, min-max --------------------------------------------------------------------------------------------------
def darken(blurred, darken_factor):
    if darken_factor == 0:
        return blurred
    return (blurred * darken_factor).astype(np.uint8)


def blend_hard(tile, background, mask):
    mask_3d = np.stack([mask] * 3, axis=-1)
    return (tile * mask_3d + background * (1 - mask_3d)).astype(np.uint8)


def blend_feather(tile, background, dist, feather_radius):
    alpha = 1.0 - (dist / feather_radius)
    alpha = np.clip(alpha, 0.0, 1.0)
    alpha_3d = np.dstack([alpha] * 3)
    assert alpha_3d.dtype == np.float32
    out = alpha_3d * tile.astype(np.float32) + (1.0 - alpha_3d) * background.astype(np.float32)
    assert out.dtype == np.float32
    return np.clip(out, 0, 255).astype(np.uint8)


def minmax_u8(tile):
    tile_min, tile_max = tile.min(), tile.max()
    if tile_min == tile_max:
        out = np.zeros_like(tile, dtype=np.uint8)
    else:
        out = 255 * (tile - tile_min) / (tile_max - tile_min)
        assert out.dtype == np.float32
    return np.clip(out, 0, 255).astype(np.uint8)


# ---- one tile --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _stretched(tile_bytes, shape, rescale, apply_clahe_flag):
    """step (2) of a float32 tile; kept, so that the variants of a test that differ only in step (3) compute it once"""
    tile = np.frombuffer(tile_bytes, np.float32).reshape(shape)
    u8 = IR.rescale_to_8bit(tile) if rescale else minmax_u8(tile)
    return np.dstack([IR.apply_clahe(u8[:, :, ch]) for ch in range(3)]) if apply_clahe_flag else u8


def process_tile(tile, mask=None, feather_radius=0.0, blur_kernel=5, darken_factor=0.8, apply_clahe_flag=True, rescale=True):
    final = _stretched(tile.tobytes(), tile.shape, bool(rescale), bool(apply_clahe_flag))
    if mask is None:
        return final
    background = darken(blur_u8(final, blur_kernel), darken_factor)
    if feather_radius > 0:
        mask_8u = (mask * 255).astype(np.uint8)
        return blend_feather(final, background, chamfer_sweep(255 - mask_8u), feather_radius)
    return blend_hard(final, background, mask.astype(np.uint8))


# ---- tiling ----------------------------------------------------------------------------------------------------------------------
def generate_tiles(bounds, step, tile_size):
    minx, miny, maxx, maxy = bounds
    y = miny
    while y < maxy:
        x = minx
        tile_top = y + tile_size
        while x < maxx:
            tile_right = x + tile_size
            yield (x, y, min(tile_right, maxx), min(tile_top, maxy))
            x += step
        y += step


def float_windows(shape, affine, tile_size, overlap):
    """(box, (row_off, col_off, height, width) as floats) per tile: rasterio.windows.from_bounds for a north-up transform
    [a, b, d, e, xoff, yoff]"""
    a, _, _, e, xoff, yoff = affine
    H, W = shape[:2]
    bounds = (xoff, yoff + e * H, xoff + a * W, yoff)
    out = []
    for box in generate_tiles(bounds, tile_size - overlap, tile_size):
        minx, miny, maxx, maxy = box
        out.append((box, ((maxy - yoff) / e, (minx - xoff) / a, (miny - maxy) / e, (maxx - minx) / a)))
    return out


def windows(shape, affine, tile_size, overlap):
    """integer windows and [a, b, c, d, e, f] transforms; every float window must be whole"""
    a, b, d, e, xoff, yoff = affine
    wins, transforms = [], []
    for _, fw in float_windows(shape, affine, tile_size, overlap):
        iw = tuple(int(round(v)) for v in fw)
        assert all(abs(v - i) < 1e-6 for v, i in zip(fw, iw)), fw
        wins.append(iw)
        transforms.append([a, b, a * iw[1] + b * iw[0] + xoff, d, e, d * iw[1] + e * iw[0] + yoff])
    return wins, transforms


def rowcol(affine, x, y):
    """rasterio.transform.rowcol: floor of ~Affine * (x, y), the inverse as the affine package computes it"""
    a, b, d, e, xoff, yoff = affine
    idet = 1.0 / (a * e - b * d)
    ra, rb, rd, re = e * idet, -b * idet, -d * idet, a * idet
    col = x * ra + y * rb + (-xoff * ra - yoff * rb)
    row = x * rd + y * re + (-xoff * rd - yoff * re)
    return math.floor(row), math.floor(col)


def annotations(bounds, shape, affine, tile_size, overlap):
    """the reference's loop (training.py:139-145, 267-318) on polygon bounds: a polygon lies within a tile when its bounds do"""
    wins, _ = windows(shape, affine, tile_size, overlap)
    out = {}
    for index, ((box, _), (row_off, col_off, out_height, out_width)) in enumerate(zip(float_windows(shape, affine, tile_size, overlap), wins), 1):
        minx, miny, maxx, maxy = box
        inside = [p for p in bounds if p[0] >= minx and p[1] >= miny and p[2] <= maxx and p[3] <= maxy]
        if not inside:
            continue
        boxes_array, labels_array = [], []
        for pxmin, pymin, pxmax, pymax in inside:
            row_tl, col_tl = rowcol(affine, pxmin, pymax)
            row_br, col_br = rowcol(affine, pxmax, pymin)
            x_min_pix = max(0, min(col_tl - col_off, out_width - 1))
            x_max_pix = max(0, min(col_br - col_off, out_width - 1))
            y_min_pix = max(0, min(row_tl - row_off, out_height - 1))
            y_max_pix = max(0, min(row_br - row_off, out_height - 1))
            if x_min_pix >= x_max_pix or y_min_pix >= y_max_pix:
                continue
            boxes_array.append([x_min_pix, y_min_pix, x_max_pix, y_max_pix])
            labels_array.append(1)
        out[f"img_{index:03d}"] = {"file_name": f"img_{index:03d}.jpg", "boxes": boxes_array, "labels": labels_array}
    return out


def tile_and_process(raster, affine, crs, mask=None, bounds=None, tile_size=150.0, overlap=50.0, selected_bands=(4, 2, 1), **kw):
    """(names, images, transforms, annotations or None)"""
    wins, tile_transforms = windows(raster.shape, affine, tile_size, overlap)
    names, images, transforms = [], [], {}
    for index, ((r0, c0, h, w), t) in enumerate(zip(wins, tile_transforms), 1):
        name = f"img_{index:03d}.jpg"
        tile = np.ascontiguousarray(raster[r0:r0 + h, c0:c0 + w][:, :, list(selected_bands)])
        m = mask[r0:r0 + h, c0:c0 + w] if mask is not None else None
        names.append(name)
        images.append(process_tile(tile, m, **kw))
        transforms[name] = {"transform": t, "crs": str(crs)}
    return names, images, transforms, (annotations(bounds, raster.shape, affine, tile_size, overlap) if bounds is not None else None)
