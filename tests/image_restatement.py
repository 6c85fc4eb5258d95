"""Plain-NumPy restatement of the image-preview path (test helper, not a conftest): the CPU reference of tests/test_gpu_image.py.

  * rescale_to_8bit                : the reference's three NumPy expressions (obia/utils/image.py:27-36), evaluated literally.
  * find_boundaries / mark_u8      : scikit-image 0.18.3 (segmentation/boundaries.py:159-177, mark_boundaries) -- pinned to the
                                     library itself by the goldens of tests/golden/boundaries/ (tests/test_image_cpu.py).
  * rgb_to_gray / equalize_hist / clahe : OpenCV's algorithms (color conversion RGB2GRAY of 8-bit images, equalizeHist, clahe.cpp)
                                     written down from their description.  They are NOT compared with cv2 anywhere: OpenCV is not
                                     installed where the tests run.  Float arithmetic is float32 throughout, multiply and add separate.
"""
import numpy as np

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- stretch
def rescale_to_8bit(image, min=2, max=98):
    image = np.asarray(image)
    p_min, p_max = np.percentile(image, (min, max))
    if p_min == p_max:
        return np.zeros(image.shape, dtype=np.uint8)
    scaled_image = 255 * (image - p_min) / (p_max - p_min)
    scaled_image = np.clip(scaled_image, 0, 255)
    return scaled_image.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- boundaries
def _shifted(a, dy, dx):
    """a[y + dy, x + dx] with coordinates clamped to the raster: a neighbour outside it becomes a copy of a pixel that is inside the
    same window, which changes neither a maximum nor a minimum over the window (what ndimage's "reflect" does for a 3 x 3 window)"""
    H, W = a.shape
    ys = np.clip(np.arange(H) + dy, 0, H - 1)
    xs = np.clip(np.arange(W) + dx, 0, W - 1)
    return a[np.ix_(ys, xs)]


S4 = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))
S8 = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))


def _dilate(a, taps):
    return np.max([_shifted(a, dy, dx) for dy, dx in taps], axis=0)


def _erode(a, taps):
    return np.min([_shifted(a, dy, dx) for dy, dx in taps], axis=0)


def find_boundaries(labels):
    """mode="outer", connectivity 1, background 0 -> bool (H, W)"""
    L = np.asarray(labels)
    b = _dilate(L, S4) != _erode(L, S4)
    bg = L == 0
    Lp = L.copy()
    Lp[bg] = np.iinfo(L.dtype).max
    adj = (_dilate(L, S8) != _erode(Lp, S8)) & ~bg
    return b & (bg | adj)


def mark_table():
    """(img_as_float(v) * 255).astype(uint8) for v = 0 .. 255: scikit-image multiplies by 1 / 255 in float64"""
    v = np.multiply(np.arange(256, dtype=np.uint8), 1.0 / 255, dtype=np.float64)
    return (v * 255).astype(np.uint8)


def mark_u8(image, labels, color=(255, 255, 0)):
    """(mark_boundaries(image, labels) * 255).astype(uint8) of a uint8 (H, W) or (H, W, 3) image"""
    image = np.asarray(image)
    if image.ndim == 2:
        image = np.stack((image,) * 3, axis=-1)
    out = mark_table()[image]
    out[find_boundaries(labels)] = np.asarray(color, np.uint8)
    return out


# -------------------------------------------------------------------------------------------------------------- grey, equalize
def rgb_to_gray(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    return ((9798 * r + 19235 * g + 3735 * b + 16384) >> 15).astype(np.uint8)


def _saturate_u8(x_f32):
    """saturate_cast<uchar>(float): round half to even, then clamp"""
    return np.clip(np.rint(x_f32), 0, 255).astype(np.uint8)


def equalize_lut(hist):
    """the table of equalizeHist, or None when the first non-empty bin holds every pixel"""
    hist = [int(h) for h in hist]
    total = sum(hist)
    i = 0
    while not hist[i]:
        i += 1
    if hist[i] == total:
        return None
    scale = F32(255.0) / F32(total - hist[i])
    lut = np.zeros(256, np.uint8)
    s = 0
    for j in range(i + 1, 256):
        s += hist[j]
        lut[j] = _saturate_u8(F32(s) * scale)
    return lut


def equalize_hist(gray):
    lut = equalize_lut(np.bincount(gray.ravel(), minlength=256))
    return gray.copy() if lut is None else lut[gray]


def apply_histogram_equalization(image):
    image = np.asarray(image)
    gray = rgb_to_gray(image) if image.ndim == 3 else image
    return np.stack((equalize_hist(gray),) * 3, axis=-1)


# ------------------------------------------------------------------------------------------------------------------ CLAHE
def reflect101(p, n):
    """borderInterpolate(p, n, BORDER_REFLECT_101)"""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def clahe_geometry(H, W):
    """(padded H, padded W, tile height, tile width, clip, lutScale)"""
    if W % 8 == 0 and H % 8 == 0:
        ph, pw = H, W
    else:
        ph, pw = H + 8 - H % 8, W + 8 - W % 8
    th, tw = ph // 8, pw // 8
    area = th * tw
    clip = max(int(2.0 * area / 256), 1)
    return ph, pw, th, tw, clip, F32(255.0) / F32(area)


def clahe_tile_lut(hist, clip, lut_scale):
    hist = [int(h) for h in hist]
    excess = 0
    for i in range(256):
        if hist[i] > clip:
            excess += hist[i] - clip
            hist[i] = clip
    batch, residual = excess // 256, excess % 256
    for i in range(256):
        hist[i] += batch
    if residual:
        step = max(256 // residual, 1)
        i = 0
        while i < 256 and residual > 0:
            hist[i] += 1
            i += step
            residual -= 1
    lut = np.zeros(256, np.uint8)
    s = 0
    for i in range(256):
        s += hist[i]
        lut[i] = _saturate_u8(F32(s) * lut_scale)
    return lut


def clahe_luts(plane):
    """(8, 8, 256) tables of one uint8 plane, and the tile size"""
    H, W = plane.shape
    ph, pw, th, tw, clip, lut_scale = clahe_geometry(H, W)
    ys = [reflect101(y, H) for y in range(ph)]
    xs = [reflect101(x, W) for x in range(pw)]
    padded = plane[np.ix_(ys, xs)]
    luts = np.zeros((8, 8, 256), np.uint8)
    for ty in range(8):
        for tx in range(8):
            tile = padded[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            luts[ty, tx] = clahe_tile_lut(np.bincount(tile.ravel(), minlength=256), clip, lut_scale)
    return luts, th, tw


def _axis_weights(n, t):
    """per coordinate: (first tile, second tile, weight of the first, weight of the second), the tiles clamped AFTER the weights"""
    inv = F32(1.0) / F32(t)
    f = np.arange(n).astype(F32) * inv - F32(0.5)
    t1 = np.floor(f).astype(np.int64)
    a = (f - t1.astype(F32)).astype(F32)
    a1 = (F32(1.0) - a).astype(F32)
    return np.maximum(t1, 0), np.minimum(t1 + 1, 7), a1, a


def clahe_plane(plane):
    plane = np.asarray(plane)
    H, W = plane.shape
    luts, th, tw = clahe_luts(plane)
    ty1, ty2, ya1, ya = (v[:, None] for v in _axis_weights(H, th))
    tx1, tx2, xa1, xa = (v[None, :] for v in _axis_weights(W, tw))
    l11 = luts[ty1, tx1, plane].astype(F32)
    l12 = luts[ty1, tx2, plane].astype(F32)
    l21 = luts[ty2, tx1, plane].astype(F32)
    l22 = luts[ty2, tx2, plane].astype(F32)
    top = (l11 * xa1).astype(F32) + (l12 * xa).astype(F32)
    bot = (l21 * xa1).astype(F32) + (l22 * xa).astype(F32)
    res = (top * ya1).astype(F32) + (bot * ya).astype(F32)
    return _saturate_u8(res)


def apply_clahe(image):
    image = np.asarray(image)
    if image.ndim == 3:
        return np.stack([clahe_plane(image[..., c]) for c in range(image.shape[2])], axis=-1)
    return clahe_plane(image)
