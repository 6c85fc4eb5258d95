"""The sharpness raster of the reference (obia/utils/image.py:97-136) restated in NumPy alone (test helper, not a conftest): the
per-band normalisation and ``rgb_to_gray``, ``cv2.Laplacian(gray, CV_32F, ksize=3)``, ``scipy.ndimage.uniform_filter`` on a float32
plane, ``variance_of_laplacian`` and the percentile stretch.  No SciPy and no OpenCV: the box filter is checked bit for bit against
SciPy 1.15.3 through tests/golden/sharpness/*.npz (tests/test_sharpness_cpu.py); the Laplacian is OpenCV's algorithm restated (filter2D
with [[2, 0, 2], [0, -8, 0], [2, 0, 2]], BORDER_REFLECT_101, float32 accumulation over the non-zero taps in row-major order) and is NOT
compared with cv2 anywhere.

The box filter walks every line sample by sample in SciPy's order (the loop below runs along the line; all lines of the plane take
each step together, which does not change any line's own arithmetic)."""
import numpy as np

COEFFS = np.array([0.299, 0.587, 0.114], dtype=np.float32)


def normalise_bands(arr):
    """(H, W, 3) float32 -> each band (x - min) / ((max - min) + 1e-8) in float32 (image.py:120-122); a constant band gives zeros"""
    arr = np.asarray(arr, np.float32)
    mn = arr.min(axis=(0, 1), keepdims=True)
    rng = (arr.max(axis=(0, 1), keepdims=True) - mn) + np.float32(1e-8)
    return (arr - mn) / rng


def rgb_to_gray(rgb):
    """(rgb * coeffs).sum(axis=-1) for three elements: every product rounded to float32, the sum from the left"""
    rgb = np.asarray(rgb, np.float32)
    return (rgb[..., 0] * COEFFS[0] + rgb[..., 1] * COEFFS[1]) + rgb[..., 2] * COEFFS[2]


def reflect101(p, n):
    """BORDER_REFLECT_101 for p in [-1, n]"""
    if n == 1:
        return 0
    if p < 0:
        return -p
    if p >= n:
        return 2 * (n - 1) - p
    return p


def laplacian3(gray):
    """cv2.Laplacian(gray, cv2.CV_32F, ksize=3): ((((2 a + 2 b) + (-8 c)) + 2 d) + 2 e), a b the upper-left and upper-right
    neighbours, c the centre, d e the lower-left and lower-right"""
    g = np.asarray(gray, np.float32)
    H, W = g.shape
    ys = np.array([reflect101(y, H) for y in range(-1, H + 1)])
    xs = np.array([reflect101(x, W) for x in range(-1, W + 1)])
    p = g[np.ix_(ys, xs)]                                              # (H + 2, W + 2)
    a, b, c, d, e = p[:-2, :-2], p[:-2, 2:], p[1:-1, 1:-1], p[2:, :-2], p[2:, 2:]
    two, m8 = np.float32(2), np.float32(-8)
    return (((two * a + two * b) + m8 * c) + two * d) + two * e


def reflect_sym(i, n):
    """SciPy's mode "reflect" (d c b a | a b c d | d c b a): period 2 n"""
    m = i % (2 * n)
    return m if m < n else 2 * n - 1 - m


def uniform_filter1d(plane, win, axis):
    """scipy.ndimage.uniform_filter1d(plane, win, axis) for a float32 plane, float32 out: the running sum in double"""
    x = np.moveaxis(np.asarray(plane, np.float32), axis, 0).astype(np.float64)      # x[i]: sample i of every line
    n = x.shape[0]
    s1 = win // 2
    s2 = win - s1 - 1
    out = np.empty(x.shape, np.float32)
    tmp = np.zeros(x.shape[1:], np.float64)
    for l in range(-s1, s2 + 1):
        tmp = tmp + x[reflect_sym(l, n)]
    out[0] = (tmp / win).astype(np.float32)
    for ll in range(1, n):
        tmp = tmp + (x[reflect_sym(ll + s2, n)] - x[reflect_sym(ll - s1 - 1, n)])
        out[ll] = (tmp / win).astype(np.float32)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def box_filter(plane, win):
    """scipy.ndimage.uniform_filter(plane.astype(float32), size=win): axis 0 into a float32 plane, axis 1 from there; SciPy skips
    an axis whose size is 1, so win = 1 is a copy"""
    p = np.asarray(plane).astype(np.float32)
    if win == 1:
        return p.copy()
    return uniform_filter1d(uniform_filter1d(p, win, 0), win, 1)


def variance_of_laplacian(gray, win):
    lap = laplacian3(gray)
    mean = box_filter(lap, win)
    mean2 = box_filter(lap * lap, win)
    return mean2 - mean * mean


def stretch(sharp):
    """image.py:130-131 and the cast of :136"""
    lo, hi = np.percentile(sharp, [2, 98])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.clip((sharp - lo) / (hi - lo), 0, 1).astype(np.float32)


def laplacian(image, win, bands=(1, 2, 4)):
    """obia.utils.image.laplacian between its read and its write, on an (H, W, C) array"""
    arr = np.asarray(image)[:, :, list(bands)].astype(np.float32)
    return stretch(variance_of_laplacian(rgb_to_gray(normalise_bands(arr)), win))


def golden_plane(data, shape):
    """the planes of tests/golden/sharpness (gen_goldens_sharpness.py): "n50" standard_normal * 50, "wide" standard_normal *
    10.0 ** randint(-12, 13), both from RandomState(1)"""
    rs = np.random.RandomState(1)
    if data == "n50":
        return (rs.standard_normal(shape) * 50).astype(np.float32)
    return (rs.standard_normal(shape) * 10.0 ** rs.randint(-12, 13, shape)).astype(np.float32)


def bits(a):
    """float32 array as its bit patterns: NaNs compare"""
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)
