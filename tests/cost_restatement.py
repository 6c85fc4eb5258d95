"""CPU restatement of obia/utils/cost.py (TEST INFRASTRUCTURE ONLY): the formulas of ``normalise``, ``chm_gradient``,
``ndvi``, ``texture_entropy``, ``slic_edge`` and ``make_cost_surface`` evaluated with NumPy >= 2 and SciPy, which are
installed here.  scikit-image is not, so its rank entropy over disk(3) is restated: the histogram of the taps inside
the raster, then e -= p * log(p) / ln 2 over the grey levels in ascending order, with the terms from libm ``log``
(``math.log``).  ``percentiles`` restates np.nanpercentile's linear method from the sorted values, so that the way the
GPU path interpolates its order statistics is pinned against NumPy on its own."""
import math

import numpy as np
from scipy.ndimage import sobel

LN2 = 0.6931471805599453
Q = np.true_divide((2, 98), 100.0)

# disk(3): x^2 + y^2 <= 9, 29 taps
DISK3 = [(dy, dx) for dy in range(-3, 4) for dx in range(-3, 4) if dy * dy + dx * dx <= 9]
assert len(DISK3) == 29


def percentiles(arr, q=Q):
    """np.nanpercentile(arr, 100 * q) (method "linear") from the sorted non-NaN values: virtual index (n - 1) * q, its floor
    and the next index (both the last one at or past n - 1), weight = index - floor, then NumPy's _lerp: b - a in the
    input dtype, a + diff * t in float64, b - diff * (1 - t) where t >= 0.5."""
    a = np.asarray(arr).ravel()
    v = np.sort(a[~np.isnan(a)])
    n = v.size
    q = np.asarray(q, np.float64)
    if n == 0:
        return np.full(q.shape, np.nan, a.dtype)
    vi = (n - 1) * q
    prev = np.floor(vi)
    above = vi >= n - 1
    prev[above] = -1
    nxt = prev + 1
    nxt[above] = -1
    prev_i, nxt_i = prev.astype(np.intp), nxt.astype(np.intp)
    t = vi - prev_i
    lo, hi = v[prev_i], v[nxt_i]
    diff = hi - lo
    out = lo + diff * t
    out = np.where(t >= 0.5, hi - diff * (1 - t), out)
    return out


def normalise(arr):
    lo, hi = np.nanpercentile(arr, (2, 98))
    arr_clip = np.clip(arr, lo, hi)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (arr_clip - lo) / (hi - lo)
    return np.nan_to_num(out)


def hypot_plane(chm):
    chm = np.asarray(chm, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = sobel(chm, axis=1, mode="nearest")
        dy = sobel(chm, axis=0, mode="nearest")
        return np.hypot(dx, dy)


def chm_gradient(chm):
    return normalise(hypot_plane(chm))


def ndvi(red, nir):
    with np.errstate(all="ignore"):
        return np.clip((nir - red) / (nir + red + 1e-9), -1, 1)


def term_table():
    """T[pop][c] = (c / pop) * log(c / pop) / ln 2 (libm log); column 0 = 0."""
    t = np.zeros((30, 32), np.float64)
    for pop in range(1, 30):
        for c in range(1, pop + 1):
            p = c / pop
            t[pop, c] = p * math.log(p) / LN2
    return t


def rank_entropy(u8, rows=256):
    """skimage.filters.rank.entropy(u8, disk(3)), float64, vectorised: the 29 taps of every pixel (256 outside the raster),
    sorted, and the runs of equal grey levels walked in ascending order."""
    u8 = np.asarray(u8, np.uint8)
    H, W = u8.shape
    T = term_table()
    pad = np.full((H + 6, W + 6), 256, np.int16)
    pad[3:H + 3, 3:W + 3] = u8
    out = np.empty((H, W), np.float64)
    for y0 in range(0, H, rows):
        y1 = min(H, y0 + rows)
        taps = np.stack([pad[y0 + 3 + dy:y1 + 3 + dy, 3 + dx:W + 3 + dx] for dy, dx in DISK3])
        pop = (taps < 256).sum(0)
        s = np.sort(taps, axis=0)
        e = np.zeros(pop.shape, np.float64)
        run = np.ones(pop.shape, np.int64)
        for i in range(29):
            end = (s[i + 1] != s[i]) if i < 28 else np.ones(pop.shape, bool)
            hit = end & (s[i] < 256)
            e = np.where(hit, e - T[pop, np.where(hit, run, 0)], e)
            run = np.where(end, 1, run + 1)
        out[y0:y1] = e
    return out


def rank_entropy_loop(u8):
    """The same, pixel by pixel and straight from the definition (small images only)."""
    u8 = np.asarray(u8, np.uint8)
    H, W = u8.shape
    out = np.zeros((H, W), np.float64)
    for y in range(H):
        for x in range(W):
            hist = np.zeros(256, np.int64)
            for dy, dx in DISK3:
                if 0 <= y + dy < H and 0 <= x + dx < W:
                    hist[u8[y + dy, x + dx]] += 1
            pop = float(hist.sum())
            e = 0.0
            for i in range(256):
                p = hist[i] / pop
                if p > 0:
                    e -= p * math.log(p) / LN2
            out[y, x] = e
    return out


def quantise(pan):
    return (normalise(pan) * 255).astype(np.uint8)


def texture_entropy(pan, raw=False):
    e = rank_entropy(quantise(pan))
    return e if raw else normalise(e)


def slic_edge(label_img):
    edge = np.zeros_like(label_img, dtype=np.uint8)
    edge[:-1, :] |= label_img[:-1, :] != label_img[1:, :]
    edge[:, :-1] |= label_img[:, :-1] != label_img[:, 1:]
    return normalise(edge.astype(np.float32))


def make_cost_surface(wv3, chm, slic=None, weights=(0.5, 0.25, 0.25, 0)):
    """The surface of make_cost_surface for arrays: wv3 (H, W, 8), chm (H, W), slic a label raster or None."""
    w_grad, w_gap, w_tex, w_slic = weights
    if abs(sum(weights) - 1) > 1e-6:
        raise SystemExit("Weights must sum to 1.")
    wv3 = np.asarray(wv3).astype(np.float32)
    C, R, N1 = wv3[:, :, 0], wv3[:, :, 4], wv3[:, :, 6]
    grad = chm_gradient(np.asarray(chm, np.float32))
    gap = normalise(1 - ndvi(R, N1))
    tex = texture_entropy(C)
    if slic is not None:
        edge = slic_edge(np.asarray(slic))
    else:
        edge = 0.0
        s = w_grad + w_gap + w_tex
        w_grad, w_gap, w_tex, w_slic = (w_grad / s, w_gap / s, w_tex / s, 0.0)
    cost = (w_grad * grad + w_gap * gap + w_tex * tex + w_slic * edge)
    cost = np.clip(cost, 0, 1).astype(np.float32)
    cost[np.isnan(cost)] = -9999.0
    return cost
