"""obia/utils/seeds.py restated with NumPy + SciPy only (test infrastructure): the expressions of _detect_chm_peaks /
_detect_den_peaks (seeds.py:11-35), _build_distance_matrix (seeds.py:139-165) and what make_canonical_seeds does with the
matrix (seeds.py:224-231), written as the reference writes them and evaluated under NumPy >= 2 promotion.  rasterio's
``rowcol(tfm, xs, ys, op=float)`` is the inverse affine applied as the affine package does, ``(x * a + y * b) + c``; DBSCAN with
``min_samples=1`` on a precomputed matrix is the connected components of ``D <= eps`` numbered by first member
(tests/test_seeds_restatement_cpu.py checks that against scikit-learn)."""
import math

import numpy as np
from scipy.ndimage import gaussian_filter, maximum_filter
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components


# ---------------------------------------------------------------------------------------------------------------- peaks
def smooth(arr, sigma):
    return gaussian_filter(arr, sigma=sigma) if sigma > 0 else arr


def peaks_scipy(arr, v_min, min_dist_px, sigma=0):
    """_detect_chm_peaks, literally: the boolean peak plane (np.where of it is the reference's list)."""
    arr = smooth(arr, sigma)
    local_max = (arr == maximum_filter(arr, size=2 * min_dist_px + 1))
    return np.logical_and(local_max, arr >= v_min)


def peaks_nan_rule(arr, v_min, min_dist_px, sigma=0):
    """The same with obia_amd's NaN rule: a NaN never wins the maximum (it counts as -inf) and a NaN pixel is never a peak."""
    arr = smooth(arr, sigma)
    nan = np.isnan(arr)
    mx = maximum_filter(np.where(nan, np.float32(-np.inf), arr), size=2 * min_dist_px + 1)
    return ~nan & (arr == mx) & (arr >= v_min)


def nan_free_window(arr, min_dist_px, sigma=0):
    """Pixels whose (2d+1)^2 window of the smoothed plane (reflect borders) holds no NaN."""
    nan = np.isnan(smooth(arr, sigma)).astype(np.uint8)
    return maximum_filter(nan, size=2 * min_dist_px + 1) == 0


# ------------------------------------------------------------------------------------------------------------- distance
def line_ts(samples):
    return np.linspace(0.0, 1.0, samples + 2, dtype=np.float32)[1:-1]


def rowcol_float(inv6, xs, ys):
    """rowcol(tfm, xs, ys, op=float): (rows, cols) = ~tfm * (x, y) in float64; inv6 = (a, b, c, d, e, f) of ~tfm."""
    a, b, c, d, e, f = inv6
    return xs * d + ys * e + f, xs * a + ys * b + c


def distance_matrix_loop(xs, ys, cost, inv6, weight, xy_thresh, samples=8):
    """_build_distance_matrix (seeds.py:139-165), line for line."""
    n = len(xs)
    D = np.zeros((n, n), np.float32)
    for i in range(n):
        xi, yi = xs[i], ys[i]
        for j in range(i + 1, n):
            dx, dy = xs[j] - xi, ys[j] - yi
            xy_dist = math.hypot(dx, dy)
            if xy_dist == 0:
                continue
            if xy_dist <= xy_thresh or weight == 0:
                D[i, j] = D[j, i] = xy_dist
                continue
            ts = np.linspace(0.0, 1.0, samples + 2, dtype=np.float32)[1:-1]
            xs_line = xi + ts * dx
            ys_line = yi + ts * dy
            rows, cols = rowcol_float(inv6, xs_line, ys_line)
            with np.errstate(invalid="ignore"):
                rows = np.clip(rows.round().astype(int), 0, cost.shape[0] - 1)
                cols = np.clip(cols.round().astype(int), 0, cost.shape[1] - 1)
            mean_cost = cost[rows, cols].mean()
            D[i, j] = D[j, i] = xy_dist * (1.0 + weight * mean_cost)
    return D


def hypot_py(dx, dy):
    """math.hypot element by element (CPython's own algorithm: np.hypot calls libm's and differs from it in the last bit)."""
    return np.fromiter(map(math.hypot, dx.tolist(), dy.tolist()), np.float64, len(dx))


def distance_matrix(xs, ys, cost, inv6, weight, xy_thresh, samples=8):
    """The same matrix, one row of pairs at a time (equal to the loop bit for bit: test_seeds_restatement_cpu.py)."""
    n = len(xs)
    D = np.zeros((n, n), np.float32)
    ts = line_ts(samples)
    for i in range(n - 1):
        xi, yi = xs[i], ys[i]
        dx, dy = xs[i + 1:] - xi, ys[i + 1:] - yi
        xy = hypot_py(dx, dy)
        xs_line = xi + ts[None, :] * dx[:, None]                  # float32 ts * float64 dx -> float64
        ys_line = yi + ts[None, :] * dy[:, None]
        rows, cols = rowcol_float(inv6, xs_line, ys_line)
        with np.errstate(invalid="ignore"):
            rows = np.clip(rows.round().astype(int), 0, cost.shape[0] - 1)
            cols = np.clip(cols.round().astype(int), 0, cost.shape[1] - 1)
        mean_cost = np.ascontiguousarray(cost[rows, cols]).mean(axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            d = xy.astype(np.float32) * (1.0 + weight * mean_cost)    # a Python float xy_dist is weak: float32 arithmetic
        short = (xy <= xy_thresh) | (weight == 0)
        d = np.where(short, xy.astype(np.float32), d)
        d = np.where(xy == 0, np.float32(0), d)
        D[i, i + 1:] = d
        D[i + 1:, i] = d
    return D


def mean_f32_written_order(a):
    """The float32 mean of `a` in the order obia_amd's kernel adds (NumPy's pairwise sum for up to 128 values)."""
    a = np.asarray(a, np.float32)
    n = len(a)
    if n < 8:
        res = np.float32(0)
        for v in a:
            res = np.float32(res + v)
    else:
        r = [a[j] for j in range(8)]
        k = 8
        while k < n - (n % 8):
            for j in range(8):
                r[j] = np.float32(r[j] + a[k + j])
            k += 8
        f = np.float32
        res = f(f(f(r[0] + r[1]) + f(r[2] + r[3])) + f(f(r[4] + r[5]) + f(r[6] + r[7])))
        while k < n:
            res = np.float32(res + a[k])
            k += 1
    return np.float32(res / np.float32(n))


def components(D, eps):
    """DBSCAN(eps, min_samples=1, metric="precomputed").fit(D).labels_: components of D <= eps, numbered by first member."""
    adj = np.asarray(D) <= np.float32(eps)
    _, lab = connected_components(csr_matrix(adj | adj.T), directed=False)
    _, first = np.unique(lab, return_index=True)
    order = np.argsort(first)                       # component ids in order of their first member
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return rank[lab].astype(np.int32)


def triu_stats(D):
    """min / np.median / max of the upper triangle (seeds.py:225-227)."""
    dvals = D[np.triu_indices(len(D), 1)]
    with np.errstate(invalid="ignore"):
        return dvals.min(), np.median(dvals), dvals.max()


# ---------------------------------------------------------------------------------------------------------------- cases
def pixel_affine(pixel, H):
    """[a, b, d, e, xoff, yoff] of a north-up raster with a dyadic pixel size and origin."""
    return [pixel, 0.0, 0.0, -pixel, 1024.0, 2048.0 + pixel * H]


def inverse6(aff):
    """(a, b, c, d, e, f) of ~Affine for [a, b, d, e, xoff, yoff], as the affine package computes it."""
    sa, sb, sd, se, sc, sf = aff
    idet = 1.0 / (sa * se - sb * sd)
    ra, rb, rd, re = se * idet, -sb * idet, -sd * idet, sa * idet
    return [ra, rb, -sc * ra - sf * rb, rd, re, -sc * rd - sf * re]


def cost_raster(rs, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.clip(0.5 + 0.4 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + rs.normal(0, 0.05, (H, W)), 0, 1).astype(np.float32)


def pixel_centre_case(seed, n, H, W, pixel):
    """n distinct pixel centres of an (H, W) raster: (xs, ys, cost, affine)."""
    rs = np.random.RandomState(seed)
    pix = rs.choice(H * W, n, replace=False)
    rows, cols = pix // W, pix % W
    aff = pixel_affine(pixel, H)
    xs = aff[0] * (cols + 0.5) + aff[1] * (rows + 0.5) + aff[4]
    ys = aff[2] * (cols + 0.5) + aff[3] * (rows + 0.5) + aff[5]
    return xs, ys, cost_raster(rs, H, W), aff


def arbitrary_case(seed, n, H=90, W=110, pixel=0.3):
    """n seeds at arbitrary float64 positions on a raster with a non-dyadic pixel size."""
    rs = np.random.RandomState(seed)
    aff = [pixel, 0.0, 0.0, -pixel, 431000.7, 5012345.1 + pixel * H]
    xs = aff[4] + rs.uniform(0, W * pixel, n)
    ys = aff[5] - rs.uniform(0, H * pixel, n)
    return xs, ys, cost_raster(rs, H, W), aff


def ulp_distance_f32(a, b):
    """Distance in float32 steps between finite values of one sign (0 for equal values, NaN pairs count as equal)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


def near_threshold(xs, ys, D, eps, xy_thresh):
    """True when a decision of the case could flip under a 1-ulp change: some D within 2 float32 ulp of eps or some xy_dist
    within 2 float64 ulp of xy_thresh."""
    iu = np.triu_indices(len(xs), 1)
    d = D[iu]
    e32 = np.float32(eps)
    close_eps = np.abs(d - e32) <= 2 * np.spacing(e32)
    xy = hypot_py(xs[iu[1]] - xs[iu[0]], ys[iu[1]] - ys[iu[0]])
    close_thr = np.abs(xy - xy_thresh) <= 2 * np.spacing(np.float64(xy_thresh))
    return bool(close_eps.any() or close_thr.any())
