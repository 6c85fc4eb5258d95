"""The definitions of include/obia_groundfilter.h in NumPy and SciPy (test helper, not a conftest): the cell minimum of a cloud, grey
erosion / dilation / opening with NaN as the empty cell, the schedule, the threshold raster and the classification -- and the scene of
the sanity case.  The GPU is held to these bit for bit.  Nothing here is compared with PDAL."""
import functools

import numpy as np
import scipy.ndimage as ndi

from tests.pointcloud_restatement import invert_affine, pixel_of, zkey, zunkey  # noqa: F401

F32 = np.float32
QNAN = np.uint32(0x7FC00000)
MAX_RADIUS, MAX_STEPS = 127, 16
COUNTERS = ("outside", "non_finite", "rejected", "ground")


def canonical(a):
    """float32 with every NaN the quiet NaN 0x7fc00000"""
    a = np.array(a, F32, copy=True)
    a.view(np.uint32)[np.isnan(a)] = QNAN
    return a


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def as_plane(Z):
    """a plane as the filters read it: float32, -0 as +0"""
    return np.asarray(Z, F32) + F32(0)


# ------------------------------------------------------------------------------------------------------------------- the filters
def _filter(Z, r, lo):
    """minimum (lo) or maximum over the clipped (2r + 1)^2 window, NaN cells ignored, NaN where the window holds nothing else; +-inf
    are data: a second filter over the NaN mask tells a window of empties from a window of infinities"""
    Z = as_plane(Z)
    size = 2 * int(r) + 1
    nan = np.isnan(Z)
    pad = F32(np.inf) if lo else F32(-np.inf)
    f = ndi.minimum_filter if lo else ndi.maximum_filter
    v = f(np.where(nan, pad, Z), size=size, mode="constant", cval=pad)
    empty = ndi.minimum_filter(nan.astype(np.uint8), size=size, mode="constant", cval=1) == 1
    return canonical(np.where(empty, F32(np.nan), v))


def erosion(Z, r):
    return _filter(Z, r, True)


def dilation(Z, r):
    return _filter(Z, r, False)


def opening(Z, r):
    return dilation(erosion(Z, r), r)


def filter_loop(Z, r, lo):
    """the definition itself: a double loop over the clipped window"""
    Z = as_plane(Z)
    H, W = Z.shape
    out = np.full((H, W), np.nan, F32)
    for i in range(H):
        for j in range(W):
            w = Z[max(i - r, 0):i + r + 1, max(j - r, 0):j + r + 1]
            w = w[~np.isnan(w)]
            if w.size:
                out[i, j] = w.min() if lo else w.max()
    return canonical(out)


# ------------------------------------------------------------------------------------------------------------------ the schedule
def schedule(cell_size=1.0, slope=1.0, initial_distance=0.15, max_distance=2.5, max_window_size=33.0, exponential=True, base=2.0):
    radii, dh = [], []
    k, w_prev = 0, None
    while True:
        r = int(round(base ** k)) if exponential else int(round((k + 1) * base))
        w = 2 * r + 1
        if w * cell_size > max_window_size:
            break
        assert len(radii) < MAX_STEPS and 1 <= r <= MAX_RADIUS
        radii.append(r)
        dh.append(initial_distance if w_prev is None else min(slope * (w - w_prev) * cell_size + initial_distance, max_distance))
        w_prev = w
        k += 1
    return radii, dh


# ---------------------------------------------------------------------------------------------------------------- the cell minimum
def z32(z):
    """(float)z + 0.0f"""
    with np.errstate(over="ignore"):
        return np.asarray(z, np.float64).astype(F32) + F32(0)


def cell_keys(x, y, z, inv6, H, W, keys=None):
    """the state: (H, W) uint32 order keys, 0 empty, a larger key a smaller value; added to the plane given"""
    keys = np.zeros(H * W, np.uint32) if keys is None else keys.reshape(-1).copy()
    z = np.asarray(z, np.float64)
    px = pixel_of(x, y, inv6, H, W)
    use = (px >= 0) & np.isfinite(z)
    np.maximum.at(keys, px[use], ~zkey(z32(z[use])))
    return keys.reshape(H, W)


def cell_min_finish(keys):
    return canonical(np.where(keys != 0, zunkey(~keys), F32(np.nan)))


def cell_min(x, y, z, inv6, H, W):
    """the same through np.minimum.at on the values: what the keys stand for"""
    z = np.asarray(z, np.float64)
    px = pixel_of(x, y, inv6, H, W)
    use = (px >= 0) & np.isfinite(z)
    Z = np.full(H * W, np.inf, F32)
    n = np.zeros(H * W, np.int64)
    np.minimum.at(Z, px[use], z32(z[use]))
    np.add.at(n, px[use], 1)
    return canonical(np.where(n > 0, Z, F32(np.nan)).reshape(H, W))


# ------------------------------------------------------------------------------------------- the threshold and the classification
def threshold(zmin, radii, dh):
    """(surface, thresh): S_k = opening(S_k-1, r_k) from zmin, T = min over k of S_k + (float)dh_k, NaN terms ignored"""
    S = canonical(as_plane(zmin))
    T = np.full(S.shape, np.nan, F32)
    for r, d in zip(radii, dh):
        S = opening(S, r)
        with np.errstate(invalid="ignore"):
            T = np.fmin(T, S + F32(d))
    return S, canonical(T)


def classify(x, y, z, inv6, thresh):
    """(flags uint8, counters (4) uint64)"""
    H, W = thresh.shape
    z = np.asarray(z, np.float64)
    px = pixel_of(x, y, inv6, H, W)
    inside = px >= 0
    fin = inside & np.isfinite(z)
    g = np.zeros(len(z), bool)
    with np.errstate(invalid="ignore"):
        g[fin] = z[fin] <= thresh.reshape(-1)[px[fin]].astype(np.float64)
    counters = np.array([(~inside).sum(), (inside & ~fin).sum(), (fin & ~g).sum(), g.sum()], np.uint64)
    return g.astype(np.uint8), counters


def ground_filter(x, y, z, affine, shape, radii, dh):
    inv = invert_affine(affine)
    zmin = cell_min_finish(cell_keys(x, y, z, inv, shape[0], shape[1]))
    S, T = threshold(zmin, radii, dh)
    flags, counters = classify(x, y, z, inv, T)
    return dict(zmin=zmin, surface=S, threshold=T, flags=flags, counters=counters)


def progressive(x, y, z, affine, shape, radii, dh):
    """the per-point progressive filter: a point survives a step when it passes that step's surface"""
    inv = invert_affine(affine)
    H, W = shape
    z = np.asarray(z, np.float64)
    px = pixel_of(x, y, inv, H, W)
    alive = (px >= 0) & np.isfinite(z)
    S = cell_min(x, y, z, inv, H, W)
    at = np.clip(px, 0, None)
    for r, d in zip(radii, dh):
        S = opening(S, r)
        with np.errstate(invalid="ignore"):
            alive &= z <= (S + F32(d)).reshape(-1)[at].astype(np.float64)
    return alive


def north_up(x, y, cell):
    """(shape, affine) of the grid obia_amd.pointcloud.ground_filter lays over a cloud without a transform"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    keep = np.isfinite(x) & np.isfinite(y)
    x, y = x[keep], y[keep]
    left, top = np.floor(x.min() / cell) * cell, np.ceil(y.max() / cell) * cell
    t = [cell, 0.0, 0.0, -cell, float(left), float(top)]
    inv = invert_affine(t)
    W = int(np.floor(inv[0] * x.max() + inv[1] * y.min() + inv[4])) + 1
    H = int(np.floor(inv[2] * x.max() + inv[3] * y.min() + inv[5])) + 1
    return (H, W), t


# ------------------------------------------------------------------------------------------------------------------ the sanity scene
SCENE_SIDE, SCENE_N = 200.0, 160000


def terrain(x, y):
    return 100 + 0.08 * x + 0.05 * y + 3.0 * np.sin(x / 25.0) * np.cos(y / 31.0)


@functools.lru_cache(maxsize=None)
def scene():
    """200 m x 200 m, 160 000 points of RandomState(7) over a sloped sinusoidal terrain with 0.03 m noise, 250 paraboloid trees with
    80 % canopy hits and a 25 x 20 m block 8 m tall: (x, y, z, truth), truth True on the ground.  Shared: do not write to it."""
    rng = np.random.RandomState(7)
    L, n = SCENE_SIDE, SCENE_N
    x, y = rng.uniform(0, L, n), rng.uniform(0, L, n)
    zt = terrain(x, y)
    z = zt + rng.normal(0, 0.03, n)
    truth = np.ones(n, bool)
    for _ in range(250):
        cx, cy, R, Ht = rng.uniform(0, L), rng.uniform(0, L), rng.uniform(1.5, 5), rng.uniform(5, 25)
        d = np.hypot(x - cx, y - cy)
        inside = d < R
        hit = inside & (rng.uniform(size=n) < 0.8)
        z[hit] = zt[hit] + Ht * (1 - (d[hit] / R) ** 2) * rng.uniform(0.5, 1.0, hit.sum()) + 0.5
        truth[hit] = False
    b = (x > 60) & (x < 85) & (y > 120) & (y < 140)
    z[b] = zt[b] + 8.0
    truth[b] = False
    for a in (x, y, z, truth):
        a.setflags(write=False)
    return x, y, z, truth


SCENE_AFFINE, SCENE_SHAPE = [1.0, 0.0, 0.0, -1.0, 0.0, 200.0], (200, 200)


@functools.lru_cache(maxsize=None)
def scene_result():
    x, y, z, _ = scene()
    radii, dh = schedule()
    return ground_filter(x, y, z, SCENE_AFFINE, SCENE_SHAPE, radii, dh)
