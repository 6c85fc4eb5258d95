"""NumPy restatement of include/obia_ground.h by brute force (test helper, not a conftest): the full nq x ng matrix of float64 squared
distances, ``np.lexsort`` by the pair (d2, i), the two sums in a Python loop over the neighbours, the terrain-raster rule and the
pixel centres of ``GroundIndex.to_raster``.  Every operation is one correctly rounded IEEE operation in the header's order, NumPy fuses
nothing, and every NaN is made the quiet NaN the header names -- so the kernels are compared with this bit for bit."""
import numpy as np

from tests.pointcloud_restatement import invert_affine, pixel_of  # noqa: F401  (the pixel rule is restated there)

MAX_COUNT = 8
BLOCK = 2048                                                       # queries per block of the distance matrix


def keep_ground(gx, gy, gz):
    """(gx, gy, gz) of the finite ground points in their order, and how many were dropped"""
    gx, gy, gz = (np.asarray(v, np.float64) for v in (gx, gy, gz))
    keep = np.isfinite(gx) & np.isfinite(gy) & np.isfinite(gz)
    return (gx[keep], gy[keep], gz[keep]), int((~keep).sum())


def canonical(a):
    """the array with every NaN the quiet NaN 0x7ff8000000000000 / 0x7fc00000"""
    a = np.array(a, copy=True)
    a[np.isnan(a)] = np.nan
    return a


def ground_z(ground, x, y, count=1, max_distance=0.0):
    """``{"zg": float64, "m": uint8, "d2": float64 (nq, count), "idx": int64 (nq, count), "tie": bool}`` of the queries against the
    kept ground points ``ground`` = (gx, gy, gz).  ``d2`` / ``idx``: the neighbours in order, inf / -1 where there is none; ``tie``:
    the order of the first ``count + 1`` candidates was decided by the index somewhere (two equal d2)."""
    gx, gy, gz = (np.asarray(v, np.float64) for v in ground)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ng, nq, count = len(gx), len(x), int(count)
    assert 1 <= count <= MAX_COUNT and ng >= 1 and np.isfinite(gx).all() and np.isfinite(gy).all() and np.isfinite(gz).all()
    md = np.float64(max_distance)
    md2 = md * md
    k = min(count, ng)
    zg = np.full(nq, np.nan)
    m = np.zeros(nq, np.uint8)
    d2_out, idx_out, tie = np.full((nq, count), np.inf), np.full((nq, count), -1, np.int64), np.zeros(nq, bool)
    index = np.arange(ng, dtype=np.int64)
    for lo in range(0, nq, BLOCK):
        xs, ys = x[lo:lo + BLOCK], y[lo:lo + BLOCK]
        finite = np.isfinite(xs) & np.isfinite(ys)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            dx, dy = xs[:, None] - gx[None, :], ys[:, None] - gy[None, :]
            d2 = (dx * dx) + (dy * dy)
            d2[~finite] = np.inf                                            # judged below: such a query finds nothing
            order = np.lexsort((np.broadcast_to(index, d2.shape), d2), axis=-1)
            first = order[:, :min(k + 1, ng)]
            dfirst = np.take_along_axis(d2, first, 1)
            tie[lo:lo + BLOCK] = (dfirst[:, 1:] == dfirst[:, :-1]).any(1) & finite
            nb, d = first[:, :k], dfirst[:, :k]
            valid = np.broadcast_to(finite[:, None], d.shape).copy()
            if md > 0.0:
                valid &= d <= md2
            mm = valid.sum(1)                                               # d ascends: the valid ones are a prefix
            assert (valid == (np.arange(k)[None, :] < mm[:, None])).all()
            z = gz[nb]
            num, den = np.zeros(len(xs)), np.zeros(len(xs))
            for j in range(k):                                              # in neighbour order: one division, one add
                on = j < mm
                num = np.where(on, num + z[:, j] / d[:, j], num)
                den = np.where(on, den + np.float64(1.0) / d[:, j], den)
            out = num / den
            out = np.where((mm == 1) | (d[:, 0] == 0.0), z[:, 0], out)
            out = np.where(mm == 0, np.nan, out)
        zg[lo:lo + BLOCK] = out
        m[lo:lo + BLOCK] = mm
        d2_out[lo:lo + BLOCK, :k] = np.where(valid, d, np.inf)
        idx_out[lo:lo + BLOCK, :k] = np.where(valid, nb, -1)
    return {"zg": canonical(zg), "m": m, "d2": d2_out, "idx": idx_out, "tie": tie}


def hag(z, zg):
    """(float32)(z - zg): the subtraction in float64, one rounding"""
    with np.errstate(invalid="ignore", over="ignore"):
        return canonical((np.asarray(z, np.float64) - np.asarray(zg, np.float64)).astype(np.float32))


def dtm_z(x, y, dtm, affine):
    """float64: the pixel of ``dtm`` (H, W) float32 that contains each point, NaN outside the raster and where it is not finite"""
    dtm = np.asarray(dtm, np.float32)
    H, W = dtm.shape
    px = pixel_of(x, y, invert_affine(affine), H, W)
    v = dtm.reshape(-1)[np.maximum(px, 0)].astype(np.float64)
    return canonical(np.where((px >= 0) & np.isfinite(v), v, np.nan))


def pixel_centres(shape, affine):
    """(x, y) float64 (H * W,) of the pixel centres, row-major: x = a (c + 0.5) + b (r + 0.5) + xoff, left to right"""
    H, W = shape
    a, b, d, e, xoff, yoff = (np.float64(v) for v in affine)
    c = (np.arange(W, dtype=np.float64) + 0.5)[None, :]
    r = (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    return (((a * c) + (b * r)) + xoff).reshape(-1), (((d * c) + (e * r)) + yoff).reshape(-1)


def to_raster(ground, shape, affine, count=1, max_distance=0.0):
    """(H, W) float32: the ground height at the pixel centres"""
    x, y = pixel_centres(shape, affine)
    return canonical(ground_z(ground, x, y, count, max_distance)["zg"].astype(np.float32)).reshape(shape)


# ---------------------------------------------------------------------------------------------------- the cases of the GPU tests
EXTENT = (64.0, 48.0)
HOLE = (30.0, 22.0, 10.0)                                          # centre and radius of the disc without ground: 20 m across
ORIGIN = (1000.0, 2000.0)


def base_ground(seed=3, n=3000):
    """about n ground points jittered on a lattice over 64 x 48 m without those in the disc, a gentle slope as elevation; eleven
    duplicates of (x, y) with another elevation; five points that are not finite (they are dropped).  Returns (gx, gy, gz) as given
    to the index -- the dropped ones included."""
    rs = np.random.RandomState(seed)
    nx = int(round(np.sqrt(n * EXTENT[0] / EXTENT[1])))
    ny = int(round(n / nx))
    jx, jy = np.meshgrid((np.arange(nx) + 0.5) * EXTENT[0] / nx, (np.arange(ny) + 0.5) * EXTENT[1] / ny)
    gx = ORIGIN[0] + jx.reshape(-1) + rs.uniform(-0.4, 0.4, nx * ny)
    gy = ORIGIN[1] + jy.reshape(-1) + rs.uniform(-0.4, 0.4, nx * ny)
    out = (gx - ORIGIN[0] - HOLE[0]) ** 2 + (gy - ORIGIN[1] - HOLE[1]) ** 2 > HOLE[2] ** 2
    gx, gy = gx[out], gy[out]
    gz = 300.0 + 0.05 * (gx - ORIGIN[0]) - 0.03 * (gy - ORIGIN[1]) + rs.normal(0.0, 0.05, len(gx))
    p = rs.permutation(len(gx))
    gx, gy, gz = gx[p], gy[p], gz[p]
    dup = rs.choice(len(gx), 11, replace=False)
    gx, gy, gz = np.concatenate([gx, gx[dup]]), np.concatenate([gy, gy[dup]]), np.concatenate([gz, gz[dup] + 1.25])
    n0 = len(gx)
    for at, (bx, by, bz) in zip((5, 77, n0 // 7, n0 // 3, (2 * n0) // 3), ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, np.nan), (-np.inf, 0, 0), (0, 0, np.inf))):
        gx, gy, gz = np.insert(gx, at, ORIGIN[0] + bx), np.insert(gy, at, ORIGIN[1] + by), np.insert(gz, at, 300.0 + bz)
    return gx, gy, gz


def base_queries(ground, side, seed=4, n=5000):
    """(x, y, z) of about n queries: most over the extent and its surroundings, every 9th up to three extents outside the bounding box,
    every 7th exactly on a ground point (the duplicates among them), every 11th on exact multiples of ``side``, a NaN and both
    infinities as x or y, every 13th elevation NaN"""
    (gx, gy, _), _ = keep_ground(*ground)
    rs = np.random.RandomState(seed)
    x = ORIGIN[0] + rs.uniform(-4.0, EXTENT[0] + 4.0, n)
    y = ORIGIN[1] + rs.uniform(-4.0, EXTENT[1] + 4.0, n)
    far = np.arange(0, n, 9)
    x[far] = ORIGIN[0] + rs.uniform(-3.0 * EXTENT[0], 4.0 * EXTENT[0], len(far))
    y[far] = ORIGIN[1] + rs.uniform(-3.0 * EXTENT[1], 4.0 * EXTENT[1], len(far))
    on = np.arange(3, n, 7)
    pick = np.concatenate([np.arange(len(gx) - 11, len(gx)), rs.randint(0, len(gx), len(on) - 11)])
    x[on], y[on] = gx[pick], gy[pick]
    mult = np.arange(5, n, 11)
    x[mult] = np.floor(x[mult] / side) * side
    y[mult[::2]] = np.floor(y[mult[::2]] / side) * side
    for at, (bx, by) in zip((17, 170, n // 3, n // 2 + 100, (5 * n) // 8, (7 * n) // 8), ((np.nan, 0), (0, np.nan), (np.inf, 0), (0, -np.inf), (-np.inf, np.inf), (np.nan, np.nan))):
        x[at], y[at] = x[at] + bx, y[at] + by
    z = 300.0 + rs.gamma(2.0, 6.0, n)
    z[::13] = np.nan
    z[6], z[8] = np.inf, -np.inf
    return x, y, z
