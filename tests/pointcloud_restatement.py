"""NumPy / plain-Python restatement of include/obia_points.h (test helper, not a conftest): the pixel rule in float64, the state with
``np.add.at`` / ``np.maximum.at``, the columns in float64 as the header orders them, the same columns in ``np.longdouble``, and the
intensity pair as exact rationals.  Also the base case the GPU tests share."""
import math
from fractions import Fraction

import numpy as np

COLUMNS = ("n_points", "ch", "pai", "fhd", "mean_intensity", "variance_intensity")


def invert_affine(t):
    """obia_amd.consumers.invert_affine, restated: [a, b, d, e, xoff, yoff] of the inverse"""
    a, b, d, e, xoff, yoff = [float(v) for v in t]
    det = a * e - b * d
    ia, ib, id_, ie = e / det, -b / det, -d / det, a / det
    return [ia, ib, id_, ie, -(ia * xoff + ib * yoff), -(id_ * xoff + ie * yoff)]


def zkey(z):
    """the order-preserving key of float32 values, uint32"""
    b = np.ascontiguousarray(z, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def zunkey(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def pixel_of(x, y, inv6, H, W):
    """flat pixel index of every point, -1 outside: separate multiplies and adds, left to right, in float64"""
    a, b, d, e, xoff, yoff = [np.float64(v) for v in inv6]
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        col = np.floor(((a * x) + (b * y)) + xoff)
        row = np.floor(((d * x) + (e * y)) + yoff)
        inside = (col >= 0.0) & (col < float(W)) & (row >= 0.0) & (row < float(H))
    px = np.full(x.shape, -1, np.int64)
    px[inside] = row[inside].astype(np.int64) * W + col[inside].astype(np.int64)
    return px


def rasters_state(x, y, z, inv6, H, W, zk=None, count=None):
    """(zkey, count) (H, W) uint32, added to the planes given"""
    zk = np.zeros(H * W, np.uint32) if zk is None else zk.reshape(-1).copy()
    count = np.zeros(H * W, np.uint32) if count is None else count.reshape(-1).copy()
    z = np.asarray(z, np.float32)
    px = pixel_of(x, y, inv6, H, W)
    inside = px >= 0
    np.add.at(count, px[inside], np.uint32(1))
    fin = inside & np.isfinite(z)
    np.maximum.at(zk, px[fin], zkey(z[fin]))
    return zk.reshape(H, W), count.reshape(H, W)


def rasters_finish(zk, count, pixel_area):
    chm = np.where(zk != 0, zunkey(zk), np.float32(np.nan)).astype(np.float32)
    density = count.astype(np.float32) / np.float32(pixel_area)
    return chm, density.astype(np.float32)


def bins_of(z, dz, nz):
    """bin of every height, -1 where the point does not enter the profile"""
    z = np.asarray(z, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(z.astype(np.float64) / np.float64(dz))
        ok = np.isfinite(z) & (z >= np.float32(0.0)) & (q < float(nz))
    j = np.full(z.shape, -1, np.int64)
    j[ok] = q[ok].astype(np.int64)
    return j


def segments_state(x, y, z, intensity, inv6, labels, start_label, N, nz, dz):
    labels = np.asarray(labels, np.int32)
    H, W = labels.shape
    z = np.asarray(z, np.float32)
    px = pixel_of(x, y, inv6, H, W)
    inside = px >= 0
    s = np.full(px.shape, -1, np.int64)
    s[inside] = labels.reshape(-1)[px[inside]].astype(np.int64) - int(start_label)
    has_row = inside & (s >= 0) & (s < N)
    j = bins_of(z, dz, nz)
    prof = has_row & (j >= 0)
    st = {"profile": np.zeros((N, nz), np.uint32), "top": np.zeros(N, np.uint32), "n_int": np.zeros(N, np.uint32),
          "s1": np.zeros(N, np.uint64), "s2": np.zeros(N, np.uint64)}
    np.add.at(st["profile"], (s[prof], j[prof]), np.uint32(1))
    np.maximum.at(st["top"], s[prof], zkey(z[prof]))
    if intensity is not None:
        v = np.asarray(intensity).astype(np.uint64)[has_row]
        np.add.at(st["n_int"], s[has_row], np.uint32(1))
        np.add.at(st["s1"], s[has_row], v)
        np.add.at(st["s2"], s[has_row], v * v)
    st["counters"] = np.array([(~inside).sum(), (inside & ~has_row).sum(), (has_row & ~prof).sum(), prof.sum()], np.uint64)
    return st


def j0_of(min_height, dz, nz):
    return int(min(max(math.ceil(float(min_height) / float(dz)), 0), nz))


def columns(st, dz, min_height=1.0, k=1.0, dtype=np.float64, pad=False):
    """the columns in the header's order of operations, every float operation in ``dtype`` (float64: what the kernel does;
    longdouble: the yardstick its tolerance is measured with)"""
    T = dtype
    profile = st["profile"].astype(np.int64)
    N, nz = profile.shape
    j0 = j0_of(min_height, dz, nz)
    nan = T(np.nan)
    out = {"n_points": np.zeros(N, np.int64)}
    for name in COLUMNS[1:]:
        out[name] = np.full(N, nan, T)
    if pad:
        out["pad"] = np.full((N, nz), nan, T)
    kdz = T(k) * T(dz)
    top = zunkey(st["top"])
    for s in range(N):
        c = [int(v) for v in profile[s]]
        n_all = n_below = 0
        for j in range(nz):
            T_j, E_j = n_all, n_all + c[j]
            if pad:
                if E_j == 0:
                    v = nan
                elif c[j] == 0:
                    v = T(0.0)
                elif T_j == 0:
                    v = nan
                else:
                    v = np.log(T(E_j) / T(T_j)) / kdz
                out["pad"][s, j] = v
            n_all += c[j]
            if j < j0:
                n_below += c[j]
        n_can = n_all - n_below
        out["n_points"][s] = n_all
        if n_all:
            out["ch"][s] = T(top[s])
        if n_all and n_below:
            out["pai"][s] = np.log(T(n_all) / T(n_below)) / T(k)
        if n_can:
            h = T(0.0)
            for j in range(j0, nz):
                if c[j]:
                    p = T(c[j]) / T(n_can)
                    h = h + p * np.log(p)
            out["fhd"][s] = -h
        n, a, b = int(st["n_int"][s]), int(st["s1"][s]), int(st["s2"][s])
        if n:
            hi, lo = divmod(n * b - a * a, 2 ** 64)
            out["mean_intensity"][s] = T(a) / T(n)
            out["variance_intensity"][s] = (T(hi) * T(2.0) ** 64 + T(lo)) / (T(n) * T(n))
    return out


def exact_intensity(st):
    """(mean, variance) of every row as Fractions, None where the row has no intensity"""
    out = []
    for n, a, b in zip(st["n_int"], st["s1"], st["s2"]):
        n, a, b = int(n), int(a), int(b)
        out.append((Fraction(a, n), Fraction(n * b - a * a, n * n)) if n else None)
    return out


def ulps(got, want):
    """|got - want| in units of the spacing of float64 at ``want`` (``want``: float64, Fraction or longdouble), elementwise"""
    got = np.asarray(got, np.float64)
    out = np.zeros(got.shape, np.float64)
    for i, (g, w) in enumerate(zip(got.reshape(-1), np.asarray(want, object).reshape(-1))):
        if isinstance(w, Fraction):
            wf = float(w)
            d = abs(Fraction(float(g)) - w) / Fraction(float(np.spacing(abs(wf)))) if wf != 0.0 else abs(Fraction(float(g))) / Fraction(5e-324)
            out.reshape(-1)[i] = float(d)
        else:
            w = np.longdouble(w)
            if np.isnan(w) or np.isnan(g):
                out.reshape(-1)[i] = 0.0 if (np.isnan(w) and np.isnan(g)) else np.inf
            else:
                out.reshape(-1)[i] = float(abs(np.longdouble(g) - w) / np.longdouble(np.spacing(abs(np.float64(w)))))
    return out


# ------------------------------------------------------------------------------------------------------------------ the base case
H, W, NSEG, DZ, ZMAX = 37, 53, 60, 0.3, 31.7
AFFINE = [0.5, 0.0, 0.0, -0.5, 1000.0, 2000.0]
_C, _S = 0.5 * math.cos(0.4), 0.5 * math.sin(0.4)
AFFINE_ROTATED = [_C, -_S, -_S, -_C, 1000.0, 2000.0]
EMPTY_IDS = (7, 23, 41, 58)                                       # segments whose points are taken off the raster: four NaN rows


def base_labels():
    ids = np.arange(1, 65, dtype=np.int32).reshape(8, 8)
    labels = np.kron(ids, np.ones((5, 7), np.int32))[:H, :W].astype(np.int32)     # 5 x 7 blocks, the last row and column of blocks cut
    labels[labels > NSEG] = 0
    labels[:2, :3] = -1
    return labels


def base_case(affine=AFFINE, n=10007, seed=7):
    """labels and a cloud in map coordinates under ``affine``: points over the raster's extent and two pixels (one metre) around it,
    every 11th column and every 13th row coordinate on a pixel border, gamma heights with every 17th a multiple of dz, every 19th
    negative, every 23rd NaN, one equal to z_max, one infinite; a NaN and an infinite coordinate; uint16 intensities with 0 and 65535"""
    rs = np.random.RandomState(seed)
    labels = base_labels()
    col, row = rs.uniform(-2.0, W + 2.0, n), rs.uniform(-2.0, H + 2.0, n)
    col[::11] = rs.randint(-1, W + 2, len(col[::11]))
    row[::13] = rs.randint(-1, H + 2, len(row[::13]))
    inside = (col >= 0) & (col < W) & (row >= 0) & (row < H)
    lab = np.zeros(n, np.int64)
    lab[inside] = labels[np.floor(row[inside]).astype(int), np.floor(col[inside]).astype(int)]
    col[np.isin(lab, EMPTY_IDS)] += 3.0 * W
    a, b, d, e, xoff, yoff = affine
    x, y = a * col + b * row + xoff, d * col + e * row + yoff
    z = rs.gamma(2.0, 4.0, n)
    z[::17] = DZ * rs.randint(0, 100, len(z[::17]))
    z[::19] = -rs.uniform(0.0, 3.0, len(z[::19]))
    z[::23] = np.nan
    z = z.astype(np.float32)
    z[5], z[29] = np.float32(ZMAX), np.float32(np.inf)
    x[31], y[37] = np.nan, np.inf
    intensity = rs.randint(0, 65536, n).astype(np.uint16)
    intensity[3], intensity[4] = 0, 65535
    return {"labels": labels, "x": x, "y": y, "z": z, "intensity": intensity, "affine": list(affine), "inv": invert_affine(affine)}
