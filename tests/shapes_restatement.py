"""The shape columns restated in NumPy and plain Python (test helper, not a conftest): the yardstick the GPU is held to
(include/obia_shapes.h, obia_amd/shapes.py).

``tables`` gives the integer sums and the boxes from ``np.add.at`` and four shifted comparisons of the padded raster; ``tables_loop``
is the double loop over pixels with Python integers the CPU tests check it against.  ``derived`` restates every float column with
``np.float64`` arrays in the stated order, one rounding per operation; ``merge`` and ``pair_shapes`` are the stated steps on the
tables of tests/adjacency_restatement.py."""
import numpy as np

from tests.adjacency_restatement import NAN, rows_of, same_bits, segment_index  # noqa: F401  (same_bits: for the tests)

F64, I32, I64 = np.float64, np.int32, np.int64
FOUR_PI = F64(4.0) * F64(np.pi)
QUARTER_PI = F64(np.pi) / F64(4.0)
FLOAT_COLUMNS = ("centroid", "mu", "eigenvalues", "major_axis_length", "minor_axis_length", "eccentricity", "orientation", "extent",
                 "compactness", "shape_index", "smoothness")
INT_COLUMNS = ("area", "perimeter", "bbox_height", "bbox_width")


# ------------------------------------------------------------------------------------------------------------ the integer tables
def tables(labels, start_label, N):
    """(sums (N, 7) int64, box (N, 4) int32)"""
    labels = np.asarray(labels)
    H, W = labels.shape
    seg = segment_index(labels, start_label, N)
    S = np.full((H + 2, W + 2), N + 1, I64)
    S[1:-1, 1:-1] = seg
    mid = S[1:-1, 1:-1]
    edges = ((S[:-2, 1:-1] != mid).astype(I64) + (S[2:, 1:-1] != mid) + (S[1:-1, :-2] != mid) + (S[1:-1, 2:] != mid))
    r, c = np.mgrid[0:H, 0:W].astype(I64)
    keep = seg < N
    i, r, c, e = seg[keep], r[keep], c[keep], edges[keep]
    sums = np.zeros((N, 7), I64)
    for k, v in enumerate((np.ones_like(r), r, c, r * r, c * c, r * c, e)):
        np.add.at(sums[:, k], i, v)
    box = np.zeros((N, 4), I64)
    if N:
        lo_r, lo_c = np.full(N, H, I64), np.full(N, W, I64)
        np.minimum.at(lo_r, i, r)
        np.minimum.at(lo_c, i, c)
        np.maximum.at(box[:, 2], i, r + 1)
        np.maximum.at(box[:, 3], i, c + 1)
        has = sums[:, 0] > 0
        box[has, 0], box[has, 1] = lo_r[has], lo_c[has]
    return sums, box.astype(I32)


def tables_loop(labels, start_label, N):
    """the same tables by a double loop over the pixels, Python integers throughout"""
    lab = np.asarray(labels)
    H, W = lab.shape
    sums = [[0] * 7 for _ in range(N)]
    box = [None] * N

    def seg(r, c):
        if not (0 <= r < H and 0 <= c < W):
            return "outside"
        d = int(lab[r, c]) - int(start_label)
        return d if 0 <= d < N else "background"
    for r in range(H):
        for c in range(W):
            i = seg(r, c)
            if isinstance(i, str):
                continue
            per = sum(seg(r + dr, c + dc) != i for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)))
            for k, v in enumerate((1, r, c, r * r, c * c, r * c, per)):
                sums[i][k] += v
            b = box[i]
            box[i] = (r, c, r + 1, c + 1) if b is None else (min(b[0], r), min(b[1], c), max(b[2], r + 1), max(b[3], c + 1))
    return np.array(sums, I64).reshape(N, 7), np.array([b or (0, 0, 0, 0) for b in box], I32).reshape(N, 4)


# ------------------------------------------------------------------------------------------------------------ the derived columns
def _nan_where_empty(x, present):
    x = np.array(x, F64, copy=True)
    x[~present] = NAN
    return x


def box_sums(sums, box):
    """the first and second sums about the box origin (r0, c0), exact int64 (wrapping arithmetic; the results fit):
    (n, S_r, S_c, S_rr, S_cc, S_rc)"""
    with np.errstate(over="ignore"):
        n, sr, sc, srr, scc, src = (sums[:, k].astype(I64) for k in range(6))
        r0, c0 = box[:, 0].astype(I64), box[:, 1].astype(I64)
        return (n, sr - n * r0, sc - n * c0, srr - 2 * r0 * sr + n * r0 * r0, scc - 2 * c0 * sc + n * c0 * c0,
                src - c0 * sr - r0 * sc + n * r0 * c0)


def _shape_terms(area, perimeter, height, width, present):
    """extent, compactness, shape_index, smoothness of (area, perimeter, box sides), int64 in"""
    fn, fp = area.astype(F64), perimeter.astype(F64)
    with np.errstate(all="ignore"):
        extent = fn / (height * width).astype(F64)
        compactness = (FOUR_PI * fn) / (fp * fp)
        shape_index = fp / (F64(4.0) * np.sqrt(fn))
        smoothness = fp / (F64(2.0) * (height + width).astype(F64))
    return {k: _nan_where_empty(v, present) for k, v in (("extent", extent), ("compactness", compactness), ("shape_index", shape_index),
                                                         ("smoothness", smoothness))}


def derived(sums, box, arctan2=np.arctan2):
    """every column of ShapeTable from the integer tables, in the stated order of operations"""
    sums, box = np.asarray(sums, I64), np.asarray(box, I32)
    present = sums[:, 0] > 0
    out = {"present": present, "area": sums[:, 0].copy(), "perimeter": sums[:, 6].copy(),
           "bbox_height": box[:, 2].astype(I64) - box[:, 0], "bbox_width": box[:, 3].astype(I64) - box[:, 1]}
    n, s_r, s_c, s_rr, s_cc, s_rc = box_sums(sums, box)
    fn = n.astype(F64)
    with np.errstate(all="ignore"):
        out["centroid"] = _nan_where_empty(np.stack([sums[:, 1].astype(F64) / fn, sums[:, 2].astype(F64) / fn], 1), present)
        f_r, f_c, nn = s_r.astype(F64), s_c.astype(F64), fn * fn
        mu_rr = (fn * s_rr.astype(F64) - f_r * f_r) / nn
        mu_cc = (fn * s_cc.astype(F64) - f_c * f_c) / nn
        mu_rc = (fn * s_rc.astype(F64) - f_r * f_c) / nn
        out["mu"] = _nan_where_empty(np.stack([mu_rr, mu_cc, mu_rc], 1), present)
        t, d = mu_rr + mu_cc, mu_rr - mu_cc
        q = np.sqrt(d * d + F64(4.0) * (mu_rc * mu_rc))
        l1 = (t + q) / F64(2.0)
        l2 = np.maximum((t - q) / F64(2.0), F64(0.0))
        out["eigenvalues"] = _nan_where_empty(np.stack([l1, l2], 1), present)
        out["major_axis_length"] = _nan_where_empty(F64(4.0) * np.sqrt(l1), present)
        out["minor_axis_length"] = _nan_where_empty(F64(4.0) * np.sqrt(l2), present)
        out["eccentricity"] = _nan_where_empty(np.where(l1 == 0, F64(0.0), np.sqrt(F64(1.0) - l2 / l1)), present)
        # scikit-image 0.18.3: a, b, b, c = inertia_tensor.flat = mu_cc, -mu_rc, -mu_rc, mu_rr; a == c: -pi/4 if b < 0 else pi/4;
        # otherwise atan2(-2 b, c - a) / 2
        angle = F64(0.5) * arctan2(F64(2.0) * mu_rc, d)
        out["orientation"] = _nan_where_empty(np.where(d == 0, np.where(mu_rc > 0, -QUARTER_PI, QUARTER_PI), angle), present)
    out.update(_shape_terms(out["area"], out["perimeter"], out["bbox_height"], out["bbox_width"], present))
    return out


def centroid_xy(centroid, affine):
    """(N, 2) map coordinates (x, y) of the pixel centres' mean; affine = [a, b, d, e, xoff, yoff]"""
    a, b, d, e, xoff, yoff = (F64(float(v)) for v in affine)
    half = F64(0.5)
    with np.errstate(all="ignore"):
        rr, cc = centroid[:, 0] + half, centroid[:, 1] + half
        x = (a * cc + b * rr) + xoff
        y = (d * cc + e * rr) + yoff
    xy = np.stack([x, y], 1)
    xy[np.isnan(xy)] = NAN
    return xy


# ------------------------------------------------------------------------------------------------------------- merge, pair shapes
def merge(sums, box, root, indptr, neighbor, border):
    """the tables of the objects ``root`` forms, stored at row root[i]; every other row empty"""
    sums, box, root = np.asarray(sums, I64), np.asarray(box, I64), np.asarray(root, I64)
    N = len(root)
    new = np.zeros_like(sums)
    for i in range(N):
        new[root[i]] += sums[i]
    rows = rows_of(indptr)
    for e in range(len(neighbor)):
        j = int(neighbor[e])
        if 0 <= j < N and root[rows[e]] == root[j]:
            new[root[j], 6] -= int(border[e])
    nbox = [None] * N
    for i in range(N):
        if sums[i, 0] > 0:
            k, b = int(root[i]), nbox[int(root[i])]
            nbox[k] = tuple(box[i]) if b is None else (min(b[0], box[i, 0]), min(b[1], box[i, 1]), max(b[2], box[i, 2]), max(b[3], box[i, 3]))
    return new, np.array([b or (0, 0, 0, 0) for b in nbox], I32).reshape(N, 4)


def pair_shapes(indptr, neighbor, border, sums, box):
    """for every CSR entry the shape of the union of its two ends; pseudo entries: 0 and NaN"""
    sums, box = np.asarray(sums, I64), np.asarray(box, I64)
    N, nnz = len(sums), len(neighbor)
    rows = rows_of(indptr)
    real = (np.asarray(neighbor) >= 0) & (np.asarray(neighbor) < N)
    j = np.where(real, neighbor, 0).astype(I64)
    i = rows if nnz else np.zeros(0, I64)
    area = np.where(real, sums[i, 0] + sums[j, 0], 0)
    perimeter = np.where(real, sums[i, 6] + sums[j, 6] - 2 * np.asarray(border, I64), 0)
    ubox = np.stack([np.minimum(box[i, 0], box[j, 0]), np.minimum(box[i, 1], box[j, 1]), np.maximum(box[i, 2], box[j, 2]),
                     np.maximum(box[i, 3], box[j, 3])], 1) * real[:, None]
    out = {"area": area.astype(I64), "perimeter": perimeter.astype(I64), "box": ubox.astype(I32)}
    terms = _shape_terms(out["area"], out["perimeter"], ubox[:, 2] - ubox[:, 0], ubox[:, 3] - ubox[:, 1], real)
    out.update({k: terms[k] for k in ("compactness", "shape_index", "smoothness")})
    return out
