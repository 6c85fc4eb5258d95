"""NumPy restatement of scikit-image 0.18's maskSLIC seeding (``_get_mask_centroids``, slic_superpixels.py:14-68), the reference the
GPU routine ``obia_amd.segmentation.mask_centroids`` is pinned on.  Test infrastructure: the library never imports it.

What it restates, in the arithmetic order of the compiled code it stands for (float64 throughout, separate multiply and add):

  picks     ``RandomState(123)``: ``n`` sorted ranks among the valid pixels, then -- only when ``n_valid > 100 * n`` -- ``100 * n``
            sorted ranks from the SAME generator (the points k-means runs on); otherwise every valid pixel is such a point
  k-means   ``scipy.cluster.vq.kmeans2(points, coord[picks], iter=5)``: per point the FIRST centroid that minimises
            ((0 + dz*dz) + dy*dy) + dx*dx (scipy's small-feature loop: ascending scan, strict ``<``); the new centroid is the sum of
            its points (integers: exact in any order) divided by their count, one division per coordinate; a centroid without points
            keeps its position
  steps     ``pdist`` + ``argmin``: per centroid the FIRST other centroid that minimises sqrt(((0 + dz*dz) + dy*dy) + dx*dx) -- the
            ROOTS are compared, two different squares can round to one root -- then ``abs(c - c[closest]).mean(0)``

The distance matrices are built in row chunks of 1 MiB, so K = 1000 on 10^5 points needs a few MB.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

DENSE_FACTOR = 100      # dense_factor ** ndim_spatial = 10 ** 2 for a (1, H, W) mask
CHUNK_BYTES = 1 << 20   # one (rows, K) float64 temporary: small enough to stay in the cache


def picks(n_valid, n):
    """(idx, idx_dense or None): the sorted ranks of the initial centroids and of the k-means points."""
    rnd = np.random.RandomState(123)
    idx_full = np.arange(n_valid, dtype=int)
    idx = np.sort(rnd.choice(idx_full, min(n, n_valid), replace=False))
    n_dense = int(DENSE_FACTOR * n)
    dense = np.sort(rnd.choice(idx_full, n_dense, replace=False)) if n_valid > n_dense else None
    return idx, dense


def _sq(points, book):
    """(len(points), K) squared distances, summed z, y, x in that order starting from 0.  An axis on which every point and every
    centroid is 0 (the depth axis of a one-plane mask) adds +0.0 to a non-negative sum, which changes no bit: it is skipped."""
    d = np.zeros((len(points), len(book)))
    for a in range(3):
        if not points[:, a].any() and not book[:, a].any():
            continue
        t = points[:, a, None] - book[None, :, a]
        t *= t
        d += t
    return d


def _rows(K):
    return max(1, CHUNK_BYTES // (8 * max(K, 1)))


def assign(points, book, count_ties=False):
    """Label of every point: the first centroid at the least squared distance.  With count_ties also the number of points for
    which two or more centroids share that least distance.  Chunks are independent; a large problem spreads them over a few
    threads (NumPy releases the interpreter lock inside its loops)."""
    rows = _rows(len(book))

    def one(s):
        d = _sq(points[s:s + rows], book)
        return d.argmin(1), int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum()) if count_ties else 0

    starts = range(0, len(points), rows)
    if len(points) * len(book) > 10 ** 7:
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            parts = list(pool.map(one, starts))
    else:
        parts = [one(s) for s in starts]
    lab = np.concatenate([p[0] for p in parts]) if parts else np.empty(0, np.int64)
    return (lab, sum(p[1] for p in parts)) if count_ties else lab


def update(points, lab, book):
    """(new code book, has_members)."""
    K = len(book)
    cnt = np.bincount(lab, minlength=K)
    new = book.copy()
    has = cnt > 0
    for a in range(3):
        s = np.bincount(lab, weights=points[:, a], minlength=K)   # sums of integers: exact
        new[has, a] = s[has] / cnt[has]
    return new, has


def kmeans(points, book, iters=5, info=None):
    book = np.array(book, np.float64)
    for it in range(iters):
        if info is not None and it == 0:
            lab, info["ties_first_iter"] = assign(points, book, count_ties=True)
        else:
            lab = assign(points, book)
        book, has = update(points, lab, book)
        if info is not None:
            info.setdefault("empty_per_iter", []).append(int((~has).sum()))
    return book


def closest_other(cent):
    K = len(cent)
    out = np.zeros(K, np.int64)
    for s in range(0, K, _rows(K)):
        d = np.sqrt(_sq(cent[s:s + _rows(K)], cent))
        d[np.arange(len(d)), np.arange(s, s + len(d))] = np.inf
        out[s:s + len(d)] = d.argmin(1)
    return out


def mask_centroids(mask, n, iters=5, info=None):
    """(centroids (K, 3) float64 as (0, y, x), steps (3,)) of scikit-image 0.18's ``_get_mask_centroids(mask[None], n, True)``.
    ``info`` (a dict) receives n_valid, n_dense (None: every valid pixel), ties_first_iter and empty_per_iter."""
    yy, xx = np.nonzero(np.asarray(mask))
    coord = np.stack([np.zeros(len(yy)), yy.astype(np.float64), xx.astype(np.float64)], 1)
    idx, dense = picks(len(coord), n)
    if info is not None:
        info.update(n_valid=len(coord), n_dense=None if dense is None else len(dense), K=len(idx))
    cent = kmeans(coord if dense is None else coord[dense], coord[idx], iters, info)
    steps = np.abs(cent - cent[closest_other(cent)]).mean(0)
    return cent, steps


FIXTURES = ("mask_128x160x4_c025", "mask_128x160x4_c10", "maskones_96x96x4", "sigma_mask_96x128x4", "spacing_mask_96x128x4")


def edge_case(name, chunk=1024):
    """(mask, n_segments) of the edge cases the tests share; ``chunk``: centroids the library stages in LDS at a time."""
    if name == "no_dense_draw":            # n_valid <= 100 * n: every valid pixel is a k-means point
        yy, xx = np.mgrid[0:41, 0:53]
        return ((yy - 20) ** 2 * 2 + (xx - 26) ** 2 < 19 ** 2 * 2), 30
    if name == "n_above_n_valid":          # K = n_valid: every valid pixel is a centroid
        m = np.zeros((9, 11), bool)
        m[2, 3:7] = m[5, 1] = m[6, 8:10] = True
        return m, 20
    if name == "empty_cluster":            # found by search: clusters lose all their points from the third iteration on
        rs = np.random.RandomState(281)
        H, W = rs.randint(6, 20), rs.randint(6, 24)
        m = rs.rand(H, W) < rs.uniform(0.3, 1.0)
        return m, int(int(m.sum()) * rs.uniform(0.4, 0.95))
    if name == "ties":                     # all-ones square: integer seeds, many points at equal distance from two of them
        return np.ones((48, 48), bool), 16
    if name == "chunk_plus_one":           # the scan crosses from one LDS chunk into a second one that holds a single centroid
        return np.ones((64, 64), bool), chunk + 1
    if name == "two":
        yy, xx = np.mgrid[0:37, 0:29]
        return (yy + xx) % 3 != 0, 2
    if name == "single_row":               # one valid row, wider than a workgroup's 256 columns, inside a taller raster
        m = np.zeros((7, 301), bool)
        m[4, 5:297] = True
        return m, 12
    if name == "blob_k1000":               # a dense draw of 10^5 points out of 107 465: 391 workgroups, each scanning the 1000 centroids
        yy, xx = np.mgrid[0:384, 0:384]
        return (yy - 192) ** 2 + (xx - 190) ** 2 < 185 ** 2, 1000
    raise KeyError(name)


EDGE_CASES = ("no_dense_draw", "n_above_n_valid", "empty_cluster", "ties", "chunk_plus_one", "two", "single_row", "blob_k1000")
