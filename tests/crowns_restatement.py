"""Cost allocation restated in plain Python and NumPy (test helper, not a conftest): the contract of include/obia_crowns.h.

`allocate` computes the distance with a heap Dijkstra in float64 (Python floats: IEEE double, nothing contracted) and the labels as a
NumPy fixpoint loop over the tight edges.  It shares no code with the library and none of its structure: no tiles, no rounds."""
import heapq
import math

import numpy as np

NO_LABEL = np.iinfo(np.int32).max
EDGE = ((0, -1), (0, 1), (-1, 0), (1, 0))
CORNER = ((-1, -1), (-1, 1), (1, -1), (1, 1))


def steps(pixel_size=1.0, connectivity=8):
    """[(dy, dx, length)]: sx for a horizontal step, sy for a vertical one, sqrt(sx * sx + sy * sy) for a diagonal one"""
    sy, sx = (float(pixel_size),) * 2 if np.ndim(pixel_size) == 0 else [float(v) for v in pixel_size]
    assert connectivity in (4, 8)
    out = [(dy, dx, sx if dy == 0 else sy) for dy, dx in EDGE]
    if connectivity == 8:
        out += [(dy, dx, math.sqrt(sx * sx + sy * sy)) for dy, dx in CORNER]
    return out


def passable(cost, mask=None):
    ok = np.isfinite(np.asarray(cost, np.float32))
    return ok if mask is None else ok & (np.asarray(mask) != 0)


def edge_weight(length, weight, cu, cv):
    """the one formula, in this order; the arguments are Python floats"""
    return length * (1.0 + weight * (0.5 * (cu + cv)))


def valid_seeds(ok, seed_rows, seed_cols, seed_ids):
    H, W = ok.shape
    return [(int(r), int(c), int(i)) for r, c, i in zip(seed_rows, seed_cols, seed_ids) if 0 <= r < H and 0 <= c < W and ok[int(r), int(c)]]


def distance(cost, seed_rows, seed_cols, mask=None, weight=0.5, pixel_size=1.0, connectivity=8):
    """D without max_dist: heap Dijkstra"""
    cost = np.asarray(cost, np.float32)
    H, W = cost.shape
    ok = passable(cost, mask)
    if (cost[ok] < 0).any():
        raise ValueError("negative cost")
    c = cost.astype(np.float64).tolist()
    okl = ok.tolist()
    nb = steps(pixel_size, connectivity)
    weight = float(weight)
    D = [[math.inf] * W for _ in range(H)]
    heap = []
    for r, q, _ in valid_seeds(ok, seed_rows, seed_cols, np.ones(len(seed_rows), np.int64)):
        if D[r][q] != 0.0:
            D[r][q] = 0.0
            heap.append((0.0, r, q))
    if not heap:
        raise ValueError("no seed lies on a passable pixel of the raster")
    heapq.heapify(heap)
    while heap:
        d, r, q = heapq.heappop(heap)
        if d > D[r][q]:
            continue
        for dy, dx, length in nb:
            r2, q2 = r + dy, q + dx
            if 0 <= r2 < H and 0 <= q2 < W and okl[r2][q2]:
                cand = d + edge_weight(length, weight, c[r][q], c[r2][q2])
                if cand < D[r2][q2]:
                    D[r2][q2] = cand
                    heapq.heappush(heap, (cand, r2, q2))
    return np.array(D, np.float64)


def _shifted(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` where that lies outside"""
    H, W = a.shape
    b = np.full_like(a, fill)
    b[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)] = a[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)]
    return b


def labels_of(D, cost, seed_rows, seed_cols, seed_ids, mask=None, weight=0.5, pixel_size=1.0, connectivity=8):
    """the greatest fixpoint of label[v] = min(label[v], min over tight u of label[u]); 0 where D is not finite"""
    cost = np.asarray(cost, np.float32)
    ok = passable(cost, mask)
    c = np.where(ok, cost, 0).astype(np.float64)
    fin = np.isfinite(D)
    L = np.full(D.shape, NO_LABEL, np.int64)
    for r, q, i in valid_seeds(ok, seed_rows, seed_cols, seed_ids):
        assert 1 <= i < NO_LABEL
        L[r, q] = min(L[r, q], i)
    tight = []
    for dy, dx, length in steps(pixel_size, connectivity):
        Du, cu = _shifted(D, dy, dx, np.inf), _shifted(c, dy, dx, 0.0)
        with np.errstate(invalid="ignore"):
            tight.append((dy, dx, fin & np.isfinite(Du) & (Du + length * (1.0 + float(weight) * (0.5 * (cu + c))) == D)))
    while True:
        new = L.copy()
        for dy, dx, t in tight:
            new = np.where(t, np.minimum(new, _shifted(L, dy, dx, NO_LABEL)), new)
        if np.array_equal(new, L):
            break
        L = new
    L[~fin] = 0
    assert not (L == NO_LABEL).any()
    return L.astype(np.int32)


def allocate(cost, seed_rows, seed_cols, seed_ids, mask=None, weight=0.5, pixel_size=1.0, connectivity=8, max_dist=None):
    """(dist float64, labels int32) of the contract"""
    kw = dict(mask=mask, weight=weight, pixel_size=pixel_size, connectivity=connectivity)
    D = distance(cost, seed_rows, seed_cols, **kw)
    if max_dist is not None:
        D[D > max_dist] = np.inf
    return D, labels_of(D, cost, seed_rows, seed_cols, seed_ids, **kw)


# ---- cases shared by the host and the device tests -------------------------------------------------------------------------------
def spiral_wall(n):
    """mask of an n x n raster (n odd): a one-pixel corridor that winds from the centre outwards between one-pixel walls"""
    m = np.zeros((n, n), np.uint8)
    r = q = n // 2
    m[r, q] = 1
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    k, run = 0, 2
    while True:
        for _ in range(2):
            dy, dx = dirs[k % 4]
            for _ in range(run):
                r, q = r + dy, q + dx
                if not (0 <= r < n and 0 <= q < n):
                    return m
                m[r, q] = 1
            k += 1
        run += 2
