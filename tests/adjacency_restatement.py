"""The segment adjacency graph restated in NumPy and plain Python (test helper, not a conftest): the yardstick the GPU is held to bit
for bit (include/obia_adjacency.h).

The graph comes from two shifted comparisons of the padded raster and ``np.unique`` on the keys; the records of a tile from the same
edges restricted to the tile of the pixel that owns them; ``graph_loop`` is the double loop over pixels the CPU tests check both
against.  ``d2``, the neighbour statistics and the best neighbour are loops over rows with ``np.float64`` scalars in the stated
order; the components are a union-find over the stated links; the drivers are the stated steps and take the statistics as a
callable."""
import numpy as np

F64, I32, I64 = np.float64, np.int32, np.int64
QNAN = 0x7ff8000000000000
NAN = np.array([QNAN], np.uint64).view(F64)[0]                  # THE quiet NaN every output holds


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def quiet(x):
    """every NaN of a float64 array as the quiet NaN"""
    x = np.array(x, F64, copy=True)
    x[np.isnan(x)] = NAN
    return x


def segment_index(labels, start_label, N):
    """0 .. N - 1 for a segment pixel, N for background"""
    d = np.asarray(labels).astype(I64) - int(start_label)
    return np.where((d >= 0) & (d < N), d, N)


# ------------------------------------------------------------------------------------------------------------------- the edges
def _edges(labels, start_label, N):
    """every pixel edge of the raster, the frame's included: (x, y, owner row, owner column), x and y in 0 .. N + 1"""
    H, W = np.asarray(labels).shape
    S = np.full((H + 2, W + 2), N + 1, I64)
    S[1:-1, 1:-1] = segment_index(labels, start_label, N)
    hx, hy = S[1:-1, :-1], S[1:-1, 1:]                            # (H, W + 1): edge k lies between the columns k - 1 and k
    hr, hk = np.mgrid[0:H, 0:W + 1]
    vx, vy = S[:-1, 1:-1], S[1:, 1:-1]                            # (H + 1, W): edge k lies between the rows k - 1 and k
    vk, vc = np.mgrid[0:H + 1, 0:W]
    x = np.concatenate([hx.ravel(), vx.ravel()])
    y = np.concatenate([hy.ravel(), vy.ravel()])
    orow = np.concatenate([hr.ravel(), np.maximum(vk.ravel() - 1, 0)])      # a pixel owns its right and its lower edge,
    ocol = np.concatenate([np.maximum(hk.ravel() - 1, 0), vc.ravel()])      # on the frame also the left and the top one
    return x, y, orow, ocol


def _records(x, y, N, group=None):
    """directed records of the border edges among (x, y): (group, key, edges), sorted by (group, key)"""
    border = (x != y) & (np.minimum(x, y) < N)
    x, y = x[border], y[border]
    g = np.zeros(len(x), I64) if group is None else group[border]
    fwd, back = x < N, y < N
    src = np.concatenate([x[fwd], y[back]])
    dst = np.concatenate([y[fwd], x[back]])
    grp = np.concatenate([g[fwd], g[back]])
    key = src * (N + 2) + dst
    if len(key) == 0:
        return np.zeros(0, I64), np.zeros(0, I64), np.zeros(0, I64)
    both = np.stack([grp, key], 1)
    uniq, counts = np.unique(both, axis=0, return_counts=True)
    return uniq[:, 0], uniq[:, 1], counts.astype(I64)


def graph(labels, start_label, N):
    """(indptr (N + 1) int64, neighbor (nnz) int32, border (nnz) int64)"""
    x, y, _, _ = _edges(labels, start_label, N)
    _, key, edges = _records(x, y, N)
    src = key // (N + 2)
    indptr = np.zeros(N + 1, I64)
    indptr[1:] = np.cumsum(np.bincount(src, minlength=N)[:N]) if N else 0
    return indptr, (key - src * (N + 2)).astype(I32), edges


def tile_records(labels, start_label, N, TH, TW):
    """per tile, row-major: (key int64, edges int32) sorted by key -- the multiset the write pass puts into the tile's rows"""
    H, W = np.asarray(labels).shape
    ntx, nty = -(-W // TW), -(-H // TH)
    x, y, orow, ocol = _edges(labels, start_label, N)
    tile, key, edges = _records(x, y, N, (orow // TH) * ntx + ocol // TW)
    return [(key[tile == t], edges[tile == t].astype(I32)) for t in range(ntx * nty)]


def graph_loop(labels, start_label, N):
    """the same graph by a double loop over the pixels and the edges each of them owns"""
    lab = segment_index(labels, start_label, N)
    H, W = lab.shape
    count = {}

    def edge(a, b):
        if a != b and min(a, b) < N:
            for s, d in ((a, b), (b, a)):
                if s < N:
                    count[(s, d)] = count.get((s, d), 0) + 1
    for r in range(H):
        for c in range(W):
            a = int(lab[r, c])
            edge(a, int(lab[r, c + 1]) if c + 1 < W else N + 1)
            edge(a, int(lab[r + 1, c]) if r + 1 < H else N + 1)
            if c == 0:
                edge(a, N + 1)
            if r == 0:
                edge(a, N + 1)
    keys = sorted(count)
    indptr = np.zeros(N + 1, I64)
    for s, _ in keys:
        indptr[s + 1] += 1
    return np.cumsum(indptr), np.array([d for _, d in keys], I32), np.array([count[k] for k in keys], I64)


def rows_of(indptr):
    return np.repeat(np.arange(len(indptr) - 1, dtype=I64), np.diff(indptr))


def row_sum(indptr, x):
    run = np.concatenate([[0], np.cumsum(np.asarray(x, I64))])
    return run[indptr[1:]] - run[indptr[:-1]]


# ------------------------------------------------------------------------------------------------------------- the table kernels
def d2(indptr, neighbor, N, values):
    values = np.asarray(values, F64).reshape(N, -1)
    out = np.full(len(neighbor), NAN, F64)
    with np.errstate(all="ignore"):
        for i in range(N):
            for e in range(indptr[i], indptr[i + 1]):
                j = int(neighbor[e])
                if not 0 <= j < N:
                    continue
                acc = F64(0.0)
                for f in range(values.shape[1]):
                    d = values[i, f] - values[j, f]
                    t = d * d
                    acc = acc + t
                out[e] = NAN if np.isnan(acc) else acc
    return out


def neighbor_stats(indptr, neighbor, border, N, values):
    values = np.asarray(values, F64).reshape(N, -1)
    F = values.shape[1]
    mean, mn, mx = (np.full((N, F), NAN, F64) for _ in range(3))
    used = np.zeros((N, F), I32)
    with np.errstate(all="ignore"):
        for i in range(N):
            for f in range(F):
                sw, s, lo, hi, n = F64(0.0), F64(0.0), None, None, 0
                for e in range(indptr[i], indptr[i + 1]):
                    j = int(neighbor[e])
                    if not 0 <= j < N:
                        continue
                    v = values[j, f]
                    if np.isnan(v):
                        continue
                    w = F64(int(border[e]))
                    sw = sw + w
                    s = s + w * v
                    if n == 0 or v < lo:
                        lo = v
                    if n == 0 or v > hi:
                        hi = v
                    n += 1
                used[i, f] = n
                if n:
                    m = s / sw
                    mean[i, f] = NAN if np.isnan(m) else m
                    mn[i, f], mx[i, f] = lo, hi
        diff = quiet(values - mean)
    return {"mean": mean, "min": mn, "max": mx, "used": used, "diff": diff}


def class_border(indptr, neighbor, border, N, classes, K):
    out = np.zeros((N, K), I64)
    for i in range(N):
        for e in range(indptr[i], indptr[i + 1]):
            j = int(neighbor[e])
            if 0 <= j < N and 0 <= int(classes[j]) < K:
                out[i, int(classes[j])] += int(border[e])
    return out


def best_neighbor(indptr, neighbor, N, dist2):
    best, best_d2 = np.full(N, -1, I32), np.full(N, NAN, F64)
    for i in range(N):
        for e in range(indptr[i], indptr[i + 1]):
            j, d = int(neighbor[e]), dist2[e]
            if not 0 <= j < N or np.isnan(d):
                continue
            if best[i] < 0 or d < best_d2[i]:
                best[i], best_d2[i] = j, d
    return best, best_d2


def components(indptr, neighbor, N, link):
    """root (N) int32: i and j are linked where the byte of i -> j or of j -> i is set; the root is the smallest member"""
    parent = list(range(N))

    def find(v):
        r = v
        while parent[r] != r:
            r = parent[r]
        while parent[v] != r:
            parent[v], v = r, parent[v]
        return r
    row = rows_of(indptr)
    for e in np.flatnonzero(np.asarray(link) != 0):
        j = int(neighbor[e])
        if 0 <= j < N:
            a, b = find(int(row[e])), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(v) for v in range(N)], I32)


def compact_roots(root, start_label, present=None):
    """the components numbered from start_label in ascending order of root; with `present` (N) bool only those with a present
    member, the others start_label - 1"""
    root = np.asarray(root, I64)
    has = np.ones(len(root), bool)
    if present is not None:
        has = np.zeros(len(root), bool)
        has[root[np.asarray(present, bool)]] = True
    counted = (root == np.arange(len(root))) & has
    return np.where(has[root], np.cumsum(counted)[root] - 1 + int(start_label), int(start_label) - 1).astype(I32)


def relabel(labels, table, start_label):
    labels = np.asarray(labels, I32)
    N = len(table)
    d = labels.astype(I64) - int(start_label)
    out = np.where(d < 0, labels, I32(int(start_label) - 1)).astype(I32)
    seg = (d >= 0) & (d < N)
    out[seg] = np.asarray(table, I32)[d[seg]]
    return out


# ---------------------------------------------------------------------------------------------------------------------- drivers
def count_labels(labels, start_label):
    return max(int(np.asarray(labels).max()) - int(start_label) + 1, 0)


def _merge(labels, root, start_label, indptr, border):
    """segments without a pixel -- without an edge around them -- are not numbered and not counted"""
    table = compact_roots(root, start_label, row_sum(indptr, border) > 0)
    return relabel(labels, table, start_label), (max(int(table.max()) - int(start_label) + 1, 0) if len(table) else 0)


def merge_by_threshold(values, labels, threshold, start_label=1):
    N = count_labels(labels, start_label)
    indptr, neighbor, border = graph(labels, start_label, N)
    dist2 = d2(indptr, neighbor, N, values)
    with np.errstate(invalid="ignore"):
        link = dist2 <= F64(float(threshold)) * F64(float(threshold))
    return _merge(labels, components(indptr, neighbor, N, link), start_label, indptr, border)


def dissolve_by_class(labels, classes, start_label=1):
    N = count_labels(labels, start_label)
    indptr, neighbor, border = graph(labels, start_label, N)
    classes = np.asarray(classes, I64)
    row = rows_of(indptr)
    link = np.zeros(len(neighbor), bool)
    for e in range(len(neighbor)):
        j = int(neighbor[e])
        link[e] = 0 <= j < N and classes[row[e]] == classes[j] and classes[j] >= 0
    return _merge(labels, components(indptr, neighbor, N, link), start_label, indptr, border)


def merge_similar(raw, labels, threshold, stats, max_rounds=8, start_label=1):
    """rounds of mutual best neighbours; ``stats(raw, labels)`` -> (N, F) means.  Returns (labels, counts after every round,
    pairs merged in every round)"""
    labels = np.asarray(labels, I32)
    t2 = F64(float(threshold)) * F64(float(threshold))
    counts, merged = [], []
    for _ in range(int(max_rounds)):
        N = count_labels(labels, start_label)
        indptr, neighbor, border = graph(labels, start_label, N)
        values = np.asarray(stats(raw, labels), F64).reshape(N, -1)
        best, best_d2 = best_neighbor(indptr, neighbor, N, d2(indptr, neighbor, N, values))
        root = np.arange(N, dtype=I32)
        pairs = 0
        for i in range(N):
            j = int(best[i])
            if j >= 0 and int(best[j]) == i and best_d2[i] <= t2:
                root[i] = min(i, j)
                pairs += i < j
        labels, n = _merge(labels, root, start_label, indptr, border)
        counts.append(n)
        merged.append(int(pairs))
        if not pairs:
            break
    return labels, counts, merged
