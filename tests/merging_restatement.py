"""Region merging on the segment graph restated in NumPy and plain Python (test helper, not a conftest): the yardstick the GPU is held
to bit for bit (include/obia_merging.h).  The cost is a loop over entries with float64 scalars and ``math.sqrt`` in the stated order,
the pair merge a loop over rows, the contraction a dictionary per row, the driver the stated steps."""
import math

import numpy as np

from tests import adjacency_restatement as R

F64, I32, I64 = np.float64, np.int32, np.int64
NAN = R.NAN


def _sqrt(x):
    x = float(x)
    return F64(math.sqrt(x)) if x >= 0.0 else F64(NAN)           # a negative or a NaN gives NaN, as the device's square root does


class State:
    """the tables of a RegionState as host arrays"""

    def __init__(self, area, mean, m2, perimeter, box, indptr, neighbor, border, root=None):
        self.area, self.perimeter = np.array(area, I64), np.array(perimeter, I64)
        self.mean, self.m2 = np.array(mean, F64).reshape(len(self.area), -1), np.array(m2, F64).reshape(len(self.area), -1)
        self.box = np.array(box, I32).reshape(-1, 4)
        self.indptr, self.neighbor, self.border = np.array(indptr, I64), np.array(neighbor, I32), np.array(border, I64)
        self.N = len(self.area)
        self.root = np.arange(self.N, dtype=I32) if root is None else np.array(root, I32)

    def graph(self):
        return self.indptr, self.neighbor, self.border


def state_of(raw, labels, start_label=1, bands=None, n_labels=None):
    """the state of a raster by NumPy: np.mean and np.var of every segment's pixels in float64"""
    from tests import shapes_restatement as S
    labels = np.asarray(labels)
    N = R.count_labels(labels, start_label) if n_labels is None else int(n_labels)
    sums, box = S.tables(labels, start_label, N)
    raw = np.asarray(raw, F64)
    if bands is not None:
        raw = raw[:, :, list(bands)]
    Fb = raw.shape[2]
    mean, m2 = np.full((N, Fb), NAN, F64), np.full((N, Fb), NAN, F64)
    idx = R.segment_index(labels, start_label, N)
    for i in range(N):
        px = raw[idx == i]
        if len(px):
            mean[i] = px.mean(0)
            m2[i] = np.maximum(px.var(0) * len(px), 0.0)
    return State(sums[:, 0], mean, m2, sums[:, 6], box, *R.graph(labels, start_label, N))


def cost_of_pair(st, a, b, border, w, w_color, w_compact):
    """the fusion cost of rows a < b with `border` shared pixel edges"""
    with np.errstate(all="ignore"):
        fa, fb = F64(int(st.area[a])), F64(int(st.area[b]))
        fm = fa + fb
        share = (fa * fb) / fm
        colour = F64(0.0)
        for f in range(st.mean.shape[1]):
            ma, mb = st.m2[a, f], st.m2[b, f]
            d = st.mean[b, f] - st.mean[a, f]
            mm = (ma + mb) + (d * d) * share
            h = fm * _sqrt(mm / fm) - (fa * _sqrt(ma / fa) + fb * _sqrt(mb / fb))
            colour = colour + F64(w[f]) * h
        pa, pb = int(st.perimeter[a]), int(st.perimeter[b])
        la, lb, lm = F64(pa), F64(pb), F64(pa + pb - 2 * int(border))
        xa, xb = [int(v) for v in st.box[a]], [int(v) for v in st.box[b]]
        ba = F64(2.0) * F64((xa[2] - xa[0]) + (xa[3] - xa[1]))
        bb = F64(2.0) * F64((xb[2] - xb[0]) + (xb[3] - xb[1]))
        bm = F64(2.0) * F64((max(xa[2], xb[2]) - min(xa[0], xb[0])) + (max(xa[3], xb[3]) - min(xa[1], xb[1])))
        hc = fm * (lm / _sqrt(fm)) - (fa * (la / _sqrt(fa)) + fb * (lb / _sqrt(fb)))
        hs = fm * (lm / bm) - (fa * (la / ba) + fb * (lb / bb))
        wc, wk = F64(w_color), F64(w_compact)
        c = wc * colour + (F64(1.0) - wc) * (wk * hc + (F64(1.0) - wk) * hs)
        return F64(NAN) if np.isnan(c) else c, colour, hc, hs


def cost(st, w=None, shape=0.1, compactness=0.5):
    w = np.ones(st.mean.shape[1], F64) if w is None else np.asarray(w, F64)
    out = np.full(len(st.neighbor), NAN, F64)
    for i in range(st.N):
        for e in range(st.indptr[i], st.indptr[i + 1]):
            j = int(st.neighbor[e])
            if 0 <= j < st.N:
                out[e] = cost_of_pair(st, min(i, j), max(i, j), st.border[e], w, F64(1.0) - F64(shape), compactness)[0]
    return out


def partner_of(partner, N, i):
    p = int(partner[i])
    if p < 0 or p >= N or p == i:
        return -1
    return p if int(partner[p]) == i else -1


def merge_tables(st, partner):
    """(area, mean, m2, perimeter, box) after the pairs of `partner` merged"""
    area, perimeter, box = st.area.copy(), st.perimeter.copy(), st.box.copy()
    mean, m2 = R.quiet(st.mean), R.quiet(st.m2)
    with np.errstate(all="ignore"):
        for i in range(st.N):
            p = partner_of(partner, st.N, i)
            if p < 0:
                continue
            if p < i:
                area[i] = perimeter[i] = 0
                box[i] = 0
                mean[i] = m2[i] = NAN
                continue
            a, b = i, p
            fa, fb = F64(int(st.area[a])), F64(int(st.area[b]))
            fm = fa + fb
            share, step = (fa * fb) / fm, fb / fm
            for f in range(st.mean.shape[1]):
                d = st.mean[b, f] - st.mean[a, f]
                mm = (st.m2[a, f] + st.m2[b, f]) + (d * d) * share
                mean[a, f] = st.mean[a, f] + d * step
                m2[a, f] = mm
            shared = 0
            for e in range(max(int(st.indptr[a]), 0), min(int(st.indptr[a + 1]), len(st.neighbor))):
                if int(st.neighbor[e]) == b:
                    shared = int(st.border[e])
                    break
            area[a] = st.area[a] + st.area[b]
            perimeter[a] = st.perimeter[a] + st.perimeter[b] - 2 * shared
            box[a] = [min(st.box[a, 0], st.box[b, 0]), min(st.box[a, 1], st.box[b, 1]), max(st.box[a, 2], st.box[b, 2]), max(st.box[a, 3], st.box[b, 3])]
    return area, R.quiet(mean), R.quiet(m2), perimeter, box


def contract(indptr, neighbor, border, N, root):
    """the CSR under `root`, by a dictionary per new row"""
    rows = [dict() for _ in range(N)]
    for i in range(N):
        r = int(root[i])
        for e in range(indptr[i], indptr[i + 1]):
            j = int(neighbor[e])
            k = int(root[j]) if 0 <= j < N else (N if j == N else N + 1)
            if k != r:
                rows[r][k] = rows[r].get(k, 0) + int(border[e])
    out_ptr = np.zeros(N + 1, I64)
    nb, bd = [], []
    for r in range(N):
        for k in sorted(rows[r]):
            nb.append(k)
            bd.append(rows[r][k])
        out_ptr[r + 1] = len(nb)
    return out_ptr, np.array(nb, I32), np.array(bd, I64)


def pair_root(partner, N):
    step = np.arange(N, dtype=I32)
    for i in range(N):
        p = partner_of(partner, N, i)
        if p >= 0:
            step[i] = min(i, p)
    return step


def merge_pairs(st, partner):
    area, mean, m2, perimeter, box = merge_tables(st, partner)
    step = pair_root(partner, st.N)
    return State(area, mean, m2, perimeter, box, *contract(st.indptr, st.neighbor, st.border, st.N, step), root=step[st.root])


def round_partner(st, scale, w=None, shape=0.1, compactness=0.5):
    """(partner, pairs, cost) of one round"""
    c = cost(st, w, shape, compactness)
    best, best_cost = R.best_neighbor(st.indptr, st.neighbor, st.N, c)
    limit = F64(float(scale)) * F64(float(scale))
    partner = np.full(st.N, -1, I32)
    pairs = 0
    for i in range(st.N):
        j = int(best[i])
        if j >= 0 and int(best[j]) == i and best_cost[i] <= limit:
            partner[i] = j
            pairs += i < j
    return partner, int(pairs), c


def drive(st, scale, w=None, shape=0.1, compactness=0.5, max_rounds=None):
    """(states after every round that merged, counts after every round that ran, the final state)"""
    n = int((st.area > 0).sum())
    states, counts = [], []
    while max_rounds is None or len(counts) < max_rounds:
        partner, pairs, _ = round_partner(st, scale, w, shape, compactness)
        if pairs:
            st = merge_pairs(st, partner)
            states.append(st)
        n -= pairs
        counts.append(n)
        if not pairs:
            break
    return states, counts, st


def labels_of(labels, st, start_label=1, present=None):
    present = (np.bincount(R.segment_index(labels, start_label, st.N).ravel(), minlength=st.N + 1)[:st.N] > 0) if present is None else present
    return R.relabel(labels, R.compact_roots(st.root, start_label, present), start_label)
