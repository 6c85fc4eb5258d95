"""The table options of the canonical seeds restated in plain Python and NumPy loops (test helper, not a conftest): the contract of
include/obia_seed_table.h and of obia_amd.seeds.canonical_seeds.  Every function follows the reference's steps one by one and is
quadratic or worse; tests/test_seed_table_restatement_cpu.py holds it against the libraries the reference calls.

Arithmetic as NumPy >= 2 promotes it: a Python scalar next to a float32 height is weak, so eps, the z_thresh and dz_merge comparisons
and the median are float32; a float32 Series iterates as Python floats, so the NMS radius is float64."""
import numpy as np

from tests import seeds_restatement as R


def in_ball(xi, yi, xj, yj, r):
    dx, dy = np.float64(xi) - np.float64(xj), np.float64(yi) - np.float64(yj)
    return bool(dx * dx + dy * dy <= np.float64(r) * np.float64(r))


def ball(xs, ys, i, r):
    """what cKDTree.query_ball_point returns, ascending (the predicate of in_ball, elementwise over the table)"""
    dx, dy = np.float64(xs[i]) - np.asarray(xs, np.float64), np.float64(ys[i]) - np.asarray(ys, np.float64)
    return np.flatnonzero(dx * dx + dy * dy <= np.float64(r) * np.float64(r)).tolist()


def eps_of(h, eps_scale, min_eps, max_eps):
    e = np.float32(eps_scale) * np.float32(h)
    return float(np.minimum(np.maximum(e, np.float32(min_eps)), np.float32(max_eps)))


def sample_heights(xs, ys, chm, affine=None):
    """(heights with NaN where dropped, surviving rows)"""
    ra, rb, rc, rd, re, rf = R.inverse6(affine if affine is not None else [1, 0, 0, 1, 0, 0])
    H, W = chm.shape
    out = np.full(len(xs), np.nan, np.float32)
    for i, (x, y) in enumerate(zip(xs, ys)):
        col, row = np.floor((ra * x + rb * y) + rc), np.floor((rd * x + re * y) + rf)
        if 0 <= col < W and 0 <= row < H:
            out[i] = chm[int(row), int(col)]
    return out, np.flatnonzero(~np.isnan(out)).astype(np.int64)


def eligible(xs, ys, hs, i, eps_scale, min_eps, max_eps, z_thresh, min_samples):
    """(eligible, why not: "" / "z" / "n")"""
    idx = ball(xs, ys, i, eps_of(hs[i], eps_scale, min_eps, max_eps))
    if z_thresh >= 0 and np.float32(hs[idx].max() - hs[idx].min()) > np.float32(z_thresh):
        return False, "z"
    if len(idx) < min_samples:
        return False, "n"
    return True, ""


def stage1(xs, ys, hs, eps_scale=0.4, min_eps=2, max_eps=8, z_thresh=-1, min_samples=2, trace=None):
    """the loop, as written; ``trace`` (a dict) receives first = every seed's first assignment and ids = the ids handed out"""
    n = len(xs)
    hs = np.asarray(hs, np.float32)
    cl1 = -np.ones(n, np.int64)
    first = -np.ones(n, np.int64)
    cid = 0
    for i in range(n):
        if cl1[i] != -1:
            continue
        idx = ball(xs, ys, i, eps_of(hs[i], eps_scale, min_eps, max_eps))
        if z_thresh >= 0 and np.float32(hs[idx].max() - hs[idx].min()) > np.float32(z_thresh):
            continue
        if len(idx) >= min_samples:
            for j in idx:
                if first[j] == -1:
                    first[j] = cid
            cl1[idx] = cid
            cid += 1
    if trace is not None:
        trace["first"], trace["ids"] = first, cid
    return cl1.astype(np.int32)


def fired_and_owner(xs, ys, hs, eps_scale=0.4, min_eps=2, max_eps=8, z_thresh=-1, min_samples=2):
    """the closed form: fired(i) = eligible(i) and no fired i' < i covers i; owner[j] = the largest fired i that covers j, or -1"""
    n = len(xs)
    hs = np.asarray(hs, np.float32)
    eps = [eps_of(h, eps_scale, min_eps, max_eps) for h in hs]
    fired = np.zeros(n, bool)
    owner = -np.ones(n, np.int64)
    for i in range(n):
        if owner[i] == -1 and eligible(xs, ys, hs, i, eps_scale, min_eps, max_eps, z_thresh, min_samples)[0]:
            fired[i] = True                                                  # no fired earlier seed covers i: owner[i] would say so
            owner[ball(xs, ys, i, eps[i])] = i                               # i is the largest fired seed so far
    return fired, owner


def stage1_closed_form(xs, ys, hs, eps_scale=0.4, min_eps=2, max_eps=8, z_thresh=-1, min_samples=2):
    """cluster1[j] = rank among the fired seeds of the largest fired i that covers j"""
    fired, owner = fired_and_owner(xs, ys, hs, eps_scale, min_eps, max_eps, z_thresh, min_samples)
    rank = np.cumsum(fired) - 1
    return np.where(owner >= 0, rank[np.maximum(owner, 0)], -1).astype(np.int32)


def stage1_rounds(xs, ys, hs, eps_scale=0.4, min_eps=2, max_eps=8, z_thresh=-1, min_samples=2):
    """the closed form decided in rounds, as obia_seedtab_stage1_dev decides it: (fired, rounds)"""
    n = len(xs)
    hs = np.asarray(hs, np.float32)
    eps = [eps_of(h, eps_scale, min_eps, max_eps) for h in hs]
    state = [0 if eligible(xs, ys, hs, i, eps_scale, min_eps, max_eps, z_thresh, min_samples)[0] else 2 for i in range(n)]
    covers = [[k for k in ball(xs, ys, i, np.inf) if k < i and state[k] != 2 and in_ball(xs[k], ys[k], xs[i], ys[i], eps[k])] for i in range(n)]
    rounds = 0
    while True:
        new = list(state)
        for i in range(n):
            if state[i] == 0:
                new[i] = 2 if any(state[k] == 1 for k in covers[i]) else 0 if any(state[k] == 0 for k in covers[i]) else 1
        state, rounds = new, rounds + 1
        if 0 not in state:
            return np.array([s == 1 for s in state]), rounds


def segments(cs, hs, dz_merge):
    """of a table sorted by (cluster, height descending, row): rank in the cluster, its size, and 1 where the cluster is split and the
    row lies above its median (what obia_seedtab_segments_dev writes)"""
    cs, hs = np.asarray(cs), np.asarray(hs, np.float32)
    rank, size, part = np.zeros(len(cs), np.int32), np.zeros(len(cs), np.int32), np.zeros(len(cs), np.uint8)
    for c in set(cs.tolist()):
        rows = np.flatnonzero(cs == c)
        rank[rows], size[rows] = np.arange(len(rows)), len(rows)
        h = hs[rows]
        if dz_merge > 0 and np.float32(h.max() - h.min()) > np.float32(dz_merge):
            part[rows] = h > median32(h)
    return rank, size, part


def tallest(rows, hs, k=None):
    """rows by height descending, ties to the earlier row; the first k"""
    out = sorted(rows, key=lambda r: (-float(hs[r]), r))
    return out if k is None else out[:k]


def reduce_stage1(cl1, hs, stage1_top=1):
    top = max(1, int(stage1_top))
    sel = []
    for c in sorted(set(int(v) for v in cl1 if v != -1)):
        sel += tallest([r for r in range(len(cl1)) if cl1[r] == c], hs, top)
    sel += [r for r in range(len(cl1)) if cl1[r] == -1]
    return np.array(sel, np.int64)


def median32(v):
    """the median of float32 values as pandas takes it: of an even count the mean of the two middle ones in float32 (their sum
    rounds, and overflows, as a float32)"""
    s = np.sort(np.asarray(v, np.float32))
    m = len(s)
    return s[m // 2] if m % 2 else np.float32(np.float32(s[m // 2 - 1] + s[m // 2]) / np.float32(2.0))


def split(cluster, hs, dz_merge):
    """(perm, new cluster column in that order)"""
    hs = np.asarray(hs, np.float32)
    if not dz_merge > 0:
        return np.arange(len(cluster), dtype=np.int64), np.asarray(cluster, np.int32)
    perm, new, nid = [], [], 0
    for c in sorted(set(int(v) for v in cluster)):
        rows = [r for r in range(len(cluster)) if cluster[r] == c]
        h = hs[rows]
        if np.float32(h.max() - h.min()) <= np.float32(dz_merge):
            parts = [rows]
        else:
            mid = median32(h)
            parts = [[r for r in rows if hs[r] <= mid], [r for r in rows if hs[r] > mid]]
        for part in parts:
            if part:
                perm += part
                new += [nid] * len(part)
                nid += 1
    return np.array(perm, np.int64), np.array(new, np.int32)


def trim(cluster, hs, m):
    n = len(cluster)
    groups = [[r for r in range(n) if cluster[r] == c] for c in sorted(set(int(v) for v in cluster))]
    if m <= 0 or all(len(g) <= m for g in groups):
        return np.arange(n, dtype=np.int64)
    sel = []
    for g in groups:
        sel += g if len(g) <= m else tallest(g, hs, m)
    return np.array(sel, np.int64)


def nms_radius(h, base, scale):
    v = float(scale) * float(h)
    return v if v > float(base) else float(base)


def nms(xs, ys, hs, cluster, base, scale):
    """the loop's behaviour: every row in turn clears the others of its cluster within its radius and sets itself"""
    n = len(xs)
    if not (base > 0 or scale > 0):
        return np.arange(n, dtype=np.int64)
    sel = []
    for c in sorted(set(int(v) for v in cluster)):
        order = tallest([r for r in range(n) if cluster[r] == c], hs)
        keep = {r: False for r in order}
        members = set(order)
        for i in order:
            for j in ball(xs, ys, i, nms_radius(hs[i], base, scale)):
                if j in members:
                    keep[j] = False
            keep[i] = True
        sel += [r for r in order if keep[r]]
    return np.array(sel, np.int64)


def canonical(chm_tab, den_tab, cost, chm=None, chm_affine=None, cost_affine=None, eps_scale=0.4, min_eps=2, max_eps=8, z_thresh=-1,
              min_samples=2, merge_radius=1.5, cost_weight=0.5, xy_thresh=0.8, dz_merge=0, keep_all_stage1=True, stage1_top=1,
              max_per_cluster=0, nms_base=0, nms_scale=0):
    """the whole function on tables (x, y, heights or None): dict of id, cluster, ch_max, origin, x, y"""
    cols = []
    for k, (x, y, h) in enumerate((chm_tab, den_tab)):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        if h is None:
            h, keep = sample_heights(x, y, chm, chm_affine)
            x, y, h = x[keep], y[keep], h[keep]
        cols.append((x, y, np.asarray(h, np.float32), np.full(len(x), k)))
    xs, ys, hs, org = [np.concatenate([c[i] for c in cols]) for i in range(4)]
    if not keep_all_stage1:
        sel = reduce_stage1(stage1(xs, ys, hs, eps_scale, min_eps, max_eps, z_thresh, min_samples), hs, stage1_top)
        xs, ys, hs, org = xs[sel], ys[sel], hs[sel], org[sel]
    inv = R.inverse6(cost_affine if cost_affine is not None else [1, 0, 0, 1, 0, 0])
    cl = R.components(R.distance_matrix(xs, ys, cost, inv, cost_weight, xy_thresh, 12), merge_radius).astype(np.int32)
    if dz_merge > 0:
        sel, cl = split(cl, hs, dz_merge)
        xs, ys, hs, org = xs[sel], ys[sel], hs[sel], org[sel]
    if max_per_cluster > 0:
        sel = trim(cl, hs, max_per_cluster)
        xs, ys, hs, org, cl = xs[sel], ys[sel], hs[sel], org[sel], cl[sel]
    if nms_base > 0 or nms_scale > 0:
        sel = nms(xs, ys, hs, cl, nms_base, nms_scale)
        xs, ys, hs, org, cl = xs[sel], ys[sel], hs[sel], org[sel], cl[sel]
    return {"id": np.arange(len(xs), dtype=np.int64), "cluster": cl, "ch_max": hs, "origin": np.array(["chm", "density"])[org], "x": xs,
            "y": ys}
