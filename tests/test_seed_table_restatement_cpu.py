"""The restatement of the seed-table options (tests/seed_table_restatement.py) against the libraries the reference calls --
scipy's cKDTree.query_ball_point, pandas' groupby / nlargest / median / sort_values, sklearn's DBSCAN -- and against a
transcription of what its NMS loop does.  Every case asserts on the restatement's own output that it holds what makes the
comparison bite (a reassigned seed, an emptied pre-cluster, a pair exactly on a radius, ...).  Comparisons are exact.

Equal heights occur only where our own tie rule is tested (nlargest's keep="first" is pandas' documented rule and is compared);
sort_values never sees a tie."""
import functools

import numpy as np
import pytest

from tests import seed_table_restatement as T
from tests import seeds_restatement as R

STAGE1 = dict(eps_scale=0.4, min_eps=2.5, max_eps=8, z_thresh=16.0, min_samples=3)


@functools.lru_cache(maxsize=None)
def lattice(seed=12, n=160, H=34, W=40):
    """pixel centres of a raster with a dyadic pixel size (0.5), so that lattice distances -- 2.5 = (1.5, 2.0), 5 = (3, 4) -- are exact;
    heights 6.25 and 12.5 give eps exactly 2.5 and 5.0, the others anything in 2 .. 25; all heights distinct but for those two"""
    xs, ys, cost, aff = R.pixel_centre_case(seed, n, H, W, 0.5)
    rs = np.random.RandomState(seed + 1)
    hs = rs.uniform(2.0, 25.0, n).astype(np.float32)
    hs[rs.rand(n) < 0.2] = 6.25
    hs[rs.rand(n) < 0.2] = 12.5
    for a in (xs, ys, hs, cost):
        a.setflags(write=False)
    return xs, ys, hs, cost, aff


def distinct(hs, seed=0):
    """the heights made distinct (for sort_values, whose order of ties is not specified)"""
    rs = np.random.RandomState(seed)
    out = (np.asarray(hs, np.float32) + rs.permutation(len(hs)).astype(np.float32) / np.float32(1024.0)).astype(np.float32)
    assert len(set(out.tolist())) == len(out)
    return out


# ---- the promotions, pinned on NumPy >= 2 / pandas ---------------------------------------------------------------------------------
def test_promotions_of_numpy_and_pandas():
    pd = pytest.importorskip("pandas")
    assert int(np.__version__.split(".")[0]) >= 2
    h = np.float32(7.3)
    e = 0.4 * h                                                              # weak Python scalar: float32
    assert isinstance(e, np.float32) and e == np.float32(0.4) * h
    assert float(np.clip(e, 2.1, 8)) == T.eps_of(h, 0.4, 2.1, 8) and float(np.clip(0.4 * np.float32(1.3), 2.1, 8)) == float(np.float32(2.1))
    s = pd.Series(np.array([3.25, 1.5, 9.0], np.float32))
    spread = s.max() - s.min()
    assert isinstance(spread, np.float32)
    assert bool(spread > 7.4999999) == bool(spread > np.float32(7.4999999)) and not spread > 7.4999999   # the threshold rounds to float32 7.5
    assert bool(np.float32(7.5) <= 7.4999999)                                # ... in <= as well
    assert all(isinstance(v, float) for v in s)                              # a float32 Series iterates as Python floats: r is float64
    assert max(0.5, 0.1 * 3.25) == T.nms_radius(np.float32(3.25), 0.5, 0.1) and max(0.1, 0.1 * 3.25) == T.nms_radius(np.float32(3.25), 0.1, 0.1)
    assert isinstance(s.median(), np.float32)


def test_the_median_of_a_float32_column():
    pd = pytest.importorskip("pandas")
    one = np.float32(1.0)
    nxt = np.nextafter(one, np.float32(2.0))
    cases = [[1.0, 2.0, 4.0], [1.0, 2.0, 4.0, 8.0], [3.0, one, nxt, 0.5], [0.1, 0.7, 0.3, 0.9, 0.5, 0.2],
             [1.0, 3.0e38, 3.0e38, 3.1e38],                                  # the float32 sum of the middle two overflows
             [1.0e-45, 3.0e-45]]
    for c in cases:
        v = np.array(c, np.float32)
        with np.errstate(over="ignore"):
            want = pd.Series(v).median()
            got = T.median32(v)
        assert isinstance(want, np.float32) and got.dtype == np.float32 and got == want, (c, got, want)
    with np.errstate(over="ignore"):
        assert np.isinf(T.median32(np.array(cases[4], np.float32)))          # the mean is taken in float32: a float64 mean gives 3e38


# ---- the ball ------------------------------------------------------------------------------------------------------------------------
def test_ball_is_inclusive_as_the_kd_tree_decides_it():
    sp = pytest.importorskip("scipy.spatial")
    xs, ys, _, _, _ = lattice()
    tree = sp.cKDTree(np.c_[xs, ys])
    exact = 0
    for i in range(len(xs)):
        for r in (2.5, 5.0, 2.0, 3.3):
            want = sorted(tree.query_ball_point([xs[i], ys[i]], r))
            assert T.ball(xs, ys, i, r) == want
            exact += sum(1 for j in want if (xs[i] - xs[j]) ** 2 + (ys[i] - ys[j]) ** 2 == r * r and j != i)
    assert exact > 0                                                         # some pair lies exactly on a radius
    tri = sp.cKDTree(np.array([[0.0, 0.0], [3.0, 4.0]]))
    assert sorted(tri.query_ball_point([0.0, 0.0], 5.0)) == [0, 1] == T.ball(np.array([0.0, 3.0]), np.array([0.0, 4.0]), 0, 5.0)
    assert tri.query_ball_point([0.0, 0.0], np.nextafter(5.0, 0.0)) == [0]


# ---- stage 1 -------------------------------------------------------------------------------------------------------------------------
def stage1_with_the_tree(xs, ys, hs, eps_scale, min_eps, max_eps, z_thresh, min_samples):
    """the sequential sweep over a k-d tree and a pandas column"""
    sp = pytest.importorskip("scipy.spatial")
    pd = pytest.importorskip("pandas")
    pts = np.c_[xs, ys]
    tree = sp.cKDTree(pts)
    height = pd.Series(hs)
    labels = np.full(len(xs), -1)
    nxt = 0
    for i in range(len(xs)):
        if labels[i] == -1:
            members = tree.query_ball_point(pts[i], float(np.clip(eps_scale * height.iloc[i], min_eps, max_eps)))
            col = height.iloc[members]
            if (z_thresh < 0 or not col.max() - col.min() > z_thresh) and len(members) >= min_samples:
                labels[members] = nxt
                nxt += 1
    return labels.astype(np.int32)


def test_stage1_against_the_tree_and_the_closed_form():
    xs, ys, hs, _, _ = lattice()
    trace = {}
    got = T.stage1(xs, ys, hs, trace=trace, **STAGE1)
    assert np.array_equal(got, stage1_with_the_tree(xs, ys, hs, **STAGE1))
    assert np.array_equal(got, T.stage1_closed_form(xs, ys, hs, **STAGE1))
    # what makes this case bite
    first, ids = trace["first"], trace["ids"]
    assert ((first != got) & (first != -1)).any()                            # a seed whose final pre-cluster is not its first
    assert set(range(ids)) - set(got.tolist())                               # an id no seed kept
    why = [T.eligible(xs, ys, hs, i, **STAGE1)[1] for i in range(len(xs))]
    assert "z" in why and "n" in why                                         # ineligible by z_thresh, and by min_samples
    on_eps = 0
    for i in range(len(xs)):
        e = T.eps_of(hs[i], STAGE1["eps_scale"], STAGE1["min_eps"], STAGE1["max_eps"])
        on_eps += sum(1 for j in range(len(xs)) if j != i and (xs[i] - xs[j]) ** 2 + (ys[i] - ys[j]) ** 2 == e * e)
    assert on_eps > 0                                                        # a pair at distance exactly eps
    # other settings, the defaults among them
    for kw in (dict(), dict(z_thresh=0), dict(min_samples=1), dict(eps_scale=0.9, min_eps=0, max_eps=3.0, z_thresh=4.5, min_samples=2)):
        a = T.stage1(xs, ys, hs, **kw)
        assert np.array_equal(a, stage1_with_the_tree(xs, ys, hs, **dict(dict(eps_scale=0.4, min_eps=2, max_eps=8, z_thresh=-1, min_samples=2), **kw)))
        assert np.array_equal(a, T.stage1_closed_form(xs, ys, hs, **kw))


def test_reduction_against_pandas():
    pd = pytest.importorskip("pandas")
    xs, ys, hs, _, _ = lattice()
    cl1 = T.stage1(xs, ys, hs, **STAGE1)
    assert (cl1 == -1).any() and len(set(hs[cl1 >= 0].tolist())) < (cl1 >= 0).sum()      # singles, and ties for keep="first"
    df = pd.DataFrame({"height": hs, "cluster1": cl1})
    for top in (0, 1, 2, 5):
        k = max(1, top)
        tall = df[df.cluster1 != -1].groupby("cluster1", group_keys=False).apply(lambda d: d.nlargest(k, "height"))
        want = list(tall.index) + list(df[df.cluster1 == -1].index)
        assert T.reduce_stage1(cl1, hs, top).tolist() == want, top
    # our tie rule, stated: equal heights keep the earlier row first
    assert T.reduce_stage1(np.array([0, 0, 0, -1, 0]), np.array([5, 7, 7, 9, 7], np.float32), 2).tolist() == [1, 2, 3]


# ---- split, trim, NMS ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clustered():
    """the lattice's seeds merged at a radius that leaves clusters of many sizes"""
    xs, ys, hs, cost, aff = lattice()
    cl = R.components(R.distance_matrix(xs, ys, cost, R.inverse6(aff), 0.5, 0.8, 12), 1.5)
    sizes = np.bincount(cl)
    assert sizes.max() >= 6 and (sizes == 1).any() and (sizes == 2).any()
    cl.setflags(write=False)
    return cl


def split_with_pandas(pd, cl, hs, dz):
    df = pd.DataFrame({"cluster": cl, "height": hs})
    parts, nid = [], 0
    for _, sub in df.groupby("cluster"):
        if sub.height.max() - sub.height.min() <= dz:
            groups = [sub]
        else:
            mid = sub.height.median()
            groups = [sub[sub.height <= mid], sub[sub.height > mid]]
        for g in groups:
            if not g.empty:
                parts.append(g.assign(cluster=nid))
                nid += 1
    out = pd.concat(parts)
    return out.index.to_numpy(), out.cluster.to_numpy()


def test_height_split_against_pandas():
    pd = pytest.importorskip("pandas")
    _, _, hs, _, _ = lattice()
    cl = clustered()
    for dz in (4.0, 0.5, 30.0, 7.4999999):
        perm, new = T.split(cl, hs, dz)
        wperm, wnew = split_with_pandas(pd, cl, hs, dz)
        assert np.array_equal(perm, wperm) and np.array_equal(new, wnew), dz
    perm, new = T.split(cl, hs, 4.0)
    assert new.max() + 1 > cl.max() + 1                                      # a cluster was split ...
    whole = [c for c in range(cl.max() + 1) if len(set(new[np.isin(perm, np.flatnonzero(cl == c))])) == 1 and (cl == c).sum() > 1]
    assert whole                                                             # ... and one of several rows kept whole
    assert not np.array_equal(T.split(cl, hs, 30.0)[0], np.arange(len(cl)))  # rows are grouped even when nothing is split
    assert np.array_equal(T.split(cl, hs, 30.0)[1], np.sort(cl))
    # an even cluster whose middle heights are adjacent float32 values; one whose upper part is empty
    one = np.float32(1.0)
    h = np.array([9.0, one, np.nextafter(one, np.float32(2.0)), 0.25, 5.0, 5.0, 1.0], np.float32)
    c = np.array([0, 0, 0, 0, 1, 1, 1])
    perm, new = T.split(c, h, 0.5)
    wperm, wnew = split_with_pandas(pd, c, h, 0.5)
    assert np.array_equal(perm, wperm) and np.array_equal(new, wnew)
    assert perm.tolist() == [1, 3, 0, 2, 4, 5, 6] and new.tolist() == [0, 0, 1, 1, 2, 2, 2]


def test_trim_against_pandas():
    pd = pytest.importorskip("pandas")
    _, _, hs, _, _ = lattice()
    cl = clustered()
    df = pd.DataFrame({"cluster": cl, "height": hs})
    biggest = int(np.bincount(cl).max())
    for m in (1, 2, 3, biggest - 1, biggest, biggest + 5):
        want = df.groupby("cluster", group_keys=False).apply(lambda d: d if len(d) <= m else d.nlargest(m, "height")).index.to_numpy()
        assert np.array_equal(T.trim(cl, hs, m), want), m
    assert np.array_equal(T.trim(cl, hs, biggest), np.arange(len(cl)))       # a call in which none is trimmed keeps the table's order
    sel = T.trim(cl, hs, 2)                                                  # trimmed clusters beside untrimmed ones
    assert len(sel) < len(cl) and (np.bincount(cl) <= 2).any() and not np.array_equal(sel, np.sort(sel))
    assert np.array_equal(T.trim(cl, hs, 0), np.arange(len(cl)))


def nms_as_the_loop_behaves(pd, sp, xs, ys, hs, cl, base, scale):
    """per cluster: sort by height, a k-d tree over the sorted rows, and a sweep in which EVERY row clears its ball and sets itself
    (the loop's test of the row's own flag can never be true at that point: the flag is set only at and after the row's own turn)"""
    df = pd.DataFrame({"x": xs, "y": ys, "height": hs, "cluster": cl})
    out = []
    for _, sub in df.groupby("cluster"):
        sub = sub.sort_values("height", ascending=False)
        pts = sub[["x", "y"]].to_numpy()
        tree = sp.cKDTree(pts)
        flags = np.zeros(len(sub), bool)
        for k, h in enumerate(sub.height):
            assert not flags[k]
            flags[tree.query_ball_point(pts[k], max(base, scale * h))] = False
            flags[k] = True
        out += list(sub.index[flags])
    return np.array(out, np.int64)


def test_nms_against_the_loops_behaviour():
    pd = pytest.importorskip("pandas")
    sp = pytest.importorskip("scipy.spatial")
    xs, ys, hs, _, _ = lattice()
    hs = distinct(hs)
    cl = clustered()
    for base, scale in ((1.0, 0.0), (0.0, 0.1), (2.5, 0.2), (0.5, 0.05), (-1.0, 0.08)):
        want = nms_as_the_loop_behaves(pd, sp, xs, ys, hs, cl, base, scale)
        got = T.nms(xs, ys, hs, cl, base, scale)
        assert np.array_equal(got, want), (base, scale)
    assert len(T.nms(xs, ys, hs, cl, 2.5, 0.2)) < len(xs)
    # a pair exactly on r_i = 2.5, (1.5, 2.0) apart inside one cluster, and it decides
    d2 = (xs[:, None] - xs[None, :]) ** 2 + (ys[:, None] - ys[None, :]) ** 2
    same = cl[:, None] == cl[None, :]
    assert ((d2 == 6.25) & same).any()
    assert len(T.nms(xs, ys, hs, cl, 2.5, 0.0)) < len(T.nms(xs, ys, hs, cl, np.nextafter(2.5, 0.0), 0.0))
    # the worked example: a taller seed removed by a lower one
    x, h = np.array([0.0, 1.0, 2.0, 10.0]), np.array([9, 8, 7, 6], np.float32)
    assert T.nms(x, np.zeros(4), h, np.zeros(4, int), 1.0, 0.0).tolist() == [2, 3]
    assert nms_as_the_loop_behaves(pd, sp, x, np.zeros(4), h, np.zeros(4, int), 1.0, 0.0).tolist() == [2, 3]
    # our own tie rule: equal heights, the earlier row first in the order, so the later one clears it
    assert T.nms(np.array([0.0, 0.5]), np.zeros(2), np.array([4, 4], np.float32), np.zeros(2, int), 1.0, 0.0).tolist() == [1]
    assert np.array_equal(T.nms(xs, ys, hs, cl, 0, 0), np.arange(len(xs)))


def test_merge_of_a_reordered_table_against_dbscan():
    sk = pytest.importorskip("sklearn.cluster")
    xs, ys, hs, cost, aff = lattice()
    sel = T.reduce_stage1(T.stage1(xs, ys, hs, **STAGE1), hs, 2)
    assert not np.array_equal(sel, np.sort(sel))
    D = R.distance_matrix(xs[sel], ys[sel], cost, R.inverse6(aff), 0.5, 0.8, 12)
    want = sk.DBSCAN(eps=2.2, min_samples=1, metric="precomputed").fit(D).labels_
    assert np.array_equal(R.components(D, 2.2), want)


def test_sample_heights_by_hand():
    chm = np.arange(12, dtype=np.float32).reshape(3, 4)
    chm[1, 2] = np.nan
    aff = [0.5, 0.0, 0.0, -0.5, 100.0, 50.0]                                 # x = 100 + 0.5 col, y = 50 - 0.5 row
    xs = np.array([100.0, 100.49, 101.0, 101.25, 101.999, 102.0, 99.999, 100.75])
    ys = np.array([50.0, 49.75, 49.25, 49.25, 48.5001, 49.0, 49.9, 48.5])
    h, keep = T.sample_heights(xs, ys, chm, aff)
    # (row 0, col 0) (0, 0) (1, 2): NaN  (1, 2): NaN  (2, 3)  col 4: outside  col -1: outside  row 3: outside
    assert keep.tolist() == [0, 1, 4] and h[keep].tolist() == [0.0, 0.0, 11.0] and np.isnan(h[[2, 3, 5, 6, 7]]).all()


def test_the_rounds_decide_what_the_closed_form_says():
    xs, ys, hs, _, _ = lattice()
    for kw in (STAGE1, dict(), dict(eps_scale=0.9, min_eps=0, max_eps=3.0, z_thresh=4.5, min_samples=2)):
        fired, rounds = T.stage1_rounds(xs, ys, hs, **kw)
        assert np.array_equal(fired, T.fired_and_owner(xs, ys, hs, **kw)[0]) and 1 <= rounds <= len(xs)
    assert T.stage1_rounds(xs, ys, hs, **STAGE1)[1] > 1                      # some seed had to wait for an earlier one
