"""The seed-table options on the GPU against the restatement (tests/seed_table_restatement.py): every stage and the whole of
``canonical_seeds``, exactly.

Sizes 1, 2, 63, 64, 65, 257 and 1500 (one lane, a wave less one / exactly / plus one, more than one workgroup, six of them); a chain
of 300 seeds that each cover the next (one round per link); 200 coincident seeds (one cell holds everything); one cluster of 400
through split, trim and NMS; two groups 10^6 units apart (the grid must not take memory for the gap); tables that lose their first,
last and interior rows to the CHM sampling; every option on in one call."""
import functools

import numpy as np
import pytest

from tests import seed_table_restatement as T
from tests import seeds_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = (1, 2, 63, 64, 65, 257, 1500)
STAGE1_SETTINGS = (dict(), dict(eps_scale=0.4, min_eps=2.5, max_eps=8, z_thresh=16.0, min_samples=3),
                   dict(eps_scale=0.9, min_eps=0, max_eps=3.0, z_thresh=0.75, min_samples=1))
KEYS = ("id", "cluster", "ch_max", "origin", "x", "y")


@pytest.fixture(scope="module")
def S():
    from obia_amd import seeds
    return seeds


@functools.lru_cache(maxsize=None)
def table(n, seed=0):
    """n seeds on the half-unit lattice of a square that holds about one seed per 5 square units (repeats allowed: coincident seeds),
    heights 2 .. 25 with the two values that put eps exactly on lattice distances, and a cluster column of about n / 4 ids"""
    rs = np.random.RandomState(1000 * seed + n)
    side = max(4, int(np.ceil(np.sqrt(5.0 * n))))
    xs = 431000.25 + 0.5 * rs.randint(0, 2 * side, n)
    ys = 5012345.75 - 0.5 * rs.randint(0, 2 * side, n)
    hs = rs.uniform(2.0, 25.0, n).astype(np.float32)
    hs[rs.rand(n) < 0.2] = 6.25
    hs[rs.rand(n) < 0.2] = 12.5
    cl = rs.randint(0, n // 4 + 1, n).astype(np.int32)
    for a in (xs, ys, hs, cl):
        a.setflags(write=False)
    return xs, ys, hs, cl


@functools.lru_cache(maxsize=None)
def want_stage1(n, k):
    xs, ys, hs, _ = table(n)
    out = T.stage1(xs, ys, hs, **STAGE1_SETTINGS[k])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_stage1_at_every_size(S, n):
    xs, ys, hs, _ = table(n)
    for k, kw in enumerate(STAGE1_SETTINGS):
        got = S.stage1_clusters(xs, ys, hs, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and np.array_equal(got, want_stage1(n, k)), (n, kw)
        rounds, seeds = S.stage1_rounds()
        assert 1 <= rounds <= n and seeds == n
    if n >= 63:
        assert (want_stage1(n, 1) >= 0).any() and (want_stage1(n, 1) == -1).any()


@pytest.mark.parametrize("n", SIZES)
def test_reduce_split_trim_nms_at_every_size(S, n):
    xs, ys, hs, cl = table(n)
    cl1 = want_stage1(n, 1)
    for top in (1, 3):
        assert np.array_equal(S.reduce_stage1(cl1, hs, top), T.reduce_stage1(cl1, hs, top)), top
    for dz in (3.0, 12.0, 100.0):
        perm, new = S.split_clusters_by_height(cl, hs, dz)
        wperm, wnew = T.split(cl, hs, dz)
        assert perm.dtype == np.int64 and new.dtype == np.int32 and np.array_equal(perm, wperm) and np.array_equal(new, wnew), dz
    for m in (1, 2, 4, 1000):
        sel = S.trim_clusters(cl, hs, m)
        assert sel.dtype == np.int64 and np.array_equal(sel, T.trim(cl, hs, m)), m
    for base, scale in ((2.5, 0.0), (0.0, 0.15), (1.0, 0.1), (-1.0, 0.05)):
        sel = S.nms_per_crown(xs, ys, hs, cl, base, scale)
        assert sel.dtype == np.int64 and np.array_equal(sel, T.nms(xs, ys, hs, cl, base, scale)), (base, scale)
    # the switches that are off are the identity
    ident = np.arange(n)
    assert np.array_equal(S.trim_clusters(cl, hs, 0), ident) and np.array_equal(S.nms_per_crown(xs, ys, hs, cl, 0, 0), ident)
    perm, new = S.split_clusters_by_height(cl, hs, 0)
    assert np.array_equal(perm, ident) and np.array_equal(new, cl)


def test_a_chain_of_300_seeds_takes_a_round_per_link(S):
    n = 300
    xs, ys, hs = 1000.0 + np.arange(n, dtype=np.float64), np.full(n, 77.5), np.full(n, 2.5, np.float32)      # eps = clip(1.0, 1, 8) = 1
    kw = dict(eps_scale=0.4, min_eps=1, max_eps=8, min_samples=2)
    fired, rounds = T.stage1_rounds(xs, ys, hs, **kw)
    assert rounds == n and fired.tolist() == [i % 2 == 0 for i in range(n)]
    got = S.stage1_clusters(xs, ys, hs, **kw)
    assert np.array_equal(got, T.stage1(xs, ys, hs, **kw))
    assert S.stage1_rounds() == (rounds, n) and rounds <= n
    # the same chain in reverse table order: the last seed of the line fires first
    got = S.stage1_clusters(xs[::-1].copy(), ys, hs, **kw)
    assert np.array_equal(got, T.stage1(xs[::-1], ys, hs, **kw)) and S.stage1_rounds()[0] <= n


def test_200_coincident_seeds(S):
    n = 200
    rs = np.random.RandomState(4)
    xs, ys = np.full(n, 431000.25), np.full(n, 5012345.75)
    hs = rs.uniform(2, 25, n).astype(np.float32)
    cl = rs.randint(0, 7, n).astype(np.int32)
    for kw in (dict(), dict(z_thresh=30.0), dict(z_thresh=5.0), dict(min_samples=201)):
        assert np.array_equal(S.stage1_clusters(xs, ys, hs, **kw), T.stage1(xs, ys, hs, **kw)), kw
    assert (S.stage1_clusters(xs, ys, hs) == 0).all()
    sel = S.nms_per_crown(xs, ys, hs, cl, 0.5, 0.0)
    assert np.array_equal(sel, T.nms(xs, ys, hs, cl, 0.5, 0.0)) and len(sel) == 7        # the lowest row of every cluster survives
    zero = S.nms_per_crown(xs, ys, hs, cl, -0.0, 1e-300)                                # a radius of almost nothing still holds distance 0
    assert np.array_equal(zero, T.nms(xs, ys, hs, cl, 0.0, 1e-300))


def test_two_groups_a_million_units_apart(S):
    rs = np.random.RandomState(9)
    n = 120
    xs = np.where(np.arange(n) % 2 == 0, 0.0, 1.0e6) + 0.5 * rs.randint(0, 24, n)
    ys = np.where(np.arange(n) % 2 == 0, -1.0e6, 0.0) + 0.5 * rs.randint(0, 24, n)
    hs = rs.uniform(2, 25, n).astype(np.float32)
    cl = rs.randint(0, 9, n).astype(np.int32)
    dx, dy, dh, dc = (torch.as_tensor(a).cuda() for a in (xs, ys, hs, cl))
    S.stage1_clusters(dx, dy, dh)                                            # the context and its workspace exist
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = S.stage1_clusters(dx, dy, dh, min_eps=0.5, max_eps=2.0, eps_scale=0.1)
    sel = S.nms_per_crown(dx, dy, dh, dc, 0.75, 0.0)
    assert torch.cuda.max_memory_allocated() - before < (1 << 20)            # a dense grid of 0.75-unit cells over the extent: 10^12 cells
    assert np.array_equal(got.cpu().numpy(), T.stage1(xs, ys, hs, min_eps=0.5, max_eps=2.0, eps_scale=0.1))
    assert np.array_equal(sel.cpu().numpy(), T.nms(xs, ys, hs, cl, 0.75, 0.0))


# ---- heights from the raster ---------------------------------------------------------------------------------------------------------
CHM_AFFINE = [0.5, 0.0, 0.0, -0.5, 431000.0, 5012400.0]


@functools.lru_cache(maxsize=None)
def chm_case():
    rs = np.random.RandomState(21)
    H, W = 60, 70
    chm = rs.uniform(2, 25, (H, W)).astype(np.float32)
    chm[rs.rand(H, W) < 0.15] = np.nan
    n = 90
    xs = 431000.0 + rs.uniform(-2.0, 0.5 * W + 2.0, n)
    ys = 5012400.0 - rs.uniform(-2.0, 0.5 * H + 2.0, n)
    xs[[0, 40, n - 1]] = [430999.9, 431001.2, 431000.0 + 0.5 * W]            # first, interior and last row off the raster ...
    xs[[1, 2]] = [431000.0, 431000.0 + 0.5 * W - 1e-9]                       # ... and two on its very edge, inside
    ys[[1, 2, 40]] = [5012400.0, 5012400.0 - 0.5 * H + 1e-9, 5012400.3]     # (row 40: above the first row of pixels)
    for a in (chm, xs, ys):
        a.setflags(write=False)
    return chm, xs, ys


def test_sample_heights_drops_first_last_and_interior_rows(S):
    chm, xs, ys = chm_case()
    wh, wkeep = T.sample_heights(xs, ys, chm, CHM_AFFINE)
    assert 0 not in wkeep and 40 not in wkeep and len(xs) - 1 not in wkeep and 10 < len(wkeep) < len(xs) - 5
    h, keep = S.sample_heights(xs, ys, chm, CHM_AFFINE)
    assert h.dtype == np.float32 and keep.dtype == np.int64 and np.array_equal(keep, wkeep) and np.array_equal(h, wh, equal_nan=True)
    assert np.isnan(h[np.setdiff1d(np.arange(len(xs)), keep)]).all() and not np.isnan(h[keep]).any()
    for sub in (slice(0, 1), slice(1, 2), slice(0, 65)):                     # nothing survives; one row; a workgroup's worth
        h, keep = S.sample_heights(xs[sub], ys[sub], chm, CHM_AFFINE)
        wh, wkeep = T.sample_heights(xs[sub], ys[sub], chm, CHM_AFFINE)
        assert np.array_equal(keep, wkeep) and np.array_equal(h, wh, equal_nan=True)
    h, keep = S.sample_heights(np.array([0.5, 69.999, 70.0, -0.0]), np.array([0.0, 59.5, 3.0, 60.0]), chm)       # pixel coordinates
    wh, wkeep = T.sample_heights(np.array([0.5, 69.999, 70.0, -0.0]), np.array([0.0, 59.5, 3.0, 60.0]), chm)
    assert np.array_equal(keep, wkeep) and np.array_equal(h, wh, equal_nan=True)


# ---- the whole function --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(n=220, H=44, W=56):
    """pixel centres of a cost raster at 0.5 units: a CHM table with heights, a density table without"""
    xs, ys, cost, aff = R.pixel_centre_case(31, n, H, W, 0.5)
    rs = np.random.RandomState(32)
    chm = rs.uniform(2, 25, (H, W)).astype(np.float32)
    chm[rs.rand(H, W) < 0.1] = np.nan
    hs = rs.uniform(2, 25, n).astype(np.float32)
    k = 130
    tabs = ((xs[:k], ys[:k], hs[:k]), (xs[k:], ys[k:], None))
    for a in (xs, ys, hs, cost, chm):
        a.setflags(write=False)
    return tabs, cost, aff, chm


def as_dicts(tabs):
    (cx, cy, ch), (dx, dy, dh) = tabs
    a = {"x": cx, "y": cy}
    b = {"x": dx, "y": dy}
    if ch is not None:
        a["ch_max"] = ch
    if dh is not None:
        b["den_max"] = dh
    return a, b


OPTION_SETS = {
    "defaults": dict(),
    "stage1": dict(keep_all_stage1=False),
    "stage1-top-z": dict(keep_all_stage1=False, stage1_top=3, z_thresh=14.0, min_samples=3, min_eps=1.5, max_eps=4.0),
    "dz": dict(dz_merge=3.0),
    "trim": dict(max_per_cluster=2),
    "nms": dict(nms_base=1.0, nms_scale=0.05),
    "all": dict(keep_all_stage1=False, stage1_top=4, z_thresh=14.0, min_samples=2, eps_scale=0.3, min_eps=1.0, max_eps=3.0, merge_radius=2.6,
                cost_weight=0.4, xy_thresh=0.7, dz_merge=2.5, max_per_cluster=3, nms_base=0.6, nms_scale=0.04),
}


@functools.lru_cache(maxsize=None)
def want_canonical(name):
    tabs, cost, aff, chm = scene()
    return T.canonical(tabs[0], tabs[1], cost, chm=chm, chm_affine=aff, cost_affine=aff, **OPTION_SETS[name])


def same_table(got, want):
    for k in KEYS:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        assert len(g) == len(want[k]) and np.array_equal(g, want[k]), k
        if k != "origin":
            assert g.dtype == want[k].dtype, (k, g.dtype)


@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_canonical_seeds_against_the_restatement(S, name):
    tabs, cost, aff, chm = scene()
    a, b = as_dicts(tabs)
    kw = dict(chm=chm, chm_affine=aff, cost_affine=aff, debug_dist=False, **OPTION_SETS[name])
    got = S.canonical_seeds(a, b, cost, **kw)
    want = want_canonical(name)
    same_table(got, want)
    assert all(isinstance(got[k], np.ndarray) for k in KEYS)
    if name != "defaults":                                                   # the options decide something
        base = want_canonical("defaults")
        assert len(want["x"]) != len(base["x"]) or not np.array_equal(want["cluster"], base["cluster"])
    if name == "all":
        again = S.canonical_seeds(a, b, cost, **kw)                          # two runs agree bit for bit
        for k in KEYS:
            assert again[k].tobytes() == got[k].tobytes(), k
        # CUDA tensors in, CUDA tensors out
        ta = {k: torch.as_tensor(v).cuda() for k, v in a.items()}
        tb = {k: torch.as_tensor(v).cuda() for k, v in b.items()}
        t = S.canonical_seeds(ta, tb, torch.as_tensor(cost).cuda(), **dict(kw, chm=torch.as_tensor(chm).cuda()))
        assert all(isinstance(t[k], torch.Tensor) and t[k].is_cuda for k in KEYS if k != "origin") and isinstance(t["origin"], np.ndarray)
        same_table(t, want)


def test_the_stages_return_tensors_for_tensors(S):
    xs, ys, hs, cl = table(257)
    dx, dy, dh, dc = (torch.as_tensor(a).cuda() for a in (xs, ys, hs, cl))
    chm, cx, cy = chm_case()
    outs = [S.stage1_clusters(dx, dy, dh), S.reduce_stage1(dc, dh, 2), *S.split_clusters_by_height(dc, dh, 3.0), S.trim_clusters(dc, dh, 2),
            S.nms_per_crown(dx, dy, dh, dc, 1.0, 0.1), *S.sample_heights(torch.as_tensor(cx).cuda(), torch.as_tensor(cy).cuda(), chm, CHM_AFFINE)]
    assert all(isinstance(o, torch.Tensor) and o.is_cuda for o in outs)
    assert np.array_equal(outs[0].cpu().numpy(), want_stage1(257, 0)) and np.array_equal(outs[4].cpu().numpy(), T.trim(cl, hs, 2))
    assert np.array_equal(outs[5].cpu().numpy(), T.nms(xs, ys, hs, cl, 1.0, 0.1))


def test_one_cluster_of_400_through_split_trim_and_nms(S):
    xs, ys, cost, aff = R.pixel_centre_case(77, 400, 50, 60, 0.5)
    hs = np.random.RandomState(78).uniform(2, 25, 400).astype(np.float32)
    tabs = ((xs[:250], ys[:250], hs[:250]), (xs[250:], ys[250:], hs[250:]))
    a, b = as_dicts(tabs)
    kw = dict(merge_radius=1.0e9, dz_merge=1.0, max_per_cluster=150, nms_base=0.5, nms_scale=0.03)
    want = T.canonical(tabs[0], tabs[1], cost, cost_affine=aff, **kw)
    got = S.canonical_seeds(a, b, cost, cost_affine=aff, debug_dist=False, **kw)
    same_table(got, want)
    assert set(want["cluster"].tolist()) == {0, 1} and 100 < len(want["x"]) < 300
    whole = S.canonical_seeds(a, b, cost, cost_affine=aff, debug_dist=False, merge_radius=1.0e9, nms_base=0.75)
    same_table(whole, T.canonical(tabs[0], tabs[1], cost, cost_affine=aff, merge_radius=1.0e9, nms_base=0.75))
    assert set(whole["cluster"].tolist()) == {0}


def test_the_defaults_are_make_canonical_seeds(S, capsys):
    tabs, cost, aff, _ = scene()
    a, b = as_dicts(((tabs[0][0], tabs[0][1], tabs[0][2]), (tabs[1][0], tabs[1][1], np.full(len(tabs[1][0]), 7.5, np.float32))))
    want = S.make_canonical_seeds(a, b, cost, cost_affine=aff, cost_nodata=0.5, nodata_cost=2)
    said = capsys.readouterr().out
    got = S.canonical_seeds(a, b, cost, cost_affine=aff, cost_nodata=0.5, nodata_cost=2)
    assert capsys.readouterr().out == said and "d_eff" in said
    assert sorted(got) == sorted(want) == sorted(KEYS)
    for k in KEYS:
        assert type(got[k]) is type(want[k]) and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_grow_crowns_makes_a_crown_per_cluster(S, tmp_path, capsys):
    from obia_amd import grow_crowns
    tabs, cost, aff, _ = scene()
    a, b = as_dicts((tabs[0], (tabs[1][0], tabs[1][1], np.random.RandomState(5).uniform(2, 25, len(tabs[1][0])).astype(np.float32))))
    plain = S.canonical_seeds(a, b, cost, cost_affine=aff, debug_dist=False, merge_radius=2.0)
    path = tmp_path / "out" / "canonical.gpkg"
    canon = S.canonical_seeds(a, b, cost, out_path=path, cost_affine=aff, debug_dist=False, merge_radius=2.0, dz_merge=2.0)
    assert f"canonical seeds: {len(canon['x']):,}" in capsys.readouterr().out
    n_clusters = len(np.unique(canon["cluster"]))
    assert n_clusters > len(np.unique(plain["cluster"])) and canon["cluster"].max() == n_clusters - 1
    labels = grow_crowns(cost, canon, cost_affine=aff)                       # every seed on a pixel of its own: every cluster owns one
    assert np.unique(labels[labels > 0]).tolist() == list(range(1, n_clusters + 1))
    # the layer it wrote
    back = S.read_seed_points(path)
    assert np.array_equal(back["x"], canon["x"]) and np.array_equal(back["y"], canon["y"])
    assert np.array_equal(np.asarray(back["id"], np.int64), canon["id"]) and np.array_equal(np.asarray(back["cluster"], np.int32), canon["cluster"])
    assert np.array_equal(np.asarray(back["ch_max"], np.float32), canon["ch_max"]) and list(back["origin"]) == list(canon["origin"])
    assert np.array_equal(grow_crowns(cost, str(path), cost_affine=aff), labels)
