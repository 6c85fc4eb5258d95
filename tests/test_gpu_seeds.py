"""Seeds on the GPU (obia_amd.seeds, seeds.hip) against the restatement of obia/utils/seeds.py (tests/seeds_restatement.py):
peaks bit for bit in np.where order; the pair distance bit for bit on pixel-centre seeds and within one float32 ulp on
arbitrary coordinates; clusters equal to the components of the restated matrix; min / median / max equal."""
import numpy as np
import pytest
from scipy.ndimage import gaussian_filter

from tests import seeds_restatement as R
from tests.test_seeds_restatement_cpu import ARBITRARY_N, ARBITRARY_SEEDS, EPS, WEIGHT, XY_THRESH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from obia_amd import seeds
    return seeds


def surface(seed, H, W, scale=30.0, blur=1.5):
    rs = np.random.RandomState(seed)
    a = rs.rand(H, W).astype(np.float32) * np.float32(scale)
    return gaussian_filter(a, blur) if min(H, W) > 1 else a


def check_peaks(S, a, v_min, d, sigma, want=None, where=None):
    rows, cols, g, raw, sm = S.detect_peaks(a, v_min, d, sigma, _smooth=True)
    ref_g = R.smooth(a, sigma)
    assert sm.dtype == np.float32 and np.array_equal(sm, ref_g, equal_nan=True), "smoothed plane differs from gaussian_filter"
    want = R.peaks_nan_rule(a, v_min, d, sigma) if want is None else want
    got = np.zeros(a.shape, bool)
    got[rows, cols] = True
    assert got.sum() == len(rows), "a peak is listed twice"
    if where is None:
        wr, wc = np.where(want)
        assert np.array_equal(rows, wr) and np.array_equal(cols, wc), "peak list differs (np.where order)"
        assert rows.dtype == np.int32 and cols.dtype == np.int32
    else:
        assert np.array_equal(got[where], want[where])
    assert np.array_equal(g, ref_g[rows, cols]) and np.array_equal(raw, a[rows, cols])
    return len(rows)


SHAPES = [(1, 1), (1, 37), (37, 1), (5, 63), (9, 64), (5, 65), (2, 3), (3, 2), (70, 130), (131, 257)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sigma,d", [(0, 1), (0, 3), (1, 3), (2, 4), (1, 1), (2, 3), (0, 4)])
def test_peaks_equal_scipy_on_nan_free_planes(S, shape, sigma, d):
    a = surface(shape[0] * 1000 + shape[1], *shape)
    n = check_peaks(S, a, 12.0, d, sigma, want=R.peaks_scipy(a, 12.0, d, sigma))
    if min(shape) >= 70:
        assert n > 0


@pytest.mark.parametrize("sigma,d", [(0, 1), (1, 3), (2, 4)])
def test_peaks_on_plateaus_and_constant_planes(S, sigma, d):
    a = np.round(surface(7, 90, 140) / 4) * 4                     # wide plateaus: every pixel of a flat top is a peak
    assert check_peaks(S, a, 8.0, d, sigma, want=R.peaks_scipy(a, 8.0, d, sigma)) > 0
    c = np.full((33, 70), 5.0, np.float32)
    assert check_peaks(S, c, 2.5, d, 0, want=R.peaks_scipy(c, 2.5, d, 0)) == c.size
    assert check_peaks(S, c, 5.5, d, 0, want=R.peaks_scipy(c, 5.5, d, 0)) == 0
    # the threshold is compared in float32, as arr >= h_min does under NumPy 2
    t = np.full((4, 5), np.float32(2.1), np.float32)
    assert check_peaks(S, t, 2.1, d, 0, want=R.peaks_scipy(t, 2.1, d, 0)) == t.size


@pytest.mark.parametrize("sigma,d", [(0, 1), (0, 3), (1, 3), (2, 4)])
def test_peaks_with_nan_follow_the_nan_rule(S, sigma, d):
    rs = np.random.RandomState(sigma * 10 + d)
    a = surface(3, 300, 400)
    a[rs.rand(*a.shape) < 0.002] = np.nan                          # scattered
    a[100:140, 150:220] = np.nan                                   # clumped
    a[0:3, :] = np.nan
    check_peaks(S, a, 5.0, d, sigma)
    ok = R.nan_free_window(a, d, sigma)
    assert ok.any()
    check_peaks(S, a, 5.0, d, sigma, want=R.peaks_scipy(a, 5.0, d, sigma), where=ok)
    # infinities are values, not nodata
    b = surface(4, 60, 80)
    b[10, 10], b[30, 40] = np.inf, -np.inf
    check_peaks(S, b, 5.0, d, 0, want=R.peaks_scipy(b, 5.0, d, 0))


def test_peaks_all_nan_and_tensor_input(S):
    import torch
    a = np.full((20, 30), np.nan, np.float32)
    assert check_peaks(S, a, -np.inf, 2, 0) == 0
    b = surface(9, 100, 120)
    out = S.detect_peaks(torch.as_tensor(b).cuda(), 10.0, 3, 1)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in out)
    wr, wc = np.where(R.peaks_scipy(b, 10.0, 3, 1))
    assert np.array_equal(out[0].cpu().numpy(), wr) and np.array_equal(out[1].cpu().numpy(), wc)


def test_peaks_large_plane(S):
    rs = np.random.RandomState(1)
    small = rs.rand(512, 512).astype(np.float32) * 30
    a = np.ascontiguousarray(np.kron(small, np.ones((8, 8), np.float32)) + rs.rand(4096, 4096).astype(np.float32))
    assert check_peaks(S, a, 20.0, 3, 1, want=R.peaks_scipy(a, 20.0, 3, 1)) > 1000


def test_make_seeds_tables(S, tmp_path):
    a = surface(21, 150, 200)
    aff = R.pixel_affine(0.5, 150)
    out = S.make_chm_seeds(a, seeds_gpkg=tmp_path / "chm.gpkg", h_min_m=12.0, affine_transformation=aff)
    wr, wc = np.where(R.peaks_scipy(a, 12.0, 3, 1))
    assert np.array_equal(out["row"], wr) and np.array_equal(out["col"], wc) and np.array_equal(out["id"], np.arange(len(wr)))
    assert np.array_equal(out["ch_max"], a[wr, wc])
    assert np.array_equal(out["x"], aff[0] * (wc + 0.5) + aff[1] * (wr + 0.5) + aff[4])
    assert np.array_equal(out["y"], aff[2] * (wc + 0.5) + aff[3] * (wr + 0.5) + aff[5])
    back = S.read_seed_points(tmp_path / "chm.gpkg")
    assert np.array_equal(back["x"], out["x"]) and np.array_equal(back["ch_max"], out["ch_max"].astype(np.float64))
    den = S.make_density_seeds(a, d_min=12.0)
    wr, wc = np.where(R.peaks_scipy(a, 12.0, 4, 2))
    assert np.array_equal(den["row"], wr) and np.array_equal(den["den_max"], a[wr, wc]) and np.array_equal(den["x"], wc + 0.5)
    with pytest.raises(SystemExit, match="No peaks found"):
        S.make_chm_seeds(a, h_min_m=1e9)
    with pytest.raises(SystemExit, match="No density peaks found"):
        S.make_density_seeds(a, d_min=1e9)


# ---------------------------------------------------------------------------------------------------------------- merge
def variants(cost):
    """(name, cost, weight): plain, NaN cost, negative cost, weight 0, negative weight."""
    nan = cost.copy(); nan[5:9, 7:12] = np.nan
    neg = cost - np.float32(0.7)
    return [("plain", cost, WEIGHT), ("nan", nan, WEIGHT), ("negative", neg, WEIGHT), ("weight0", cost, 0.0), ("negweight", cost, -0.4)]


@pytest.mark.parametrize("pixel", [0.5, 1.0])
@pytest.mark.parametrize("n", [1, 2, 63, 65, 300, 512])
def test_pair_distance_is_bit_equal_on_pixel_centres(S, pixel, n):
    xs, ys, cost, aff = R.pixel_centre_case(n, n, 40, 50, pixel)
    if n > 60:
        xs[17], ys[17] = xs[3], ys[3]                             # coincident points
    inv = R.inverse6(aff)
    for name, c, w in variants(cost):
        for thresh in (XY_THRESH, 0.0, 3.0):
            want = R.distance_matrix(xs, ys, c, inv, w, thresh, 12)
            got = S.pair_distances(xs, ys, c, inv, w, thresh, 12)
            assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True), (name, thresh)


@pytest.mark.parametrize("samples", [1, 5, 8, 12, 13, 16, 40])
def test_pair_distance_for_other_sample_counts(S, samples):
    xs, ys, cost, aff = R.pixel_centre_case(samples, 150, 40, 50, 1.0)
    inv = R.inverse6(aff)
    want = R.distance_matrix(xs, ys, cost, inv, WEIGHT, XY_THRESH, samples)
    assert np.array_equal(S.pair_distances(xs, ys, cost, inv, WEIGHT, XY_THRESH, samples), want)


def test_pair_distance_samples_outside_the_raster_are_clipped(S):
    xs, ys, cost, aff = R.pixel_centre_case(2, 80, 30, 30, 1.0)
    xs = xs + np.where(np.arange(80) % 3 == 0, 64.0, 0.0)          # a third of the seeds lie off the raster
    ys = ys - np.where(np.arange(80) % 4 == 0, 48.0, 0.0)
    inv = R.inverse6(aff)
    want = R.distance_matrix(xs, ys, cost, inv, WEIGHT, XY_THRESH, 12)
    assert np.array_equal(S.pair_distances(xs, ys, cost, inv, WEIGHT, XY_THRESH, 12), want)


@pytest.mark.parametrize("pixel,n,H,W", [(1.0, 1, 10, 10), (1.0, 2, 10, 10), (0.5, 64, 20, 30), (1.0, 700, 60, 80), (0.5, 3000, 130, 160)])
def test_clusters_are_the_components_of_the_restated_matrix(S, pixel, n, H, W):
    xs, ys, cost, aff = R.pixel_centre_case(n + 1, n, H, W, pixel)
    inv = R.inverse6(aff)
    cases = variants(cost) if n <= 700 else variants(cost)[:1]
    for name, c, w in cases:
        D = R.distance_matrix(xs, ys, c, inv, w, XY_THRESH, 12)
        for eps in (EPS, 1.0, 2.5):
            want = R.components(D, eps)
            got = S.merge_clusters(xs, ys, c, inv, w, XY_THRESH, eps)
            assert got.dtype == np.int32 and np.array_equal(got, want), (name, eps)
            assert np.array_equal(S.merge_clusters(xs, ys, c, inv, w, XY_THRESH, eps, prune=False), want), (name, eps, "no prune")
    if n >= 700:
        k = R.components(R.distance_matrix(xs, ys, cost, inv, WEIGHT, XY_THRESH, 12), EPS).max() + 1
        assert 1 < k < n


def test_clusters_chain_across_tiles(S):
    # a line of seeds one pixel apart, shuffled: one component that spans every pair tile; then cut in three places
    n = 1000
    order = np.random.RandomState(0).permutation(n)
    xs, ys = order.astype(np.float64) + 0.5, np.full(n, 0.5)
    cost = np.zeros((1, n), np.float32)
    inv = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert not S.merge_clusters(xs, ys, cost, inv, WEIGHT, XY_THRESH, EPS).any()
    xs2 = xs + 5.0 * (order >= 250) + 5.0 * (order >= 500) + 5.0 * (order >= 750)
    D = R.distance_matrix(xs2, ys, np.zeros((1, n + 20), np.float32), inv, WEIGHT, XY_THRESH, 12)
    got = S.merge_clusters(xs2, ys, np.zeros((1, n + 20), np.float32), inv, WEIGHT, XY_THRESH, EPS)
    assert np.array_equal(got, R.components(D, EPS)) and got.max() == 3


@pytest.mark.parametrize("n", [2, 3, 4, 64, 65, 300, 301])       # even and odd pair counts
def test_pair_stats_equal_numpy(S, n):
    xs, ys, cost, aff = R.pixel_centre_case(n + 7, n, 40, 50, 0.5)
    inv = R.inverse6(aff)
    for name, c, w in variants(cost):
        D = R.distance_matrix(xs, ys, c, inv, w, XY_THRESH, 12)
        want = R.triu_stats(D)
        got = S.pair_stats(xs, ys, c, inv, w, XY_THRESH, 12)
        assert all(isinstance(v, np.float32) for v in got)
        assert np.array_equal(np.array(got), np.array(want, np.float32), equal_nan=True), (name, n, got, want)
    if n >= 64:
        assert np.isnan(S.pair_stats(xs, ys, variants(cost)[1][1], inv, WEIGHT, XY_THRESH, 12)).all()


def test_pair_stats_with_negative_distances_and_ties(S):
    xs, ys, cost, aff = R.pixel_centre_case(4, 200, 30, 30, 1.0)
    inv = R.inverse6(aff)
    c = cost - np.float32(3.0)                                     # 1 + w * mean < 0: negative distances
    D = R.distance_matrix(xs, ys, c, inv, 1.0, XY_THRESH, 12)
    assert (D < 0).any()
    assert np.array_equal(np.array(S.pair_stats(xs, ys, c, inv, 1.0, XY_THRESH, 12)), np.array(R.triu_stats(D), np.float32))
    z = np.zeros_like(cost)                                        # lattice distances: many equal values
    D = R.distance_matrix(xs, ys, z, inv, WEIGHT, XY_THRESH, 12)
    assert np.array_equal(np.array(S.pair_stats(xs, ys, z, inv, WEIGHT, XY_THRESH, 12)), np.array(R.triu_stats(D), np.float32))


@pytest.mark.parametrize("seed", ARBITRARY_SEEDS)
def test_arbitrary_coordinates_within_one_ulp_and_equal_clusters(S, seed):
    xs, ys, cost, aff = R.arbitrary_case(seed, ARBITRARY_N)
    inv = R.inverse6(aff)
    D = R.distance_matrix(xs, ys, cost, inv, WEIGHT, XY_THRESH, 12)
    sub = slice(0, 512)
    got = S.pair_distances(xs[sub], ys[sub], cost, inv, WEIGHT, XY_THRESH, 12)
    ulp = R.ulp_distance_f32(got, D[sub, sub])
    print(f"seed {seed}: max ulp distance {ulp.max()}, pairs off by one {(ulp == 1).sum() // 2} of {512 * 511 // 2}")
    assert ulp.max() <= 1
    assert not R.near_threshold(xs, ys, D, EPS, XY_THRESH), "the case generator must keep every decision away from a threshold"
    assert np.array_equal(S.merge_clusters(xs, ys, cost, inv, WEIGHT, XY_THRESH, EPS), R.components(D, EPS))


def test_chain_cost_surface_seeds_canonical(S, capsys, tmp_path):
    import torch
    from obia_amd.cost import make_cost_surface
    rs = np.random.RandomState(5)
    H, W = 160, 200
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    chm = (12 + 8 * np.sin(xx / 6.0) * np.cos(yy / 7.0) + rs.normal(0, 0.4, (H, W))).astype(np.float32)
    den = (6 + 4 * np.sin(xx / 6.0 + 0.3) * np.cos(yy / 7.0) + rs.normal(0, 0.2, (H, W))).astype(np.float32)
    wv3 = np.stack([400 * np.sin(xx / (11 + 3 * c)) * np.cos(yy / (13 + 2 * c)) + 1000 + 50 * c + rs.normal(0, 20, (H, W))
                    for c in range(8)], -1).astype(np.float32)
    aff = R.pixel_affine(0.5, H)
    with pytest.warns(UserWarning):
        cost = make_cost_surface(torch.as_tensor(wv3).cuda(), torch.as_tensor(chm).cuda())
    cs = S.make_chm_seeds(torch.as_tensor(chm).cuda(), h_min_m=2.5, affine_transformation=aff)
    ds = S.make_density_seeds(torch.as_tensor(den).cuda(), d_min=4.5, affine_transformation=aff)
    out = S.make_canonical_seeds(cs, ds, cost, cost_affine=aff, cost_nodata=-9999.0)
    assert all(isinstance(out[k], torch.Tensor) and out[k].is_cuda for k in ("id", "cluster", "ch_max", "x", "y"))
    # the same chain from the restatement, fed with the GPU's cost surface
    cost_h = cost.cpu().numpy()
    cr, cc = np.where(R.peaks_scipy(chm, 2.5, 3, 1))
    dr, dc = np.where(R.peaks_scipy(den, 4.5, 4, 2))
    rows, cols = np.concatenate([cr, dr]), np.concatenate([cc, dc])
    xs = aff[0] * (cols + 0.5) + aff[1] * (rows + 0.5) + aff[4]
    ys = aff[2] * (cols + 0.5) + aff[3] * (rows + 0.5) + aff[5]
    n = len(xs)
    assert len(cr) > 20 and len(dr) > 20
    cost_h[cost_h == -9999.0] = 1
    D = R.distance_matrix(xs, ys, cost_h, R.inverse6(aff), 0.5, 0.8, 12)
    assert np.array_equal(out["x"].cpu().numpy(), xs) and np.array_equal(out["y"].cpu().numpy(), ys)
    assert np.array_equal(out["cluster"].cpu().numpy(), R.components(D, 1.5))
    assert np.array_equal(out["ch_max"].cpu().numpy(), np.concatenate([chm[cr, cc], den[dr, dc]]))
    assert list(out["origin"]) == ["chm"] * len(cr) + ["density"] * len(dr) and np.array_equal(out["id"].cpu().numpy(), np.arange(n))
    lo, med, hi = R.triu_stats(D)
    assert f"d_eff  min/median/max = {lo:.2f} / {med:.2f} / {hi:.2f}" in capsys.readouterr().out
    # NumPy in -> NumPy out, and the written layer
    host = S.make_canonical_seeds({k: v.cpu().numpy() for k, v in cs.items()}, {k: v.cpu().numpy() for k, v in ds.items()}, cost_h,
                                  out_path=tmp_path / "canonical.gpkg", cost_affine=aff, debug_dist=False)
    assert isinstance(host["cluster"], np.ndarray) and np.array_equal(host["cluster"], out["cluster"].cpu().numpy())
    back = S.read_seed_points(tmp_path / "canonical.gpkg")
    assert np.array_equal(back["cluster"], host["cluster"]) and list(back["origin"]) == list(host["origin"])
    assert np.array_equal(back["x"], xs) and np.array_equal(back["y"], ys)
