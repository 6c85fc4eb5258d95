"""The seeds restatement (tests/seeds_restatement.py) against the libraries the reference calls, on the CPU: what the GPU tests
take as their reference is pinned here first."""
import math

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter, maximum_filter

from tests import seeds_restatement as R

ARBITRARY_SEEDS = (11, 12, 13, 14)          # the cases test_gpu_seeds.py compares clusters on
ARBITRARY_N = 700
EPS, XY_THRESH, WEIGHT = 1.5, 0.8, 0.5


@pytest.mark.parametrize("seed", range(6))
def test_components_are_dbscan_labels(seed):
    cluster = pytest.importorskip("sklearn.cluster")
    rs = np.random.RandomState(seed)
    n = 40 + 30 * seed
    D = rs.uniform(0, 12, (n, n)).astype(np.float32)
    D = np.minimum(D, D.T)
    D[rs.rand(n, n) < 0.02] = np.float32(1.5)        # values exactly on eps
    D = np.minimum(D, D.T)
    np.fill_diagonal(D, 0)
    want = cluster.DBSCAN(eps=1.5, min_samples=1, metric="precomputed").fit(D).labels_
    assert np.array_equal(R.components(D, 1.5), want)


def test_components_of_a_real_distance_matrix_are_dbscan_labels():
    cluster = pytest.importorskip("sklearn.cluster")
    xs, ys, cost, aff = R.pixel_centre_case(5, 300, 40, 50, 1.0)
    D = R.distance_matrix(xs, ys, cost, R.inverse6(aff), WEIGHT, XY_THRESH, 12)
    want = cluster.DBSCAN(eps=EPS, min_samples=1, metric="precomputed").fit(D).labels_
    got = R.components(D, EPS)
    assert np.array_equal(got, want) and 1 < got.max() + 1 < 300


@pytest.mark.parametrize("samples", range(1, 17))
def test_written_mean_order_is_numpy_mean(samples):
    rs = np.random.RandomState(samples)
    for _ in range(200):
        a = (rs.rand(samples) * 10.0 ** rs.randint(-3, 4, samples)).astype(np.float32)
        assert R.mean_f32_written_order(a) == a.mean()
        rows = np.ascontiguousarray(np.tile(a, (5, 1)))
        assert np.array_equal(rows.mean(axis=1), np.full(5, a.mean(), np.float32))


@pytest.mark.parametrize("pixel", [0.5, 1.0])
def test_sqrt_of_squares_is_hypot_on_pixel_centres(pixel):
    xs, ys, _, _ = R.pixel_centre_case(3, 600, 700, 900, pixel)
    dx = xs[None, :] - xs[:, None]
    dy = ys[None, :] - ys[:, None]
    got = np.sqrt(dx * dx + dy * dy)
    assert np.array_equal(got.ravel(), R.hypot_py(dx.ravel(), dy.ravel()))
    assert got[5, 77] == math.hypot(dx[5, 77], dy[5, 77])


def nan_plane(seed, H=120, W=150):
    rs = np.random.RandomState(seed)
    a = gaussian_filter(rs.rand(H, W).astype(np.float32) * 30, 2)
    a[rs.rand(H, W) < 0.002] = np.nan
    a[40:52, 60:75] = np.nan
    return a


@pytest.mark.parametrize("sigma,d", [(0, 1), (0, 3), (1, 3), (2, 4)])
def test_nan_rule_is_scipy_wherever_the_window_has_no_nan(sigma, d):
    a = nan_plane(sigma * 10 + d)
    ok = R.nan_free_window(a, d, sigma)
    assert 0 < ok.sum() < ok.size
    assert np.array_equal(R.peaks_nan_rule(a, 5.0, d, sigma)[ok], R.peaks_scipy(a, 5.0, d, sigma)[ok])
    assert not R.peaks_nan_rule(a, -np.inf, d, sigma)[np.isnan(R.smooth(a, sigma))].any()


def test_nan_rule_is_scipy_on_a_nan_free_plane():
    rs = np.random.RandomState(0)
    a = np.round(gaussian_filter(rs.rand(90, 70).astype(np.float32) * 30, 1.5))     # plateaus
    for sigma, d in [(0, 1), (0, 4), (1, 3)]:
        assert np.array_equal(R.peaks_nan_rule(a, 10.0, d, sigma), R.peaks_scipy(a, 10.0, d, sigma))
    g = gaussian_filter(a, 1)
    assert np.array_equal(maximum_filter(g, size=7), maximum_filter(maximum_filter(g, size=(1, 7)), size=(7, 1)))


@pytest.mark.parametrize("weight,thresh", [(0.5, 0.8), (0.0, 0.8), (-0.3, 2.0)])
def test_row_at_a_time_matrix_is_the_loop(weight, thresh):
    xs, ys, cost, aff = R.pixel_centre_case(1, 60, 20, 25, 0.5)
    xs[7], ys[7] = xs[3], ys[3]                        # coincident points
    cost[3, 4] = np.nan
    inv = R.inverse6(aff)
    a = R.distance_matrix_loop(xs, ys, cost, inv, weight, thresh, 12)
    b = R.distance_matrix(xs, ys, cost, inv, weight, thresh, 12)
    assert np.array_equal(a, b, equal_nan=True)
    xs, ys, cost, aff = R.arbitrary_case(2, 50)
    inv = R.inverse6(aff)
    assert np.array_equal(R.distance_matrix_loop(xs, ys, cost, inv, weight, thresh, 5),
                          R.distance_matrix(xs, ys, cost, inv, weight, thresh, 5))


@pytest.mark.parametrize("seed", ARBITRARY_SEEDS)
def test_arbitrary_cases_have_no_decision_near_a_threshold(seed):
    xs, ys, cost, aff = R.arbitrary_case(seed, ARBITRARY_N)
    D = R.distance_matrix(xs, ys, cost, R.inverse6(aff), WEIGHT, XY_THRESH, 12)
    assert not R.near_threshold(xs, ys, D, EPS, XY_THRESH)
    lab = R.components(D, EPS)
    assert 1 < lab.max() + 1 < ARBITRARY_N            # some seeds merge, not all
