"""Cost surface, host side: known answers for the CPU restatement (tests/cost_restatement.py) and the argument checks of
obia_amd.cost that fire before any device work."""
import math
import warnings

import numpy as np
import pytest

from tests import cost_restatement as R


def test_constant_image_has_zero_entropy():
    assert np.array_equal(R.rank_entropy(np.full((9, 11), 77, np.uint8)), np.zeros((9, 11)))


def test_all_distinct_taps_give_the_29_term_sum():
    u8 = np.arange(49, dtype=np.uint8).reshape(7, 7) * 5
    e = R.rank_entropy(u8)
    want = 0.0
    for _ in range(29):
        p = 1 / 29.0
        want -= p * math.log(p) / R.LN2
    assert e[3, 3] == want
    assert abs(e[3, 3] - math.log2(29)) < 1e-12


def test_corner_population_is_11():
    u8 = np.zeros((10, 10), np.uint8)
    u8[0, 0] = 1                                      # one of 11 taps differs at the corner
    p = 1 / 11
    want = -((10 / 11) * math.log(10 / 11) / R.LN2) - (p * math.log(p) / R.LN2)
    assert R.rank_entropy(u8)[0, 0] == want
    pad = np.full((16, 16), -1); pad[3:13, 3:13] = 0
    assert sum(1 for dy, dx in R.DISK3 if pad[3 + dy, 3 + dx] == 0) == 11


@pytest.mark.parametrize("seed,levels", [(0, 256), (1, 3), (2, 12)])
def test_vectorised_entropy_matches_the_direct_loop(seed, levels):
    rs = np.random.RandomState(seed)
    u8 = (rs.randint(0, levels, (13, 17)) * (255 // max(levels - 1, 1))).astype(np.uint8)
    assert np.array_equal(R.rank_entropy(u8, rows=5), R.rank_entropy_loop(u8))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_percentile_restatement_is_bit_identical_to_numpy(dtype):
    rs = np.random.RandomState(3)
    for n in range(1, 301):
        kind = n % 3
        if kind == 0:
            a = rs.standard_normal(n)
        elif kind == 1:
            a = rs.randint(0, 4, n).astype(np.float64) - 1.5          # ties
        else:
            a = rs.standard_normal(n) * 1e-40                          # subnormal in float32
        a = a.astype(dtype)
        a[rs.rand(n) < 0.2] = np.nan
        q = np.concatenate([Q_STD, rs.rand(4)])
        if np.isnan(a).all():
            continue
        got = R.percentiles(a, q)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = np.nanpercentile(a, 100 * q)
        # q * 100 / 100 need not round-trip: compare against NumPy's own virtual index from the same q
        want_q = np.nanquantile(a, q)
        assert got.dtype == want_q.dtype
        assert np.array_equal(got.view(np.uint64), want_q.view(np.uint64)), (n, q)
        assert np.array_equal(got[:2], want[:2])


Q_STD = np.true_divide((2, 98), 100.0)


def test_normalise_promotes_float32_to_float64():
    a = np.linspace(0, 1, 50, dtype=np.float32)
    assert R.normalise(a).dtype == np.float64
    assert np.array_equal(R.normalise(np.full(5, 3, np.float32)), np.zeros(5))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        z = R.normalise(np.full(4, np.nan, np.float32))
    assert z.dtype == np.float32 and not z.any()       # all NaN: float32 NaN percentiles, nothing promotes


def test_restated_surface_small_case_properties():
    rs = np.random.RandomState(4)
    wv3 = rs.uniform(1, 1000, (20, 23, 8)).astype(np.float32)
    chm = rs.uniform(0, 30, (20, 23)).astype(np.float32)
    chm[3:6, 4:9] = np.nan
    lab = (np.arange(20)[:, None] // 5 * 10 + np.arange(23)[None] // 6).astype(np.int32)
    c = R.make_cost_surface(wv3, chm, lab, (0.4, 0.3, 0.2, 0.1))
    assert c.dtype == np.float32 and c.shape == (20, 23) and (c >= 0).all() and (c <= 1).all()


# ------------------------------------------------------------------------------------- obia_amd.cost argument checks
def _inputs(H=6, W=7):
    return np.zeros((H, W, 8), np.float32), np.zeros((H, W), np.float32)


def test_weights_must_sum_to_one():
    from obia_amd.cost import make_cost_surface
    wv3, chm = _inputs()
    with pytest.raises(SystemExit, match="Weights must sum to 1."):
        make_cost_surface(wv3, chm, weights=(0.5, 0.5, 0.5, 0))


@pytest.mark.parametrize("bands", [3, 4, 7, 9])
def test_band_count_is_checked(bands):
    from obia_amd.cost import make_cost_surface
    with pytest.raises(ValueError, match="8"):
        make_cost_surface(np.zeros((6, 7, bands), np.float32), np.zeros((6, 7), np.float32), slic=np.zeros((6, 7), np.int32))


def test_shapes_are_checked():
    from obia_amd.cost import make_cost_surface
    wv3, chm = _inputs()
    with pytest.raises(ValueError, match="chm"):
        make_cost_surface(wv3, chm[:5], slic=np.zeros((6, 7), np.int32))
    with pytest.raises(ValueError, match="slic"):
        make_cost_surface(wv3, chm, slic=np.zeros((6, 8), np.int32))
    with pytest.raises(ValueError):
        make_cost_surface(np.zeros((6, 7), np.float32), chm, slic=np.zeros((6, 7), np.int32))


def test_gpkg_slic_is_not_implemented():
    from obia_amd.cost import make_cost_surface
    wv3, chm = _inputs()
    with pytest.raises(NotImplementedError, match="label raster"):
        make_cost_surface(wv3, chm, slic="segments.GPKG")


def test_entropy_term_table_matches_the_restatement():
    from obia_amd.cost import entropy_table
    assert np.array_equal(entropy_table(), R.term_table())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_path_interpolation_matches_numpy(dtype):
    """obia_amd.cost._lerp turns the four order statistics the device selects into np.nanpercentile(x, (2, 98))."""
    from obia_amd.cost import _lerp
    rs = np.random.RandomState(5)
    for n in list(range(1, 301)) + [1000, 4097, 65537]:
        a = (rs.randint(0, 5, n) if n % 2 else rs.standard_normal(n) * 10.0 ** rs.randint(-42, 30)).astype(dtype)
        a[rs.rand(n) < 0.1] = np.nan
        v = np.sort(a[~np.isnan(a)])
        m = v.size
        if m == 0:
            continue
        vi = (m - 1) * Q_STD
        ia = np.where(vi >= m - 1, m - 1, np.floor(vi)).astype(np.int64)
        ib = np.where(vi >= m - 1, m - 1, ia + 1)
        got = _lerp(m, v[ia], v[ib], dtype)
        want = np.nanpercentile(a, (2, 98))
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint64), want.view(np.uint64)), n
