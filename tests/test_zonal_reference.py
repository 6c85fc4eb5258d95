"""Pins the float64 zonal-statistics reference (tests/zonal_reference.py) without a GPU: against SciPy's skew / kurtosis on
float64 input, against math.fsum on small cases, against the SciPy golden moments_96x131x5.npz at its 1e-4, and checks
that the bars of the GPU tests reject one dropped or doubled pixel."""
import math
import os

import numpy as np
import pytest
from scipy.stats import kurtosis, skew

from tests.zonal_reference import (EPS32, assert_bars_detect_one_pixel, compare, segment_stats, tolerances,
                                   zonal_reference)

HERE = os.path.dirname(os.path.abspath(__file__))


def _case(seed, H=23, W=31, C=3, nan_frac=0.05):
    rs = np.random.RandomState(seed)
    raw = (rs.gamma(2.0, 40.0, (H, W, C)) + rs.uniform(0, 3000, C)).astype(np.float32)
    raw[rs.rand(H, W, C) < nan_frac] = np.nan
    lab = rs.randint(-1, 9, (H, W)).astype(np.int32)
    return raw, lab


@pytest.mark.parametrize("seed", range(6))
def test_reference_vs_scipy_float64(seed):
    raw, lab = _case(seed)
    ref = zonal_reference(raw, lab, start_label=1, n_labels=9)
    for L in range(9):
        for b in range(raw.shape[2]):
            v = raw[:, :, b][lab == L + 1].astype(np.float64)
            v = v[~np.isnan(v)]
            if v.size == 0:
                assert np.isnan(ref["mean"][L, b]) and np.isnan(ref["skewness"][L, b]) and ref["n"][L, b] == 0
                continue
            assert ref["n"][L, b] == v.size
            assert ref["min"][L, b] == np.float32(v.min()) and ref["max"][L, b] == np.float32(v.max())
            np.testing.assert_allclose(ref["mean"][L, b], v.mean(), rtol=1e-15)
            np.testing.assert_allclose(ref["variance"][L, b], v.var(), rtol=1e-13)
            np.testing.assert_allclose(ref["skewness"][L, b], skew(v), rtol=1e-11, atol=1e-13)
            np.testing.assert_allclose(ref["kurtosis"][L, b], kurtosis(v), rtol=1e-11, atol=1e-13)
    assert np.array_equal(ref["count"], np.bincount(lab.ravel() + 1, minlength=11)[2:11])


def test_reference_vs_fsum_small():
    rs = np.random.RandomState(3)
    # values with a large common offset: the sums that cancel in a one-pass formula
    for off, spread, n in ((4e6, 1.0, 300), (60000.0, 0.5, 200), (1000.0, 30.0, 57), (0.0, 1e-3, 11)):
        v = (off + rs.uniform(-spread, spread, n)).astype(np.float32).astype(np.float64)
        raw = v.reshape(1, n, 1).astype(np.float32)
        ref = zonal_reference(raw, np.ones((1, n), np.int32))
        mean = math.fsum(v) / n
        d = [x - mean for x in v]
        m2 = math.fsum(x * x for x in d) / n
        m3 = math.fsum(x ** 3 for x in d) / n
        m4 = math.fsum(x ** 4 for x in d) / n
        np.testing.assert_allclose(ref["mean"][0, 0], mean, rtol=4e-16)
        np.testing.assert_allclose(ref["variance"][0, 0], m2, rtol=1e-13)
        if not m2 <= (EPS32 * mean) ** 2:
            np.testing.assert_allclose(ref["skewness"][0, 0], m3 / m2 ** 1.5, rtol=1e-11, atol=1e-14)
            np.testing.assert_allclose(ref["kurtosis"][0, 0], m4 / m2 ** 2 - 3.0, rtol=1e-11, atol=1e-14)
        st = segment_stats(v)
        for k in ("mean", "variance", "skewness", "kurtosis"):
            np.testing.assert_allclose(st[k], ref[k][0, 0], rtol=1e-12, atol=1e-14, equal_nan=True)


def test_reference_vs_scipy_golden():
    z = np.load(os.path.join(HERE, "golden", "moments_96x131x5.npz"))
    raw = z["dn"].astype(np.float32)
    nanmask = np.unpackbits(z["nanmask"])[:raw.size].reshape(raw.shape).astype(bool)
    raw[nanmask] = np.nan
    ref = zonal_reference(raw, z["labels"])
    for k in ("skewness", "kurtosis"):
        assert np.array_equal(np.isnan(ref[k]), np.isnan(z[k]))
        np.testing.assert_allclose(ref[k], z[k], rtol=1e-4, atol=1e-4, equal_nan=True)
    assert not ref["near_threshold"].any()


def test_constant_and_threshold_rules():
    raw = np.zeros((2, 8, 2), np.float32)
    raw[:, :4, 0] = 1234.0                                   # label 1, band 0: constant
    raw[:, :4, 1] = np.nan                                   # label 1, band 1: no valid pixel
    raw[:, 4:, 0] = np.float32(60000.0)                      # label 2, band 0: nearly constant, one ulp apart
    raw[0, 4, 0] = np.nextafter(np.float32(60000.0), np.float32(np.inf))
    raw[:, 4:, 1] = np.arange(8).reshape(2, 4)
    lab = np.repeat([[1] * 4 + [2] * 4], 2, 0).astype(np.int32)
    ref = zonal_reference(raw, lab)
    assert ref["variance"][0, 0] == 0.0 and np.isnan(ref["skewness"][0, 0]) and np.isnan(ref["kurtosis"][0, 0])
    assert ref["n"][0, 1] == 0 and np.isnan(ref["mean"][0, 1]) and np.isnan(ref["min"][0, 1])
    # one pixel one ulp (2^-8 at 60000) above seven others: m2 = 7/64 * 2^-16 < (eps * mean)^2 -> NaN
    assert ref["variance"][1, 0] > 0 and np.isnan(ref["skewness"][1, 0])
    assert np.isfinite(ref["skewness"][1, 1])
    # a segment placed exactly on the threshold is flagged
    t = EPS32 * 1024.0                                         # one float32 ulp at 1024
    v = np.array([1024.0 - t, 1024.0 + t], np.float64)        # m2 = t^2 = (eps * mean)^2 exactly
    raw2 = v.reshape(1, 2, 1).astype(np.float32)
    r2 = zonal_reference(raw2, np.ones((1, 2), np.int32))
    m2 = r2["m2"][0, 0]
    assert m2 == (EPS32 * r2["mean"][0, 0]) ** 2 and r2["near_threshold"][0, 0] and np.isnan(r2["skewness"][0, 0])


def test_labels_out_of_range_and_n_labels():
    raw, lab = _case(11, C=2, nan_frac=0.0)
    lab = lab - 1                                             # -2 .. 7
    ref0 = zonal_reference(raw, lab, start_label=0, n_labels=5)    # labels 5..7 and < 0 ignored
    assert ref0["count"].tolist() == [int((lab == i).sum()) for i in range(5)]
    ref1 = zonal_reference(raw, lab, start_label=0, n_labels=12)   # larger than the largest label: empty rows
    assert np.all(ref1["count"][8:] == 0) and np.isnan(ref1["mean"][8:]).all()
    np.testing.assert_array_equal(ref1["mean"][:5], ref0["mean"])


@pytest.mark.parametrize("moments", [False, True])
def test_bars_reject_one_pixel(moments):
    raw, lab = _case(5, H=40, W=50, C=4)
    ref = zonal_reference(raw, lab)
    tol = tolerances(ref)
    assert not compare(ref, ref, tol, moments=moments)
    assert_bars_detect_one_pixel(raw, lab, ref, tol, moments=moments)
    # and a result computed in float32 (NumPy's own arithmetic on the raster dtype) is rejected on the mean
    got = dict(ref)
    got["mean"] = ref["mean"].astype(np.float32).astype(np.float64) + ref["mean"] * 2e-7
    assert compare(got, ref, tol)
