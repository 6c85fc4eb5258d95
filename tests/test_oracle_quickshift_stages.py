"""The oracle pieces the quickshift stage tests stand on (CPU only): obia_oracle_quickshift_stages computes what the pinned
core computes, rgb2lab_f64 is scikit-image's float64 Lab conversion, and the near-tie flags mark what they say they mark."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden")

# The fixtures were written by a NumPy whose pow / cbrt differ from this one's in the last bit here and there; the a channel
# (500 * (x - y)) turns one ulp of x or y into 500 ulp(1) = 1.1e-13: measured 1.67e-13 = 11.8 ulp of max |Lab| (98.4).  Bar: 16 ulp.
LAB_ULPS = 16


def _noise(shape):
    return np.random.RandomState(42).normal(scale=0.00001, size=shape[:2])


def test_stage_labels_equal_core_labels_on_the_goldens(oracle):
    z = np.load(os.path.join(GOLD, "quickshift_small.npz"))
    for i in range(3):
        ks, md = z[f"par{i}"]
        img = z[f"lab{i}"] * 1.0
        st = oracle.quickshift_stages(img, _noise(img.shape), ks, md)
        assert np.array_equal(st["labels"], oracle.quickshift_core(img, _noise(img.shape), ks, md))
        assert np.array_equal(st["labels"], z[f"labels{i}"])
    z = np.load(os.path.join(GOLD, "quickshift_sigma.npz"))
    for i in range(3):
        ks, md, _sg, ratio, _lab = z[f"par{i}"]
        img = z[f"smoothed{i}"] * ratio
        st = oracle.quickshift_stages(img, _noise(img.shape), ks, md)
        assert np.array_equal(st["labels"], oracle.quickshift_core(img, _noise(img.shape), ks, md))
        assert np.array_equal(st["labels"], z[f"labels{i}"])
        # the stages hang together: roots flatten the cut parents, every link climbs to a higher density
        n = img.shape[0] * img.shape[1]
        idx = np.arange(n)
        par = st["parent"].reshape(-1)
        dp = st["dist_parent"].reshape(-1)
        cut = np.where(dp > md, idx, par)
        roots = st["roots"].reshape(-1)
        assert np.array_equal(roots[roots], roots) and np.array_equal(roots[cut], roots)
        link = par != idx
        assert (st["dens"].reshape(-1)[par[link]] > st["dens"].reshape(-1)[link]).all()
        assert np.isinf(dp[~link]).all() and np.isfinite(dp[link]).all()


def test_rgb2lab_f64_matches_the_fixtures(oracle):
    z = np.load(os.path.join(GOLD, "quickshift_small.npz"))
    cases = [(z[f"raw{i}"], z[f"lab{i}"]) for i in range(3)]
    z = np.load(os.path.join(GOLD, "quickshift_sigma.npz"))
    cases += [(z[f"raw{i}"], z[f"feat{i}"]) for i in range(3) if z[f"par{i}"][4]]
    assert len(cases) == 4
    for raw, ref in cases:
        img = oracle.normalize(raw.astype(np.float32)).astype(np.float64)
        lab = oracle.rgb2lab_f64(img)
        err = np.abs(lab - ref).max()
        assert err <= LAB_ULPS * np.spacing(np.abs(ref).max()), f"max |diff| {err:.3g}"
        assert (lab == ref).mean() > 0.4          # most values to the bit


def test_tie_flags_on_hand_made_cases(oracle):
    # a constant row, no noise: pixels 3, 4, 5 see the whole window in the same order -> bitwise equal densities (bit 0)
    img = np.full((1, 9, 1), 0.5)
    st = oracle.quickshift_stages(img, np.zeros((1, 9)), 1.0, 10.0)
    assert ((st["flags"][0, 3:6] & 1) != 0).all()
    assert ((st["flags"][0, [0, 8]] & 1) == 0).all()
    # densities climb away from the centre: pixel 4 has two higher neighbours at squared distance 1 (bit 1); the first in
    # scan order wins; max_dist exactly 1.0 flags the cut (bit 2) and keeps the link (the cut is `>`)
    noise = (1e-3 * np.abs(np.arange(9) - 4.0) + 1e-4 * np.arange(9))[None, :]
    st = oracle.quickshift_stages(img, noise, 1.0, 1.0)
    assert st["flags"][0, 4] & 2 and st["parent"][0, 4] == 3 and st["dist_parent"][0, 4] == 1.0
    assert st["flags"][0, 4] & 4 and st["roots"][0, 4] != 4
    assert not (st["flags"] & 1).any()
    st = oracle.quickshift_stages(img, noise, 1.0, 0.999)
    assert not (st["flags"][0, 4] & 4) and st["roots"][0, 4] == 4
    # texture and tie noise: nothing flagged; the flags follow tau
    rs = np.random.RandomState(0)
    img = rs.uniform(size=(20, 23, 3))
    noise = rs.normal(scale=1e-5, size=(20, 23))
    st = oracle.quickshift_stages(img, noise, 2.0, 6.0)
    assert not st["flags"].any()
    assert (oracle.quickshift_stages(img, noise, 2.0, 6.0, tau=1.0)["flags"] & 1).all()
    # the pixel without a higher neighbour is its own parent at +inf
    top = np.unravel_index(np.argmax(st["dens"]), st["dens"].shape)
    assert st["parent"][top] == top[0] * 23 + top[1] and np.isinf(st["dist_parent"][top])
