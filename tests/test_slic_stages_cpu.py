"""The references of tests/slic_stages.py, validated on the oracle's own chain before they judge a kernel (no GPU): the float64 sweep
agrees with the oracle's C sweep wherever it is binding, near ties stay under the cap the GPU test relies on, the float64 centroid
means hold the oracle's integer-sum centroids inside the derived bound, and the float32 feature chain reproduces scipy's smoothed
images bit for bit."""
import glob
import os

import numpy as np
import pytest

from tests import slic_stages as S


def oracle_chain(oracle, case):
    """Features, seeds and, sweep by sweep, (pass, N, centroids the sweep assigns from, its labels, centroids after its update) of the
    oracle in the library's sum mode -- the sweeps of a masked case are its pre-pass, then the colour pass.  One call of the core per
    sweep: labels start from the fill value every time, so an orphan of sweep n > 1 drops out of the update where a real run of n
    sweeps would keep its earlier label.  Good enough to validate the references on, not the chain a run follows."""
    img, mask, seeds = S.make_inputs(case)
    feat = S.features_ref32(oracle, img, case)
    yx, step = S.reference_seeds(oracle, case, mask, seeds)
    seg = S.initial_segments(yx, feat.shape[2])
    sp = None if case["spacing"] is None else (case["spacing"][1], case["spacing"][2])
    sweeps = []
    oracle.set_sum_mode(1)
    try:
        for ignore_color in ([True, False] if mask is not None else [False]):
            for n in range(1, case["iters"] + 1):
                before = seg.copy()
                lab = oracle.slic_core(feat, seg, step, max_iter=1, mask=mask, ignore_color=ignore_color, start_label=case["start_label"],
                                       spacing_yx=sp)
                sweeps.append((ignore_color, n, before, lab, seg.copy()))
    finally:
        oracle.set_sum_mode(0)
    return img, mask, feat, step, sweeps


@pytest.mark.parametrize("case", S.FIXED_CASES, ids=lambda c: c["name"])
def test_references_agree_with_the_oracle_chain(oracle, case):
    img, mask, feat, step, sweeps = oracle_chain(oracle, case)
    H, W, C = feat.shape
    valid = np.ones((H, W), bool) if mask is None else mask != 0
    fscale = S.expected_fscale(feat)
    for ignore_color, n, cent, lab, cent_next in sweeps:
        tag = f"{case['name']}: {'pre-pass' if ignore_color else 'colour'} sweep {n}"
        ref64, gap = S.sweep_ref64(oracle, feat, cent, step, mask=mask, ignore_color=ignore_color, start_label=case["start_label"],
                                   spacing=case["spacing"])
        # the same pixels are reached
        assert np.array_equal(ref64 == case["start_label"] - 1, lab == case["start_label"] - 1), tag
        if not ignore_color:
            wrong, near = S.judge_sweep64(lab, ref64, gap, C, valid)
            assert wrong == 0, f"{tag}: {wrong} px where the float64 winner is binding and the oracle disagrees"
            assert near <= S.NEAR_TIE_CAP or not S.cap_applies(case, mask, n, feat, step), f"{tag}: {near:.3%} of the valid pixels are near ties"
        else:   # spatial only: distances of small rationals, exact ties everywhere; the lowest k wins them
            wrong, _ = S.judge_sweep64(lab, ref64, gap, 0, valid)
            assert wrong == 0, f"{tag}: {wrong} px where the float64 winner is binding and the oracle disagrees"
        mean, cnt = S.centroid_ref64(feat, lab, mask, cent.shape[0], case["start_label"])
        assert np.array_equal(np.isnan(mean), np.isnan(cent_next)), tag
        ok = ~np.isnan(mean)
        err = np.abs(cent_next.astype(np.float64) - mean)
        bound = S.centroid_bounds(mean, fscale)
        assert (err[ok] <= bound[ok]).all(), f"{tag}: centroid off by {np.nanmax(err / bound):.3f} of the bound"


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(S.GOLD, "sigma*.npz"))), ids=os.path.basename)
def test_features_ref32_reproduces_scipy_smoothed(oracle, path):
    z = np.load(path)
    raw = z["raw"].astype(np.float32)
    sig = float(z["sigma_arg"]) if z["sigma_arg"].shape == () else [float(v) for v in z["sigma_arg"]]
    sp = [float(v) for v in z["spacing_zyx"]]
    case = dict(normalize=True, lab=raw.shape[2] == 3, sigma=sig, spacing=None if sp == [1.0, 1.0, 1.0] else sp, compactness=1.0)
    got = S.features_ref32(oracle, raw, case)       # compactness 1: `* float32(1)` changes no bit
    if case["lab"]:   # NumPy's float32 pow / cbrt are not glibc's: the Lab goldens are pinned within float32 rounding, not bitwise
        np.testing.assert_allclose(got, z["smoothed"], rtol=0, atol=2e-4)
    else:
        assert np.array_equal(got.view(np.uint32), z["smoothed"].view(np.uint32))


@pytest.mark.parametrize("case", [c for c in S.FIXED_CASES if c["lab"]] + [S._case("uniform_129x257", 129, 257, 3, 80, 1.0, lab=True, norm=False)],
                         ids=lambda c: c["name"])
def test_lab_float32_error_is_reported(oracle, case, capsys):
    """The yardstick of Stage A on Lab input: how far the oracle's float32 chain is from float64, per channel (printed)."""
    if case["name"].startswith("uniform"):
        img = np.random.RandomState(0).rand(129, 257, 3).astype(np.float32)
    else:
        img = S.make_inputs(case)[0]
    e = np.abs(S.features_ref32(oracle, img, case).astype(np.float64) - S.features_ref64(oracle, img, case)).reshape(-1, 3).max(0)
    with capsys.disabled():
        print(f"\n  {case['name']}: float32 chain vs float64, max |diff| L / a / b = {e[0]:.2e} / {e[1]:.2e} / {e[2]:.2e} "
              f"(features span {np.abs(S.features_ref64(oracle, img, case)).max():.3g})")
    assert np.isfinite(e).all() and (e < 1e-3 * max(1.0, 1.0 / case["compactness"])).all()
