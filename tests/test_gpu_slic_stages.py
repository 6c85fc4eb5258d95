"""SLIC stage by stage on the GPU (obia_slic_stages_f32_dev, the function behind slic(..., _stage="pre")), each stage against its own
reference (tests/slic_stages.py; the references themselves are validated by tests/test_slic_stages_cpu.py):

  A  features   no Lab: bit-equal to the float32 restatement.  Lab: per channel  max |device - float64|  <=  2 x max |oracle float32 -
                float64|  on the same input (the factor: device powf / cbrtf against glibc's, amplified by 500 * (fx - fy)).
  B  one sweep  the labels of sweep N equal the reference's sweep from the DEVICE's features and centroids at every pixel, N in
                {1, 2, max_num_iter}; an orphan (a valid pixel no window reaches) keeps the label of sweep N - 1, the fill value at
                N = 1.  Second opinion in float64, independent of the oracle's C code, wherever its gap is binding.
  C  the update centroids of sweep N + 1 against the float64 means over the labels of sweep N, inside the derived bound
                (slic_stages.centroid_bounds); same NaN pattern; without Lab bit-equal to the oracle in the library's sum mode.
  D  the ends   seeds, initial centroids, labels_pre == slic(_stage="pre"), exit_on_fixed_point changes nothing.

A run with max_num_iter = N hands out the centroids and labels of sweep N.  Masked cases: `prepass_only` runs hand out sweep N of the
spatial pre-pass; full runs hand out colour sweep N after a pre-pass of `prepass_iters` = M sweeps (M = the case's max_num_iter, the
pre-pass slic() itself runs), so that colour sweeps N - 1, N and N + 1 follow the SAME pre-pass and chain like those of an unmasked
case."""
import functools
import os

import numpy as np
import pytest

from tests import slic_stages as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = S.FIXED_CASES + [S.random_case(i) for i in range(int(os.environ.get("OBIA_RANDOM_SLIC_STAGE_CASES", "24")))]
BY_NAME = {c["name"]: c for c in CASES}
case_param = pytest.mark.parametrize("name", [c["name"] for c in CASES])


@functools.lru_cache(maxsize=None)
def inputs(name):
    img, mask, seeds = S.make_inputs(BY_NAME[name])
    img.setflags(write=False)
    return img, mask, seeds


@functools.lru_cache(maxsize=None)
def run(name, n, prepass_only=False, exit_on_fixed_point=False):
    """Stage outputs of the case with max_num_iter = n, on the host; computed once and shared (read-only).  A full run of a masked case
    has the pre-pass of the case's own max_num_iter, whatever n is."""
    from obia_amd.segmentation import _slic_stages
    case = BY_NAME[name]
    img, mask, seeds = inputs(name)
    old = os.environ.pop("OBIA_PREP_GROUPED", None)
    if case["grouped"]:
        os.environ["OBIA_PREP_GROUPED"] = "1"
    try:
        g = _slic_stages(torch.as_tensor(img).cuda(), max_num_iter=n, prepass_only=prepass_only, exit_on_fixed_point=exit_on_fixed_point,
                         prepass_iters=0 if (mask is None or prepass_only) else case["iters"], **S.slic_kwargs(case, mask, seeds))
    finally:
        os.environ.pop("OBIA_PREP_GROUPED", None)
        if old is not None:
            os.environ["OBIA_PREP_GROUPED"] = old
    out = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in g.items()}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def sweeps_of(case):
    return sorted({1, 2, case["iters"]})


def passes_of(case, mask):
    """(prepass_only, ignore_color) of the passes whose sweeps can be handed out."""
    return [(True, True), (False, False)] if mask is not None else [(False, False)]


# ---- Stage A -------------------------------------------------------------------------------------------------------------------
@case_param
def test_stage_a_features(oracle, name):
    case = BY_NAME[name]
    img, mask, seeds = inputs(name)
    g = run(name, 1)
    dev = g["features"]
    ref32 = S.features_ref32(oracle, img, case)
    # the power of two folded into the planes: known beforehand only for normalised bands without Lab and without SLIC-zero
    ps = g["prescale"]
    assert ps > 0 and np.frexp(ps)[0] == 0.5, f"prescale {ps} is not a power of two"
    if case["lab"] or case["slic_zero"] or not case["normalize"]:
        assert ps == 1.0
    assert g["fscale"] == S.expected_fscale(dev), f"fscale {g['fscale']} against max |feature| {np.abs(dev).max()}"
    if not case["lab"]:
        diff = dev.view(np.uint32) != ref32.view(np.uint32)
        assert not diff.any(), (f"{name}: {int(diff.sum())} features differ from the float32 reference, "
                                f"max |diff| {np.abs(dev.astype(np.float64) - ref32).max():.3e}")
        return
    ref64 = S.features_ref64(oracle, img, case)
    e_dev = np.abs(dev.astype(np.float64) - ref64).reshape(-1, 3).max(0)
    e_ref = np.abs(ref32.astype(np.float64) - ref64).reshape(-1, 3).max(0)
    msg = (f"{name}: max |x - float64| per channel L / a / b: device {e_dev[0]:.3e} / {e_dev[1]:.3e} / {e_dev[2]:.3e}, "
           f"oracle float32 {e_ref[0]:.3e} / {e_ref[1]:.3e} / {e_ref[2]:.3e}")
    print(msg)
    assert (e_dev <= 2.0 * e_ref).all(), msg


# ---- Stage B -------------------------------------------------------------------------------------------------------------------
@case_param
def test_stage_b_one_sweep(oracle, name):
    case = BY_NAME[name]
    img, mask, seeds = inputs(name)
    fill = case["start_label"] - 1
    C = case["C"]
    valid = np.ones(img.shape[:2], bool) if mask is None else mask != 0
    for prepass_only, ignore_color in passes_of(case, mask):
        # SLIC-zero: only sweep 1 of the colour pass, where the per-cluster scale is still 1 (the pre-pass has no colour term at all)
        ns = [1] if (case["slic_zero"] and not ignore_color) else sweeps_of(case)
        for n in ns:
            g = run(name, n, prepass_only)
            tag = f"{name}: {'pre-pass' if ignore_color else 'colour'} sweep {n}"
            lab = g["labels_pre"].astype(np.int64)
            kw = dict(mask=mask, ignore_color=ignore_color, start_label=case["start_label"], spacing=case["spacing"])
            ref = S.sweep_ref32(oracle, g["features"], g["centroids"], g["step"], slic_zero=case["slic_zero"] and not ignore_color, **kw)
            assert (lab[~valid] == fill).all(), f"{tag}: masked pixels must carry {fill}"
            orphan = valid & (ref == fill)
            bad = valid & ~orphan & (lab != ref)
            assert not bad.any(), f"{tag}: {int(bad.sum())} px differ from the reference's sweep, first at {tuple(np.argwhere(bad)[0])}"
            if orphan.any():
                if n == 1:
                    assert (lab[orphan] == fill).all(), f"{tag}: an orphan of the first sweep keeps the fill value"
                else:   # (a colour sweep of a masked case: sweep N - 1 after the same pre-pass)
                    prev = run(name, n - 1, prepass_only)["labels_pre"]
                    assert np.array_equal(lab[orphan], prev[orphan]), f"{tag}: an orphan keeps its label of sweep {n - 1}"
            ref64, gap = S.sweep_ref64(oracle, g["features"], g["centroids"], g["step"], **kw)
            wrong, near = S.judge_sweep64(lab, ref64, gap, 0 if ignore_color else C, valid & ~orphan)
            assert wrong == 0, f"{tag}: {wrong} px where the float64 winner is binding and the device disagrees"
            if not ignore_color and S.cap_applies(case, mask, n, g["features"], g["step"]):
                assert near <= S.NEAR_TIE_CAP, f"{tag}: {near:.3%} of the valid pixels are near ties: the case does not test the sweep"


# ---- Stage C -------------------------------------------------------------------------------------------------------------------
def check_update(tag, cent_next, feat, labels, mask, case, fscale, columns=slice(None)):
    mean, cnt = S.centroid_ref64(feat, labels, mask, cent_next.shape[0], case["start_label"])
    assert np.array_equal(np.isnan(cent_next), np.isnan(mean)), f"{tag}: NaN pattern (a centroid without a pixel is 0 / 0)"
    bound = S.centroid_bounds(mean, fscale)[:, columns]
    err = np.abs(cent_next.astype(np.float64) - mean)[:, columns]
    ok = ~np.isnan(err)
    assert (err[ok] <= bound[ok]).all(), f"{tag}: centroid off by {np.nanmax(err / bound):.3f} of the bound (worst |diff| {np.nanmax(err):.3e})"


# (SLIC-zero carries a per-cluster scale from sweep to sweep: only its first colour sweep stands alone, Stage B)
@pytest.mark.parametrize("name", [c["name"] for c in CASES if not c["slic_zero"]])
def test_stage_c_centroid_update(oracle, name):
    case = BY_NAME[name]
    img, mask, seeds = inputs(name)
    M = case["iters"]
    ns = sorted({1, 2, M - 1})
    for n in ns:   # the colour pass (of a masked case: after its pre-pass of M sweeps)
        a, b = run(name, n), run(name, n + 1)
        check_update(f"{name}: centroids of colour sweep {n + 1}", b["centroids"], a["features"], a["labels_pre"], mask, case, a["fscale"])
    if mask is not None:
        # inside the pre-pass: positions (its sweeps fold no colours but the last one, and compare none)
        for n in ns:
            a, b = run(name, n, True), run(name, n + 1, True)
            check_update(f"{name}: centroids of pre-pass sweep {n + 1}", b["centroids"], a["features"], a["labels_pre"], mask, case,
                         a["fscale"], columns=slice(0, 2))
        # the hand-over: the last pre-pass sweep folds the colours the colour pass starts from
        a, b = run(name, M, True), run(name, 1)
        check_update(f"{name}: centroids of colour sweep 1", b["centroids"], a["features"], a["labels_pre"], mask, case, a["fscale"])
    if case["lab"]:
        return
    # Without Lab the features are the oracle's bit for bit (Stage A), and so are the integer sums: in the library's sum mode the
    # oracle's centroids after N sweeps are the ones sweep N + 1 assigns from, bit for bit.
    same = lambda x, y: np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))   # noqa: E731
    oracle.set_sum_mode(1)
    try:
        if mask is None:
            ref_in = oracle.normalize(img) if case["normalize"] else np.asarray(img)
            for n in ns:
                cent = oracle.slic(ref_in, n_segments=S.n_segments(case, mask), compactness=case["compactness"], max_iter=n, convert2lab=False,
                                   start_label=case["start_label"], sigma=case["sigma"], spacing=case["spacing"], enforce_connectivity=False,
                                   return_all=True)[2]
                assert same(run(name, n + 1)["centroids"], cent), f"{name}: centroids of sweep {n + 1} differ from the oracle's integer-sum centroids"
            return
        # masked: the two calls of _slic_cython chained on the device's features (the oracle's own, Stage A) -- the pre-pass from the
        # initial segments, then the colour pass from what M pre-pass sweeps left (oracle.slic would tie both passes to one count)
        feat = run(name, 1)["features"]
        yx, step = S.reference_seeds(oracle, case, mask, seeds)
        sp = None if case["spacing"] is None else (case["spacing"][1], case["spacing"][2])
        kw = dict(mask=mask, start_label=case["start_label"], spacing_yx=sp)
        for n in ns:
            seg = S.initial_segments(yx, case["C"])
            oracle.slic_core(feat, seg, step, max_iter=n, ignore_color=True, **kw)
            assert same(run(name, n + 1, True)["centroids"][:, :2], seg[:, :2]), f"{name}: positions of pre-pass sweep {n + 1} differ from the oracle's"
        start = S.initial_segments(yx, case["C"])
        oracle.slic_core(feat, start, step, max_iter=M, ignore_color=True, **kw)
        assert same(run(name, 1)["centroids"], start), f"{name}: centroids of colour sweep 1 differ from the oracle's after its pre-pass"
        for n in ns:
            seg = start.copy()
            oracle.slic_core(feat, seg, step, max_iter=n, **kw)
            assert same(run(name, n + 1)["centroids"], seg), f"{name}: centroids of colour sweep {n + 1} differ from the oracle's integer-sum centroids"
    finally:
        oracle.set_sum_mode(0)


# ---- Stage D -------------------------------------------------------------------------------------------------------------------
@case_param
def test_stage_d_ends_of_the_chain(oracle, name):
    from obia_amd.segmentation import slic
    case = BY_NAME[name]
    img, mask, seeds = inputs(name)
    M = case["iters"]
    first = run(name, 1, mask is not None)
    yx, step = S.reference_seeds(oracle, case, mask, seeds)
    assert first["K"] == len(yx) and np.array_equal(first["seeds_yx"], yx), f"{name}: seeds"
    assert first["step"] == float(step)
    # the reference's initial segments: the seed positions and ZERO colours (slic_superpixels.py: np.zeros((K, C)))
    assert np.array_equal(first["centroids"].view(np.uint32), S.initial_segments(yx, case["C"]).view(np.uint32)), f"{name}: initial centroids"
    full = run(name, M)
    old = os.environ.pop("OBIA_PREP_GROUPED", None)
    try:
        if case["grouped"]:
            os.environ["OBIA_PREP_GROUPED"] = "1"
        kw = S.slic_kwargs(case, mask, seeds)
        pre = slic(torch.as_tensor(np.asarray(img)).cuda(), max_num_iter=M, enforce_connectivity=False, _stage="pre", **kw).cpu().numpy()
    finally:
        os.environ.pop("OBIA_PREP_GROUPED", None)
        if old is not None:
            os.environ["OBIA_PREP_GROUPED"] = old
    assert np.array_equal(full["labels_pre"], pre), f"{name}: labels_pre of the stage entry and of slic(_stage='pre')"
    fixed = run(name, M, False, True)
    for k, v in full.items():
        same = np.array_equal(v.view(np.uint32), fixed[k].view(np.uint32)) if isinstance(v, np.ndarray) and v.dtype == np.float32 else np.array_equal(v, fixed[k])
        assert same, f"{name}: exit_on_fixed_point changes `{k}`"
