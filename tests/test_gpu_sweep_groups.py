"""Grouped colour pass (slic_sweep.hip: queue_sweeps, "two window groups in flight"): in a batch of at least two problems and at
least two sweeps, the colour sweeps and the centroid steps in front of them run as two groups of consecutive problems, group 0 on the
context's stream and group 1 on its side stream, forked behind the pre-pass (the clears of an unmasked batch) and joined behind the
last sweep.  Nothing may change: for every case the labels and the segment count of `create_tiled_segments` under OBIA_SWEEP_GROUPS=2
(group at any size) must be IDENTICAL to the same call under OBIA_SWEEP_GROUPS=0 (never group) and, where
tests/test_gpu_prepass_groups.py holds its case against it, to the oracle tiler with integer sums; three forced runs must be identical
to each other (a race between the groups shows as a difference); and `timing()["assign_group_launches"]` (obia_last_timing 19) must be
what the shapes say: 2 x max_iter per grouped batch, 0 under the switch's 0 -- it proves which path ran, so that a silent fallback
cannot pass.

The batches of a tiler call are described in tests/test_gpu_prepass_groups.py.  Unlike the pre-pass, the colour pass of a batch that
SHARES its pre-pass is grouped too: the black batch of an all-ones mask counts."""
import os

import numpy as np
import pytest

from tests.test_gpu_fused_features import ragged_mask
from tests.test_gpu_prepass_groups import KW, holes_in_every_black_tile, integer_sums, oracle_tiler, tiler as prepass_tiler  # noqa: F401
from tests.test_gpu_tiling import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = lambda ms: 0.01 * ms + 0.005   # |assign_busy_ms - assign_ms|: the tolerance of tests/test_gpu_tiling.py::test_sweep_timing_sum_and_union


def tiler(img_dev, mask, switch, prepass=None, profiling=0, **kw):
    """(labels, n, timing) of one call on a context of its own under OBIA_SWEEP_GROUPS=switch ("0" never, "2" whenever a batch is
    eligible, None: unset, the size threshold decides) and OBIA_PREPASS_GROUPS=prepass"""
    old = os.environ.pop("OBIA_SWEEP_GROUPS", None)
    if switch is not None:
        os.environ["OBIA_SWEEP_GROUPS"] = switch
    try:
        return prepass_tiler(img_dev, mask, prepass, profiling=profiling, **kw)
    finally:
        os.environ.pop("OBIA_SWEEP_GROUPS", None)
        if old is not None:
            os.environ["OBIA_SWEEP_GROUPS"] = old


def check(img, mask, launches, what, against_oracle=True, prepass=None, prepass_launches=0, **kw):
    """forced three times against off (and the oracle tiler): identical; the counter says which path ran"""
    dev = torch.as_tensor(img).cuda()
    lab0, n0, t0 = tiler(dev, mask, "0", **kw)
    assert t0["assign_group_launches"] == 0, f"{what}: OBIA_SWEEP_GROUPS=0 must not group"
    t = None
    for run in range(3):
        lab, n, t = tiler(dev, mask, "2", prepass=prepass, **kw)
        diff = int((lab != lab0).sum())
        print(f"{what}, forced run {run}: assign_group_launches {t['assign_group_launches']:.0f} (expected {launches}), pre-pass "
              f"{t['prepass_group_launches']:.0f} (expected {prepass_launches}), n {n} / {n0}, {diff} px differ from OBIA_SWEEP_GROUPS=0, "
              f"repeats {t['batch_repeats']:.0f} / {t0['batch_repeats']:.0f}")
        assert t["assign_group_launches"] == launches, f"{what}: {t['assign_group_launches']} launches as a group member, expected {launches}"
        assert t["prepass_group_launches"] == prepass_launches
        assert n == n0 and diff == 0, f"{what}, forced run {run}: {diff} px differ from OBIA_SWEEP_GROUPS=0, n {n} vs {n0}"
        assert t["batch_repeats"] == t0["batch_repeats"]
    if against_oracle:
        ref, n_ref = oracle_tiler(img, mask, **kw)
        d = int((lab0 != ref).sum())
        print(f"{what}: {d} px differ from the oracle tiler, n {n0} vs {n_ref}")
        assert n0 == n_ref and d == 0, f"{what}: {d} px differ from the oracle tiler, n {n0} vs {n_ref}"
    return t


def test_black_batch_with_a_shared_pre_pass_and_white_rows(integer_sums):
    """384 x 512, all-ones mask: the six black tiles are one class -- their pre-pass is shared, their colour pass runs 3 + 3 -- and
    every one of the three white rows has two windows, 1 + 1.  4 batches x 2 x 10."""
    check(synth(384, 512, 8, seed=21), np.ones((384, 512), bool), 4 * 2 * 10, "384x512 all-ones", **KW)


@pytest.mark.parametrize("prepass,prepass_launches", [(None, 0), ("2", 4 * 2 * 9)], ids=["colour", "both"])
def test_ragged_mask(integer_sums, prepass, prepass_launches):
    """the same raster with holes in every black tile and sweep tile (1, 1) masked: problems of unequal K.  4 batches x 2 x 10; with
    both switches forced a batch forks twice (the last pre-pass sweep between the two stays whole-batch)."""
    mask = holes_in_every_black_tile(384, 512, 128, 7)
    check(synth(384, 512, 8, seed=21), mask, 4 * 2 * 10, "384x512 ragged", prepass=prepass, prepass_launches=prepass_launches, **KW)


def test_clipped_windows_of_unequal_size(integer_sums):
    """400 x 650, no mask: tile rows of 128, 128, 128, 16 and columns of 5 x 128 and 10, windows clipped at the right and the bottom
    edge.  The unmasked batches have no pre-pass: the fork stands behind the clears.  The black batch (12 problems) and four white rows
    of three windows, groups of 2 + 1 among them.  5 batches x 2 x 10."""
    check(synth(400, 650, 8, seed=25), None, 5 * 2 * 10, "400x650", **KW)


def test_five_bands(integer_sums):
    """5 bands in records padded to 8: the padded variant of the colour kernel (NCH = 5)"""
    check(synth(384, 512, 5, seed=26), None, 4 * 2 * 10, "384x512x5", **KW)


@pytest.mark.parametrize("bands,compactness,against_oracle", [(8, 0.25, True), (3, 10.0, False)], ids=["8_bands_c0.25", "3_bands_lab_c10"])
def test_low_compactness_kernel(integer_sums, bands, compactness, against_oracle):
    """slic_assign_collb_kernel.  The suite has no counter for the path; it is taken because slic_batch_settings sets col_lb when
    slic_use_colour_bound(ratio = 1 / compactness, to_lab) holds -- ratio >= 2 for 8 bands at compactness 0.25 (4), ratio x 100 >= 2 for
    the Lab features of 3 bands at compactness 10 (10) -- and neither SLIC-zero, exit_on_fixed_point nor a spacing is set;
    launch_assign then launches the colour-bound kernel for every colour sweep (the tiler allocates the colour boxes whenever col_lb
    is set).  The 3-band case goes through rgb2lab, which the oracle matches within a tolerance only: forced against off alone."""
    check(synth(384, 512, bands, seed=21), None, 4 * 2 * 10, f"{bands} bands, compactness {compactness}", against_oracle=against_oracle,
          compactness=compactness, **KW)


@pytest.mark.parametrize("iters,launches", [(2, 4 * 2 * 2), (1, 0)])
def test_two_sweeps_and_one(integer_sums, iters, launches):
    """max_num_iter=2: the first sweep accumulates, the second stores the labels.  max_num_iter=1: nothing for a centroid step to hide
    behind, the path is the old one"""
    check(synth(384, 512, 8, seed=21), np.ones((384, 512), bool), launches, f"max_num_iter={iters}", max_num_iter=iters, **KW)


def test_orphan_repeat_runs_ungrouped(integer_sums):
    """the orphan case of tests/test_gpu_tiling.py: islands of valid pixels that no window reaches raise the flag from inside a grouped
    sweep (both groups store the same word), and the batch runs again with every sweep storing its labels, ungrouped.  256 x 300, tiles
    of 128: the black batch (three problems) and white row 1 (two windows) are grouped in their first run; white row 0 has one window.
    2 batches x 2 x 10."""
    rs = np.random.RandomState(12)
    H, W = 256, 300
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([350 * np.sin(xx / (9 + 3 * c)) * np.cos(yy / (12 + 2 * c)) + 900 + 60 * c + rs.normal(0, 22, (H, W)) for c in range(4)], -1).astype(np.float32)
    mask = np.zeros((H, W), bool)
    mask[:, :70] = True
    mask[10:250:40, 150:152] = True
    mask[30:250:40, 260:263] = True
    t = check(img, mask, 2 * 2 * 10, "orphan repeat", tile_size=128, buffer=16, crown_radius=6.0, pixel_size=(1.0, 1.0), compactness=10.0)
    assert t["batch_repeats"] >= 1, "the case is meant to take the repeat path"


def test_parity_class_of_two_rows_in_one_batch(integer_sums):
    """white_order="parity": the white tiles of rows 0 and 2 are one batch of four windows (2 + 2), row 1 is one of two; with the black
    batch 3 batches x 2 x 10."""
    check(synth(384, 512, 8, seed=21), np.ones((384, 512), bool), 3 * 2 * 10, "parity", white_order="parity", **KW)


def test_a_batch_of_one_problem(integer_sums):
    """a raster of one tile: one black problem, no white tile"""
    check(synth(120, 100, 8, seed=27), ragged_mask(120, 100, 3).astype(bool), 0, "single tile", **KW)


def test_exit_on_fixed_point_is_never_grouped():
    """every sweep stores its labels and the tiles replay them: not grouped, labels identical"""
    check(synth(384, 512, 8, seed=21), np.ones((384, 512), bool), 0, "exit_on_fixed_point", against_oracle=False, exit_on_fixed_point=True, **KW)


def test_default_keeps_small_batches_ungrouped():
    """without the switch a group must hold one residency of its colour kernel (occupancy x compute units, more than a thousand sweep
    tiles): these batches have 18 to 54 tiles and stay ungrouped"""
    dev = torch.as_tensor(synth(384, 512, 8, seed=21)).cuda()
    mask = holes_in_every_black_tile(384, 512, 128, 7)
    lab, n, t = tiler(dev, mask, None, **KW)
    lab0, n0, t0 = tiler(dev, mask, "0", **KW)
    assert t["assign_group_launches"] == 0 and t0["assign_group_launches"] == 0
    assert n == n0 and np.array_equal(lab, lab0)


@pytest.mark.parametrize("profiling", [1, 2])
def test_timing_resolves_across_the_two_streams(profiling):
    """profiling on: the event pairs of the grouped sweeps are bound to dispatches on two streams.  Every span resolves -- sweeps and
    pixels are what the ungrouped run counts, every pixel once; class 0 is the union of a grouped batch's launches, so it stays equal to
    the call's busy time, and the plain sum of the launches is no smaller"""
    dev = torch.as_tensor(synth(384, 512, 8, seed=21)).cuda()
    mask = holes_in_every_black_tile(384, 512, 128, 7)
    lab, n, t = tiler(dev, mask, "2", profiling=profiling, **KW)
    lab0, n0, t0 = tiler(dev, mask, "0", profiling=profiling, **KW)
    print(f"profiling {profiling}: assign_ms {t['assign_ms']:.4f} / {t0['assign_ms']:.4f}, busy {t['assign_busy_ms']:.4f} / {t0['assign_busy_ms']:.4f}, "
          f"launch sum {t['assign_launch_sum_ms']:.4f} / {t0['assign_launch_sum_ms']:.4f}, sweeps {t['sweeps']:.0f} / {t0['sweeps']:.0f}, "
          f"assign_px {t['assign_px']:.0f} / {t0['assign_px']:.0f}, store_px {t['assign_store_px']:.0f} / {t0['assign_store_px']:.0f}")
    assert n == n0 and np.array_equal(lab, lab0)
    assert t["assign_group_launches"] == 4 * 2 * 10 and t0["assign_group_launches"] == 0
    assert t["sweeps"] == t0["sweeps"] == 4 * 10, "a sweep of a grouped batch is two launches and counts once"
    assert t["assign_px"] == t0["assign_px"] > 0, "every grouped launch counts its problems' pixels, once"
    assert t["assign_store_px"] == t0["assign_store_px"] > 0
    assert t["assign_ms"] > 0 and abs(t["assign_busy_ms"] - t["assign_ms"]) <= TOL(t["assign_ms"])
    assert abs(t0["assign_busy_ms"] - t0["assign_ms"]) <= TOL(t0["assign_ms"])
    assert t["assign_launch_sum_ms"] >= t["assign_ms"] * (1 - 1e-6)
    assert abs(t0["assign_launch_sum_ms"] - t0["assign_ms"]) <= 1e-6 * t0["assign_ms"], "ungrouped: class 0 is the plain sum"
