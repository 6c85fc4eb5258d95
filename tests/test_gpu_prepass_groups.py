"""Grouped spatial pre-pass (slic_sweep.hip: queue_sweeps, "two window groups in flight"): in a masked batch of at least two problems
that shares no pre-pass, the spatial-only sweeps and the centroid steps in front of them run as two groups of consecutive problems,
group 0 on the context's stream and group 1 on its side stream, joined in front of the last pre-pass sweep.  Nothing may change: for
every case the labels and the segment count of `create_tiled_segments` under OBIA_PREPASS_GROUPS=2 (group at any size) must be
IDENTICAL to the same call under OBIA_PREPASS_GROUPS=0 (never group) and to the oracle tiler with integer sums, three forced runs must
be identical to each other (a race between the groups shows as a difference), and `timing()["prepass_group_launches"]`
(obia_last_timing 15) must be what the shapes say: 2 x (pre-pass sweeps - 1) per grouped batch, 0 under the switch's 0 -- it proves
which path ran, so that a silent fallback cannot pass.

The batches of a tiler call: ONE black batch, its problems the tiles (tj, ti) with (tj + ti) even in raster order, and one white
batch per tile row (white_order="parity": per parity class of tile rows), its problems that row's tiles with (tj + ti) odd.  A batch
is grouped when it has at least two problems and no two of them form a class of the shared pre-pass (same shape and seeds, a mask that
hides nothing: tests/test_gpu_prepass_share.py).  A white window's mask always hides something here (corner squares, kept segments)."""
import os

import numpy as np
import pytest

from tests.test_gpu_fused_features import ragged_mask
from tests.test_gpu_tiling import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KW = dict(tile_size=128, buffer=32, crown_radius=3, pixel_size=(1.0, 1.0))   # 384 x 512: 3 x 4 tiles; a white window is 9 sweep tiles (64 x 64)


@pytest.fixture()
def integer_sums(oracle):
    oracle.set_sum_mode(1)
    try:
        yield oracle
    finally:
        oracle.set_sum_mode(0)


class groups_switch:
    """OBIA_PREPASS_GROUPS for the calls inside: "0" never, "2" whenever a batch is eligible, None: unset (the size threshold decides)"""
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.pop("OBIA_PREPASS_GROUPS", None)
        if self.value is not None:
            os.environ["OBIA_PREPASS_GROUPS"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("OBIA_PREPASS_GROUPS", None)
        if self.old is not None:
            os.environ["OBIA_PREPASS_GROUPS"] = self.old


def tiler(img_dev, mask, switch, profiling=0, **kw):
    """(labels, n, timing) of one call on a context of its own"""
    from obia_amd import _lib
    from obia_amd.tiling import create_tiled_segments
    ctx = _lib.Context(0)
    ctx.set_profiling(profiling)
    with groups_switch(switch):
        lab, n = create_tiled_segments(img_dev, input_mask=mask, ctx=ctx, **kw)
        t = ctx.timing()
    return lab.cpu().numpy(), n, t


def oracle_tiler(img, mask, **kw):
    from oracle import tiler as ot
    kw = dict(kw)
    if "max_num_iter" in kw:
        kw["max_iter"] = kw.pop("max_num_iter")
    if "white_order" in kw:
        kw["white_order"] = 1 if kw["white_order"] == "parity" else 0
    return ot.create_tiled_segments(img, mask, **kw)


def check(img, mask, launches, what, against_oracle=True, **kw):
    """forced three times against off (and the oracle tiler): identical; the counter says which path ran"""
    dev = torch.as_tensor(img).cuda()
    lab0, n0, t0 = tiler(dev, mask, "0", **kw)
    assert t0["prepass_group_launches"] == 0, f"{what}: OBIA_PREPASS_GROUPS=0 must not group"
    t = None
    for run in range(3):
        lab, n, t = tiler(dev, mask, "2", **kw)
        diff = int((lab != lab0).sum())
        print(f"{what}, forced run {run}: prepass_group_launches {t['prepass_group_launches']:.0f} (expected {launches}), n {n} / {n0}, "
              f"{diff} px differ from OBIA_PREPASS_GROUPS=0, repeats {t['batch_repeats']:.0f} / {t0['batch_repeats']:.0f}")
        assert t["prepass_group_launches"] == launches, f"{what}: {t['prepass_group_launches']} launches as a group member, expected {launches}"
        assert n == n0 and diff == 0, f"{what}, forced run {run}: {diff} px differ from OBIA_PREPASS_GROUPS=0, n {n} vs {n0}"
        assert t["batch_repeats"] == t0["batch_repeats"]
    if against_oracle:
        ref, n_ref = oracle_tiler(img, mask, **kw)
        d = int((lab0 != ref).sum())
        print(f"{what}: {d} px differ from the oracle tiler, n {n0} vs {n_ref}")
        assert n0 == n_ref and d == 0, f"{what}: {d} px differ from the oracle tiler, n {n0} vs {n_ref}"
    return t


def holes_in_every_black_tile(H, W, T, seed):
    """ragged holes, a wholly masked sweep tile, and a few invalid pixels inside every black tile: no black tile's mask hides nothing,
    so the black batch forms no class"""
    mask = ragged_mask(H, W, seed, full_tile=(1, 1))
    for tj in range(-(-H // T)):
        for ti in range(-(-W // T)):
            if (tj + ti) % 2 == 0:
                y, x = tj * T + 5 + 7 * ti, ti * T + 9 + 11 * tj
                mask[y:y + 2 + ti, x:x + 3 + tj] = 0
    return mask.astype(bool)


def test_white_rows_of_two_windows(integer_sums):
    """384 x 512, all-ones mask: the six black tiles are one class (shared pre-pass: not grouped); every one of the three white rows has
    two windows, grouped 1 + 1.  3 batches x 2 x 9."""
    check(synth(384, 512, 8, seed=21), np.ones((384, 512), bool), 3 * 2 * 9, "384x512 all-ones", **KW)


def test_ragged_mask_groups_the_black_batch_too(integer_sums):
    """the same raster with holes in every black tile and sweep tile (1, 1) masked: the black batch forms no class and its six problems
    run 3 + 3, their K unequal (the crown rule counts valid pixels).  4 batches x 2 x 9."""
    mask = holes_in_every_black_tile(384, 512, 128, 7)
    check(synth(384, 512, 8, seed=21), mask, 4 * 2 * 9, "384x512 ragged", **KW)


def test_clipped_windows_of_unequal_size(integer_sums):
    """400 x 650: tile rows of 128, 128, 128, 16 and columns of 5 x 128 and 10, so the windows at the right and the bottom edge are
    clipped.  No mask: the black batch has its classes and is not grouped.  Every white row has three windows -- the last one's are 48
    rows high, of 160, 192 and 170 columns, three sweep tiles each: groups of 2 + 1 problems.  4 batches x 2 x 9."""
    check(synth(400, 650, 8, seed=25), None, 4 * 2 * 9, "400x650", **KW)


def test_five_bands(integer_sums):
    """5 bands in records padded to 8 (the centroid step and the sweep are the 8-channel kernels)"""
    check(synth(384, 512, 5, seed=26), None, 3 * 2 * 9, "384x512x5", **KW)


@pytest.mark.parametrize("iters,launches", [(2, 3 * 2 * 1), (1, 0)])
def test_one_grouped_sweep_and_none(integer_sums, iters, launches):
    """max_num_iter=2: one spatial-only sweep per batch, fork and join around the same sweep.  max_num_iter=1: the pre-pass is its last
    sweep alone, nothing to group, the path is the old one"""
    check(synth(384, 512, 8, seed=21), np.ones((384, 512), bool), launches, f"max_num_iter={iters}", max_num_iter=iters, **KW)


def test_orphan_repeat_runs_ungrouped(integer_sums):
    """the orphan case of tests/test_gpu_tiling.py: islands of valid pixels that no window reaches raise the flag from inside a grouped
    sweep (both groups store the same word), and the batch runs again with every sweep storing its labels, ungrouped.  256 x 300, tiles
    of 128: the black batch (three problems, no class) and white row 1 (two windows) are grouped in their first run; white row 0 has
    one window.  2 batches x 2 x 9."""
    rs = np.random.RandomState(12)
    H, W = 256, 300
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([350 * np.sin(xx / (9 + 3 * c)) * np.cos(yy / (12 + 2 * c)) + 900 + 60 * c + rs.normal(0, 22, (H, W)) for c in range(4)], -1).astype(np.float32)
    mask = np.zeros((H, W), bool)
    mask[:, :70] = True
    mask[10:250:40, 150:152] = True
    mask[30:250:40, 260:263] = True
    t = check(img, mask, 2 * 2 * 9, "orphan repeat", tile_size=128, buffer=16, crown_radius=6.0, pixel_size=(1.0, 1.0), compactness=10.0)
    assert t["batch_repeats"] >= 1, "the case is meant to take the repeat path"


def test_parity_class_of_two_rows_in_one_batch(integer_sums):
    """white_order="parity": the white tiles of rows 0 and 2 are one batch of four windows (2 + 2), row 1 is one of two.  2 batches x 2 x 9."""
    check(synth(384, 512, 8, seed=21), np.ones((384, 512), bool), 2 * 2 * 9, "parity", white_order="parity", **KW)


def test_a_batch_of_one_problem(integer_sums):
    """a raster of one tile: one black problem, no white tile"""
    check(synth(120, 100, 8, seed=27), ragged_mask(120, 100, 3).astype(bool), 0, "single tile", **KW)


def test_default_keeps_small_batches_ungrouped():
    """without the switch a group must fill the device once (occupancy of the spatial kernel x compute units, thousands of sweep tiles):
    these batches have 18 to 54 tiles and stay ungrouped"""
    dev = torch.as_tensor(synth(384, 512, 8, seed=21)).cuda()
    mask = holes_in_every_black_tile(384, 512, 128, 7)
    lab, n, t = tiler(dev, mask, None, **KW)
    lab0, n0, t0 = tiler(dev, mask, "0", **KW)
    assert t["prepass_group_launches"] == 0 and t0["prepass_group_launches"] == 0
    assert n == n0 and np.array_equal(lab, lab0)


def test_timing_resolves_across_the_two_streams():
    """profiling on: the event pairs of the grouped sweeps are bound to dispatches on two streams.  Every span resolves (pixels and time
    counted for every launch); prepass_ms sums overlapping durations, prepass_busy_ms is their union"""
    dev = torch.as_tensor(synth(384, 512, 8, seed=21)).cuda()
    mask = holes_in_every_black_tile(384, 512, 128, 7)
    lab, n, t = tiler(dev, mask, "2", profiling=1, **KW)
    lab0, n0, t0 = tiler(dev, mask, "0", profiling=1, **KW)
    print(f"prepass_ms {t['prepass_ms']:.4f} / {t0['prepass_ms']:.4f}, busy {t['prepass_busy_ms']:.4f} / {t0['prepass_busy_ms']:.4f}, "
          f"prepass_px {t['prepass_px']:.0f} / {t0['prepass_px']:.0f}")
    assert n == n0 and np.array_equal(lab, lab0)
    assert t["prepass_group_launches"] == 4 * 2 * 9
    assert t["prepass_px"] == t0["prepass_px"] > 0, "every grouped launch counts its problems' pixels, once"
    assert t["prepass_ms"] > 0 and 0 < t["prepass_busy_ms"] <= t["prepass_ms"] * (1 + 1e-6) + 1e-6
    assert abs(t0["prepass_busy_ms"] - t0["prepass_ms"]) <= 0.01 * t0["prepass_ms"] + 0.005, "ungrouped: the sweeps run one after the other"
    assert abs(t["assign_busy_ms"] - t["assign_ms"]) <= 0.01 * t["assign_ms"] + 0.005, "the colour sweeps stay serial"
