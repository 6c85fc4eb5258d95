"""Shared spatial pre-pass (slic_sweep.hip, slic_prepass_broadcast_kernel): black tiles of one shape whose mask hides nothing run the
same nine spatial-only sweeps, so only the first of such a class runs them and the others receive its centroid sums in front of the
last pre-pass sweep.  Nothing may change: for every case the labels and the segment count of `create_tiled_segments` must be
IDENTICAL to the same call under OBIA_PREPASS_SHARE=0 (every problem runs every sweep) and to the oracle tiler with integer sums
(tests/test_gpu_exact_sums.py), and the pixel-sweeps that were covered by sharing, `timing()["prepass_shared_px"]` = S, must be what
the shapes say: per class of m black tiles of h x w pixels, (m - 1) * h * w * (pre-pass sweeps - 1).

Black tiles are the tiles (tj, ti) with (tj + ti) even, cut with their exact windows; the problems of the black batch are in raster
order of the tiles."""
import os

import numpy as np
import pytest

from tests.test_gpu_tiling import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KW = dict(tile_size=128, buffer=16, crown_radius=3, pixel_size=(1.0, 1.0))   # the first raster: 384 x 512, 3 x 4 tiles of 128 x 128
T2 = 128 * 128


@pytest.fixture()
def integer_sums(oracle):
    oracle.set_sum_mode(1)
    try:
        yield oracle
    finally:
        oracle.set_sum_mode(0)


@pytest.fixture(scope="module")
def first_raster():
    return synth(384, 512, 8, seed=21)


def tiler(img, mask, share, ctx=None, **kw):
    """(labels, n, timing) of one call with the sharing on or off"""
    from obia_amd import _lib
    from obia_amd.tiling import create_tiled_segments
    if ctx is None:
        ctx = _lib.Context(0)
    ctx.set_profiling(1)
    old = os.environ.pop("OBIA_PREPASS_SHARE", None)
    try:
        if not share:
            os.environ["OBIA_PREPASS_SHARE"] = "0"
        lab, n = create_tiled_segments(img if torch.is_tensor(img) else torch.as_tensor(img).cuda(), input_mask=mask, ctx=ctx, **kw)
        t = ctx.timing()
    finally:
        os.environ.pop("OBIA_PREPASS_SHARE", None)
        if old is not None:
            os.environ["OBIA_PREPASS_SHARE"] = old
    return lab.cpu().numpy(), n, t


def oracle_tiler(img, mask, **kw):
    from oracle import tiler as ot
    kw = dict(kw)
    if "max_num_iter" in kw:
        kw["max_iter"] = kw.pop("max_num_iter")
    for k in ("exit_on_fixed_point", "seeding"):   # neither changes what the grid-seeded reference computes / not the oracle's to restate
        kw.pop(k, None)
    return ot.create_tiled_segments(img, mask, **kw)


def check(img, mask, S, what, against_oracle=True, **kw):
    dev = torch.as_tensor(img).cuda()
    lab, n, t = tiler(dev, mask, True, **kw)
    lab0, n0, t0 = tiler(dev, mask, False, **kw)
    diff0 = int((lab != lab0).sum())
    print(f"{what}: shared {t['prepass_shared_px']:.0f} px-sweeps (expected {S}), covered {t['prepass_px']:.0f} / {t0['prepass_px']:.0f}, "
          f"n {n} / {n0}, {diff0} px differ from the unshared call")
    assert n == n0 and diff0 == 0, f"{what}: {diff0} px differ from OBIA_PREPASS_SHARE=0, n {n} vs {n0}"
    assert t0["prepass_shared_px"] == 0
    assert t["prepass_shared_px"] == S, f"{what}: shared {t['prepass_shared_px']} px-sweeps, expected {S}"
    assert t["prepass_px"] == t0["prepass_px"], "prepass_px counts the pixels the pre-pass covered, shared ones included"
    if against_oracle:
        ref, n_ref = oracle_tiler(img, mask, **kw)
        diff = int((lab != ref).sum())
        print(f"{what}: {diff} px differ from the oracle tiler, n {n} vs {n_ref}")
        assert n == n_ref and diff == 0, f"{what}: {diff} px differ from the oracle tiler, n {n} vs {n_ref}"
    return lab, n, t


def test_one_class_of_six_black_tiles(integer_sums, first_raster):
    """384 x 512, tiles of 128: the six black tiles are 128 x 128 with the same n -- one class, its representative is the first problem
    of the batch (a span of tiles, no table).  Several sweep tiles (64 x 64) per problem.  S = 9 sweeps x 5 members x 128^2."""
    check(first_raster, None, 9 * 5 * T2, "one class", **KW)


def test_several_classes_and_singletons(integer_sums):
    """300 x 340, tiles of 100: rows of 100, 100, 100, columns of 100, 100, 100, 40.  Black tiles (0,0) (0,2) (1,1) (2,0) (2,2) are
    100 x 100: one class of five; (1,3) is 100 x 40: alone.  The problems that run the shared sweeps are the first and the fourth of the
    batch: not consecutive, a table of tiles.  S = 9 x 4 x 100^2.
    330 x 340 adds a bottom row of 30: (3,1) is 30 x 100 and (3,3) 30 x 40, both alone (interior, right-edge, bottom-edge and corner
    shapes); the class of five is the same.  S = 9 x 4 x 100^2 again."""
    kw = dict(tile_size=100, buffer=16, crown_radius=3, pixel_size=(1.0, 1.0))
    check(synth(300, 340, 8, seed=22), None, 9 * 4 * 100 * 100, "300x340", **kw)
    check(synth(330, 340, 8, seed=23), None, 9 * 4 * 100 * 100, "330x340", **kw)


def test_two_classes_with_members(integer_sums):
    """340 x 440, tiles of 100: three classes with members.  S = 9 x (5 x 100^2 + 1 x 100 x 40 + 1 x 40 x 100)."""
    kw = dict(tile_size=100, buffer=16, crown_radius=3, pixel_size=(1.0, 1.0))
    # rows 0..2 are 100 high, row 3 is 40; columns 0..3 are 100 wide, column 4 is 40.  (tj + ti) even:
    # 100 x 100: (0,0) (0,2) (1,1) (1,3) (2,0) (2,2) = 6;  100 x 40: (0,4) (2,4) = 2;  40 x 100: (3,1) (3,3) = 2
    check(synth(340, 440, 8, seed=24), None, 9 * (5 * 100 * 100 + 100 * 40 + 40 * 100), "340x440", **kw)


def test_three_invalid_pixels_take_a_tile_out_of_its_class(integer_sums, first_raster):
    """three masked pixels inside black tile (1,1): n_valid != H * W, it runs its own sweeps.  S shrinks by that tile's share."""
    mask = np.ones((384, 512), bool)
    mask[150, 160] = mask[151, 160] = mask[200, 131] = False
    check(first_raster, mask, 9 * 4 * T2, "three invalid pixels", **KW)


def test_a_black_tile_wholly_invalid(integer_sums, first_raster):
    """black tile (0,2) has no valid pixel: skipped (no centroids), in no class.  S = 9 x 4 x 128^2."""
    mask = np.ones((384, 512), bool)
    mask[0:128, 256:384] = False
    check(first_raster, mask, 9 * 4 * T2, "empty black tile", **KW)


def test_a_black_tile_constant_in_a_band(integer_sums, first_raster):
    """black tile (2,0) is constant in band 3: skipped like the reference's ValueError tile, in no class (no centroids).  Its mask hides
    nothing, so every pixel of it is a valid pixel no window reaches: the batch's orphan flag is raised and the batch runs again with
    every sweep storing its labels -- the fallback, as before this sharing existed.  S = 0 (the repeat counts its own pixels), identical
    labels."""
    img = first_raster.copy()
    img[256:384, 0:128, 3] = 7.0
    _, _, t = check(img, None, 0, "constant band", **KW)
    assert t["batch_repeats"] >= 1, "a skipped tile with valid pixels takes the orphan repeat"


def test_dense_grid_and_centroids_without_pixels(integer_sums, oracle):
    """384 x 384, tiles of 64, buffer 8, n_segments = 700 per full tile: a grid step of 2 pixels, 1024 centroids per 64 x 64 tile (more
    candidates than a sweep tile lists: the unlisted path).  Eighteen black tiles of 64 x 64: S = 9 x 17 x 64^2.
    A centroid that loses all its pixels in a pre-pass sweep (n = 0: NaN position, empty window) would travel to the members through
    the copied sums.  The oracle shows NONE on a 64 x 64 tile whose mask hides nothing, at any density: the grid rule gives integer
    steps (4, 3, 2, 1 for n = 300 ... 4096, at step 1 every pixel is a centroid) and in a spatial-only sweep every centroid of a
    regular grid keeps at least the pixel it sits on.  The scan below repeats that for the steps 3, 2 and 1 and prints the counts; with
    none to be had the case pins the dense grid alone.  (Members are all-valid by the class rule, so no mask can produce one either.)"""
    mask = np.ones((64, 64), np.uint8)
    for n in (400, 700, 4096):
        yx, steps = oracle.masked_grid_centroids(mask, n)
        seg = np.zeros((yx.shape[0], 3), np.float32)
        seg[:, :2] = yx
        empty = []
        for _ in range(9):   # a sweep depends on the centroids alone: one more sweep from where the last one ended
            oracle.slic_core(np.zeros((64, 64, 1), np.float32), seg, float(max(steps.max(), 1.0)), max_iter=1, mask=mask, ignore_color=True)
            empty.append(int(np.isnan(seg[:, 0]).sum()))
        print(f"oracle, 64 x 64, n_segments {n}: K {yx.shape[0]}, steps {steps}, empty centroids after each pre-pass sweep {empty}")
    kw = dict(tile_size=64, buffer=8, crown_radius=3, pixel_size=(1.0, 1.0), n_segments=700)
    check(synth(384, 384, 8, seed=25), None, 9 * 17 * 64 * 64, "dense grid", **kw)


def test_three_bands_lab(integer_sums, first_raster):
    """3 bands: Lab features, CP = 4, the colour-bound kernel's neighbourhood in the main pass"""
    check(np.ascontiguousarray(first_raster[:, :, :3]), None, 9 * 5 * T2, "3 bands", **KW)


def test_nine_bands(integer_sums):
    """9 bands: CP = 12"""
    check(synth(384, 512, 9, seed=26), None, 9 * 5 * T2, "9 bands", **KW)


def test_low_compactness(integer_sums, first_raster):
    check(first_raster, None, 9 * 5 * T2, "compactness 0.25", compactness=0.25, **KW)


def test_one_sweep_has_nothing_to_share(integer_sums, first_raster):
    """max_num_iter = 1: the pre-pass is its last sweep alone"""
    check(first_raster, None, 0, "max_num_iter 1", max_num_iter=1, **KW)


def test_two_sweeps_share_one(integer_sums, first_raster):
    """max_num_iter = 2: one shared sweep, the broadcast follows the very first centroid step.  S = 1 x 5 x 128^2."""
    check(first_raster, None, 1 * 5 * T2, "max_num_iter 2", max_num_iter=2, **KW)


def test_exit_on_fixed_point_falls_back(integer_sums, first_raster):
    """every sweep stores its labels: today's path, S = 0"""
    check(first_raster, None, 0, "exit_on_fixed_point", exit_on_fixed_point=True, **KW)


def test_orphan_repeat_falls_back(integer_sums):
    """the masked case of test_gpu_tiling.py that takes the orphan repeat: the black batch (two tiles of 128 x 128 with sparse masks, no
    class) runs again with every sweep storing.  Identical labels; nothing shared."""
    rs = np.random.RandomState(12)
    H, W = 256, 300
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([350 * np.sin(xx / (9 + 3 * c)) * np.cos(yy / (12 + 2 * c)) + 900 + 60 * c + rs.normal(0, 22, (H, W)) for c in range(4)], -1).astype(np.float32)
    mask = np.zeros((H, W), bool)
    mask[:, :70] = True
    mask[10:250:40, 150:152] = True
    mask[30:250:40, 260:263] = True
    kw = dict(tile_size=128, buffer=16, crown_radius=6.0, pixel_size=(1.0, 1.0), compactness=10.0)
    _, _, t = check(img, mask, 0, "orphan repeat", **kw)
    assert t["batch_repeats"] >= 1, "the case is meant to take the repeat path"


def test_skimage_seeding_falls_back(first_raster):
    """seeding="skimage": the seeds arrive as external seeds, which form no class: S = 0, identical labels.  (The oracle
    tiler restates the grid rule only; tests/test_gpu_tiling_skimage.py pins this seeding against its own reference.)"""
    check(first_raster, np.ones((384, 512), bool), 0, "seeding skimage", against_oracle=False, seeding="skimage", n_segments=40, **KW)


def test_two_calls_on_one_context_leak_nothing(first_raster):
    """share, OBIA_PREPASS_SHARE=0, share on ONE context: the arena is reused, a member's records and lists hold whatever the call
    before left there until the broadcast and its first build"""
    from obia_amd import _lib
    ctx = _lib.Context(0)
    dev = torch.as_tensor(first_raster).cuda()
    a = tiler(dev, None, True, ctx=ctx, **KW)
    b = tiler(dev, None, False, ctx=ctx, **KW)
    c = tiler(dev, None, True, ctx=ctx, **KW)
    assert a[1] == b[1] == c[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
    assert a[2]["prepass_shared_px"] == c[2]["prepass_shared_px"] == 9 * 5 * T2 and b[2]["prepass_shared_px"] == 0
