"""Fused feature pass (slic_sweep.hip: RAWIN; slic.hpp: slic_fuse_features): in a masked batch of normalised bands the last sweep of
the spatial pre-pass reads the caller's raster, normalises in registers, writes the feature planes and folds from the registers; the
feature step is the min / max pass alone.  Nothing may change: every output must be IDENTICAL, bit for bit, to the same call under
OBIA_FUSE_FEATURES=0 (the separate feature pass) and equal to the oracle wherever tests/slic_stages.py / the oracle tiler give the
comparison.  `timing()["feature_fused_px"]` (obia_last_timing 14) counts the pixels whose planes a sweep wrote: it proves which
path ran, so that a silent fallback cannot pass.

Every pixel of every window must receive its planes: masked pixels (the colour sweeps load them), fully masked footprints and
sweep tiles, the zeros outside the window inside its last quad row / column block, tiles that take slow_tile() -- Stage A compares
all H x W pixels."""
import os

import numpy as np
import pytest

from tests import slic_stages as S
from tests.test_gpu_tiling import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEYS = ("features", "seeds_yx", "centroids", "labels_pre", "K", "step", "prescale", "fscale")


class fuse_switch:
    """OBIA_FUSE_FEATURES for the calls inside: "0" forces the separate pass, "1" asks for the fused one wherever it applies"""
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.pop("OBIA_FUSE_FEATURES", None)
        if self.value is not None:
            os.environ["OBIA_FUSE_FEATURES"] = self.value

    def __exit__(self, *exc):
        os.environ.pop("OBIA_FUSE_FEATURES", None)
        if self.old is not None:
            os.environ["OBIA_FUSE_FEATURES"] = self.old


def same(a, b):
    if isinstance(a, np.ndarray) and a.dtype == np.float32:
        return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


def stages(img_dev, fused, **kw):
    """(stage outputs on the host, feature_fused_px) of one call"""
    from obia_amd import _lib
    from obia_amd.segmentation import _slic_stages
    ctx = _lib.Context(0)
    with fuse_switch("1" if fused else "0"):
        g = _slic_stages(img_dev, ctx=ctx, **kw)
        px = ctx.timing()["feature_fused_px"]
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in g.items()}, px


def ragged_mask(H, W, seed, full_tile=None, full_footprint=None):
    """valid everywhere but ragged holes; optionally one whole 64 x 64 sweep tile and one whole 16 x 16 footprint masked"""
    rs = np.random.RandomState(seed)
    m = np.ones((H, W), np.uint8)
    for _ in range(6):
        y, x = rs.randint(0, H), rs.randint(0, W)
        for dy in range(rs.randint(2, 9)):
            if y + dy < H:
                a = max(0, x - rs.randint(0, 7))
                m[y + dy, a:min(W, x + rs.randint(1, 11))] = 0
    if full_tile:
        ty, tx = full_tile
        m[64 * ty:64 * ty + 64, 64 * tx:64 * tx + 64] = 0
    if full_footprint:
        fy, fx = full_footprint
        m[16 * fy:16 * fy + 16, 16 * fx:16 * fx + 16] = 0
    return m


def extremes_under_the_mask(img, mask):
    """the band minima and maxima sit on masked pixels: the normalisation reads them, and their planes must come out like any other's"""
    img = img.copy()
    ys, xs = np.nonzero(mask == 0)
    for c in range(img.shape[2]):
        i, j = (2 * c) % len(ys), (2 * c + 1) % len(ys)
        img[ys[i], xs[i], c] = img[..., c].min() - 100.0 - c
        img[ys[j], xs[j], c] = img[..., c].max() + 250.0 + c
    return img


def check_stages(oracle, img, mask, per_seg, name, runs, compactness=10.0):
    """the runs fused and unfused: identical, the counter says which path ran, features and labels equal to the oracle's"""
    H, W, C = img.shape
    case = S._case(name, H, W, C, per_seg, compactness, mask="given")
    dev = torch.as_tensor(img).cuda()
    kw0 = S.slic_kwargs(case, mask, None)
    valid = mask != 0
    fill = case["start_label"] - 1
    ref32 = S.features_ref32(oracle, img, case)
    for n, prepass_only in runs:
        tag = f"{name}: max_num_iter {n}{', pre-pass only' if prepass_only else ''}"
        kw = dict(kw0, max_num_iter=n, prepass_only=prepass_only)
        a, px = stages(dev, True, **kw)
        b, px0 = stages(dev, False, **kw)
        print(f"{tag}: K {a['K']}, feature_fused_px {px:.0f} / {px0:.0f}")
        assert px == H * W, f"{tag}: {px} pixels written by a sweep, expected all {H * W}: the fused path did not run"
        assert px0 == 0, f"{tag}: OBIA_FUSE_FEATURES=0 must take the separate pass"
        for k in KEYS:
            assert same(a[k], b[k]), f"{tag}: `{k}` differs from the separate feature pass"
        diff = a["features"].view(np.uint32) != ref32.view(np.uint32)
        assert not diff.any(), f"{tag}: {int(diff.sum())} features differ from the float32 reference, first at {tuple(np.argwhere(diff)[0])}"
        assert a["fscale"] == S.expected_fscale(a["features"])
        ref = S.sweep_ref32(oracle, a["features"], a["centroids"], a["step"], mask=mask, ignore_color=prepass_only, start_label=case["start_label"])
        lab = a["labels_pre"]
        assert (lab[~valid] == fill).all()
        bad = valid & (ref != fill) & (lab != ref)
        assert not bad.any(), f"{tag}: {int(bad.sum())} px differ from the reference's sweep"


RUNS = [(1, False), (2, False), (10, False), (1, True), (2, True), (10, True)]


def test_stages_single_masked_raster(oracle):
    """150 x 203 x 8: H no multiple of 4 or 16, W no multiple of 16; ragged holes, sweep tile (1, 1) and footprint (1, 9) wholly masked;
    the band extremes under the mask"""
    H, W = 150, 203
    mask = ragged_mask(H, W, 5, full_tile=(1, 1), full_footprint=(1, 9))
    img = extremes_under_the_mask(synth(H, W, 8, seed=31), mask)
    check_stages(oracle, img, mask, 80, "fused_150x203_c8", RUNS)


@pytest.mark.parametrize("H,W,C", [(70, 90, 4), (64, 64, 8), (65, 65, 8)])
def test_stages_four_bands_and_tile_edges(oracle, H, W, C):
    """4 bands (CP = 4); 8 bands on exactly one sweep tile and on one pixel more in both directions"""
    mask = ragged_mask(H, W, 6 + H)
    img = extremes_under_the_mask(synth(H, W, C, seed=32 + H), mask)
    check_stages(oracle, img, mask, 60, f"fused_{H}x{W}_c{C}", RUNS)


def test_stages_dense_seeds_take_the_direct_tile_path(oracle):
    """one centroid per 9 pixels: a 64 x 64 tile meets more candidates than it has slots and takes slow_tile(), which writes the tile's
    planes first"""
    H, W = 70, 83
    mask = ragged_mask(H, W, 9)
    img = extremes_under_the_mask(synth(H, W, 8, seed=41), mask)
    check_stages(oracle, img, mask, 9, "fused_dense_c8", [(1, False), (3, False), (2, True)])


FALLBACKS = {
    "three_bands_lab": dict(C=3, convert2lab=True),
    "five_bands": dict(C=5),
    "nine_bands": dict(C=9),
    "sixteen_bands": dict(C=16),
    "compactness_0.25": dict(compactness=0.25),
    "sigma": dict(sigma=1.3),
    "spacing": dict(spacing=[1.0, 0.5, 1.75]),
    "exit_on_fixed_point": dict(exit_on_fixed_point=True),
    "slic_zero": dict(slic_zero=True),
    "no_mask": dict(masked=False),
}


@pytest.mark.parametrize("what", list(FALLBACKS))
def test_fallbacks_keep_the_separate_pass(what):
    """what the fused pass does not cover runs exactly as with OBIA_FUSE_FEATURES=0, and the counter stays 0"""
    opt = dict(FALLBACKS[what])
    H, W, C = 70, 90, opt.pop("C", 8)
    masked = opt.pop("masked", True)
    mask = ragged_mask(H, W, 12) if masked else None
    dev = torch.as_tensor(synth(H, W, C, seed=50 + C)).cuda()
    kw = dict(n_segments=60, compactness=10.0, max_num_iter=4, _normalize_bands=True, mask=mask, convert2lab=False)
    kw.update(opt)
    a, px = stages(dev, True, **kw)
    b, px0 = stages(dev, False, **kw)
    assert px == 0 and px0 == 0, f"{what}: {px} / {px0} pixels written by a sweep: this case must take the separate feature pass"
    for k in KEYS:
        assert same(a[k], b[k]), f"{what}: `{k}` differs"


# ---- the tiler ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def integer_sums(oracle):
    oracle.set_sum_mode(1)
    try:
        yield oracle
    finally:
        oracle.set_sum_mode(0)


def tiler(img_dev, mask, fused, ctx=None, **kw):
    """(labels, n, timing), or the error's text, of one call"""
    from obia_amd import _lib
    from obia_amd.tiling import create_tiled_segments
    if ctx is None:
        ctx = _lib.Context(0)
    ctx.set_profiling(1)   # (prepass_shared_px is counted with profiling on)
    with fuse_switch("1" if fused else "0"):
        try:
            lab, n = create_tiled_segments(img_dev, input_mask=mask, ctx=ctx, **kw)
        except Exception as e:   # noqa: BLE001  (compared with the other path's)
            return f"{type(e).__name__}: {e}"
        t = ctx.timing()
    return lab.cpu().numpy(), n, t


def check_tiler(img, mask, what, against_oracle=True, **kw):
    from oracle import tiler as ot
    dev = torch.as_tensor(img).cuda()
    a = tiler(dev, mask, True, **kw)
    b = tiler(dev, mask, False, **kw)
    assert not isinstance(a, str) and not isinstance(b, str), f"{what}: {a if isinstance(a, str) else b}"
    diff = int((a[0] != b[0]).sum())
    print(f"{what}: n {a[1]} / {b[1]}, {diff} px differ from OBIA_FUSE_FEATURES=0, feature_fused_px {a[2]['feature_fused_px']:.0f} / "
          f"{b[2]['feature_fused_px']:.0f}, repeats {a[2]['batch_repeats']:.0f}")
    assert a[1] == b[1] and diff == 0, f"{what}: {diff} px differ from OBIA_FUSE_FEATURES=0, n {a[1]} vs {b[1]}"
    assert a[2]["feature_fused_px"] > 0, f"{what}: the fused path did not run"
    assert b[2]["feature_fused_px"] == 0
    if against_oracle:
        ref, n_ref = ot.create_tiled_segments(img, mask, **kw)
        d = int((a[0] != ref).sum())
        assert a[1] == n_ref and d == 0, f"{what}: {d} px differ from the oracle tiler, n {a[1]} vs {n_ref}"
    return a


KW = dict(tile_size=96, buffer=16, crown_radius=3, pixel_size=(1.0, 1.0))


def test_tiler_black_tiles_white_rows_and_edges(integer_sums):
    """300 x 280, tiles of 96: 4 x 3 tiles, the last row 12 and the last column 88 wide: black tiles, white rows (grown windows: their
    planes come from the batch's own arena), partial edge tiles, corner squares.  Every window's pixels are counted once."""
    H, W = 300, 280
    mask = np.ones((H, W), bool)
    mask[40:47, 30:60] = False
    mask[100:180, 200:204] = False
    a = check_tiler(synth(H, W, 8, seed=61), mask, "300x280", **KW)
    black = sum(min(96, H - 96 * j) * min(96, W - 96 * i) for j in range(4) for i in range(3) if (i + j) % 2 == 0)
    white = sum((min(H, 96 * j + 112) - max(0, 96 * j - 16)) * (min(W, 96 * i + 112) - max(0, 96 * i - 16))
                for j in range(4) for i in range(3) if (i + j) % 2 == 1)
    assert a[2]["feature_fused_px"] == black + white, "every pixel of every window of both passes, once"


def test_tiler_one_class_of_identical_black_tiles(integer_sums):
    """384 x 512, tiles of 128, no mask: six identical all-valid black tiles share one pre-pass; its last sweep, the fused one, runs for all"""
    a = check_tiler(synth(384, 512, 8, seed=21), None, "one class", tile_size=128, buffer=16, crown_radius=3, pixel_size=(1.0, 1.0))
    assert a[2]["prepass_shared_px"] == 9 * 5 * 128 * 128


def test_tiler_black_tile_constant_in_one_band(integer_sums):
    """black tile (2, 0) is constant in band 3: skipped from the flags of the min / max pass; its planes are written all the same"""
    img = synth(300, 280, 8, seed=62)
    img[192:288, 0:96, 3] = 7.0
    check_tiler(img, None, "constant band", **KW)


def test_tiler_wholly_invalid_tile(integer_sums):
    mask = np.ones((300, 280), bool)
    mask[0:96, 192:280] = False
    check_tiler(synth(300, 280, 8, seed=63), mask, "invalid tile", **KW)


def test_tiler_orphan_repeat_runs_the_plain_kernel(integer_sums):
    """the orphan case of test_gpu_prepass_share.py::test_orphan_repeat_falls_back: the repeat finds the planes written"""
    rs = np.random.RandomState(12)
    H, W = 256, 300
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([350 * np.sin(xx / (9 + 3 * c)) * np.cos(yy / (12 + 2 * c)) + 900 + 60 * c + rs.normal(0, 22, (H, W)) for c in range(4)], -1).astype(np.float32)
    mask = np.zeros((H, W), bool)
    mask[:, :70] = True
    mask[10:250:40, 150:152] = True
    mask[30:250:40, 260:263] = True
    a = check_tiler(img, mask, "orphan repeat", tile_size=128, buffer=16, crown_radius=6.0, pixel_size=(1.0, 1.0), compactness=10.0)
    assert a[2]["batch_repeats"] >= 1, "the case is meant to take the repeat path"


def test_tiler_nan_in_the_raster():
    """a NaN inside one tile: whatever the separate pass makes of it (an error, or a skipped tile), the fused one makes the same"""
    img = synth(300, 280, 8, seed=64)
    img[130, 140, 2] = np.nan
    dev = torch.as_tensor(img).cuda()
    a, b = tiler(dev, None, True, **KW), tiler(dev, None, False, **KW)
    print("NaN in the raster:", a if isinstance(a, str) else f"n {a[1]}", "|", b if isinstance(b, str) else f"n {b[1]}")
    if isinstance(b, str):
        assert a == b
    else:
        assert not isinstance(a, str), a
        assert a[1] == b[1] and np.array_equal(a[0], b[0])
        assert a[2]["feature_fused_px"] > 0 and b[2]["feature_fused_px"] == 0


def test_nan_under_the_mask_is_the_same_error():
    """single raster: a NaN (under the mask: the normalisation reads every pixel) is refused from the non-finite flag of the min / max
    pass, with the text of the separate pass -- the planes, and with them max |feature|, do not exist yet on the fused path"""
    from obia_amd import _lib
    H, W = 70, 90
    mask = ragged_mask(H, W, 12)
    img = synth(H, W, 8, seed=66)
    ys, xs = np.nonzero(mask == 0)
    img[ys[3], xs[3], 5] = np.nan
    dev = torch.as_tensor(img).cuda()
    kw = dict(n_segments=60, compactness=10.0, max_num_iter=4, _normalize_bands=True, mask=mask, convert2lab=False)
    errs = []
    for fused in (True, False):
        with pytest.raises(Exception) as e:
            stages(dev, fused, **kw)
        errs.append(f"{type(e.value).__name__}: {e.value}")
    print("NaN under the mask:", errs)
    assert "input raster holds NaN" in errs[0], errs[0]
    assert errs[0] == errs[1]
    # (and the library did decide to fuse this call: the same call without the NaN does)
    img[ys[3], xs[3], 5] = 1000.0
    _, px = stages(torch.as_tensor(img).cuda(), True, **kw)
    assert px == H * W


def test_arena_reuse_fused_unfused_fused():
    """one context: the planes of a call hold whatever the call before left there until a sweep writes them"""
    from obia_amd import _lib
    ctx = _lib.Context(0)
    mask = np.ones((300, 280), bool)
    mask[50:60, 100:140] = False
    dev = torch.as_tensor(synth(300, 280, 8, seed=65)).cuda()
    a = tiler(dev, mask, True, ctx=ctx, **KW)
    b = tiler(dev, mask, False, ctx=ctx, **KW)
    c = tiler(dev, mask, True, ctx=ctx, **KW)
    assert a[1] == b[1] == c[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
    assert a[2]["feature_fused_px"] == c[2]["feature_fused_px"] > 0 and b[2]["feature_fused_px"] == 0
