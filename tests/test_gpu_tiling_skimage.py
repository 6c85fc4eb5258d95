"""``create_tiled_segments(..., seeding="skimage")`` on the GPU -- every tile seeded as scikit-image seeds maskSLIC, picks from NumPy,
k-means and steps in the library -- against the CPU reference tests/tiler_skimage_restatement.py (the oracle's tile loops, the NumPy
restatement of the seeding, the pinned SLIC oracle on those seeds).  Every comparison is equality of the label rasters and of the segment
counts: the seeding is bit-exact (tests/test_gpu_mask_seeds.py), the sweeps cannot flip a pixel at compactness >= 5 and are
bit-exact at any compactness against the oracle with integer sums (tests/test_gpu_exact_sums.py).  The rasters are the smallest that
reach every branch: black and white tiles, clipped and grown windows, corner squares, an empty tile, small tiles, both k-means point
sets."""
import numpy as np
import pytest

from tests import tiler_skimage_restatement as TR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def synth(H, W, C, seed=0):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([400 * np.sin(xx / (11 + 3 * c)) * np.cos(yy / (13 + 2 * c)) + 1000 + 50 * c + rs.normal(0, 20, (H, W))
                     for c in range(C)], -1).astype(np.float32)


def checkerboard_case():
    """96 x 128 x 4, 3 x 4 tiles of 32, buffer 8: a mask with holes and one fully masked tile"""
    img = synth(96, 128, 4, seed=5)
    yy, xx = np.mgrid[0:96, 0:128]
    mask = np.ones((96, 128), bool)
    mask[(yy - 40) ** 2 + (xx - 50) ** 2 < 9 ** 2] = False          # a hole across the seam of four tiles
    mask[(yy - 80) ** 2 * 3 + (xx - 100) ** 2 < 11 ** 2] = False    # one inside a white tile's grown window
    mask[60:64, 0:20] = False
    mask[0:32, 64:96] = False                                       # black tile (0, 2): empty
    return img, mask, dict(tile_size=32, buffer=8, n_segments=12, compactness=10.0)


def gpu(img, mask, device=True, **kw):
    from obia_amd.tiling import create_tiled_segments
    lab, n = create_tiled_segments(torch.as_tensor(img).cuda() if device else img, input_mask=mask, **kw)
    return (lab.cpu().numpy() if device else lab), n


def same(lab, n, ref, n_ref, what=""):
    assert lab.shape == ref.shape and n == n_ref and np.array_equal(lab, ref), f"{what}: {(lab != ref).sum()} px differ, n {n} vs {n_ref}"


@pytest.fixture(scope="module")
def board(oracle):
    """the checkerboard case and its references, computed once: the restatement in both white orders (with its per-tile info), the
    grid oracle, and the GPU result under seeding="skimage" """
    img, mask, kw = checkerboard_case()
    from oracle import tiler
    info = []
    out = dict(img=img, mask=mask, kw=kw, info=info)
    out["ref"] = TR.create_tiled_segments(img, mask, tile_info=info, **kw)
    out["ref_parity"] = TR.create_tiled_segments(img, mask, white_order=1, **kw)
    out["grid_ref"] = tiler.create_tiled_segments(img, mask, **kw)
    out["gpu"] = gpu(img, mask, seeding="skimage", **kw)
    return out


def test_checkerboard_is_exact(board):
    info = board["info"]
    wins = {t["window"] for t in info}
    assert (0, 0, 32, 32) in wins and (0, 24, 40, 48) in wins and (24, 0, 48, 40) in wins and (56, 88, 40, 40) in wins   # exact, clipped and grown windows
    assert any(t["skipped"] == "empty" and t["n_valid"] == 0 for t in info)                 # the fully masked black tile
    assert len(info) == 12 and sum(t["skipped"] is None for t in info) == 11
    lab, n = board["gpu"]
    assert lab.dtype == np.int32 and (lab[~board["mask"]] == 0).all()
    same(lab, n, *board["ref"], "checkerboard")
    ids = np.unique(lab[lab > 0])
    assert ids[0] == 1 and ids[-1] == n and len(ids) == n


def test_low_compactness_is_exact_with_integer_sums(oracle, board):
    oracle.set_sum_mode(1)
    try:
        kw = dict(board["kw"], compactness=0.25)
        ref, n_ref = TR.create_tiled_segments(board["img"], board["mask"], **kw)
    finally:
        oracle.set_sum_mode(0)
    same(*gpu(board["img"], board["mask"], seeding="skimage", **kw), ref, n_ref, "compactness 0.25")


def test_ragged_raster_crown_rule_half_metre_pixels(oracle):
    img = synth(70, 90, 4, seed=6)
    yy, xx = np.mgrid[0:70, 0:90]
    mask = (yy - 30) ** 2 + (xx - 48) ** 2 < 47 ** 2
    kw = dict(tile_size=32, buffer=7, crown_radius=2.6, pixel_size=(0.5, 0.5), compactness=10.0)   # ~12 segments per full tile
    info = []
    ref, n_ref = TR.create_tiled_segments(img, mask, tile_info=info, **kw)
    assert {t["window"][2:] for t in info} >= {(32, 32), (6, 26), (39, 46), (13, 46)} and sum(t["skipped"] is None for t in info) >= 6
    same(*gpu(img, mask, seeding="skimage", **kw), ref, n_ref, "ragged")


def small_tile_cases():
    img = synth(64, 96, 4, seed=7)
    base = np.ones((64, 96), bool)
    base[0:32, 32:64] = False                       # white tile (0, 1) emptied, then given back a few pixels
    one, two, few = base.copy(), base.copy(), base.copy()
    one[10, 40] = True
    two[10, 40:42] = True
    few[8:14, 36:50] = True                         # 84 valid pixels at 12 per 1024: n = round(0.98) = 1
    sane = dict(tile_size=32, buffer=0, n_segments=12, compactness=10.0)
    # a density that asks for segments of single pixels: n = round(1.57 * n_valid) >= 2 on ONE valid pixel (skipped for n_valid < 2),
    # and K = min(n, n_valid) = n_valid everywhere else -- every valid pixel a centroid
    dense = dict(tile_size=16, buffer=0, crown_radius=0.45, pixel_size=(1.0, 1.0), compactness=10.0)
    dimg = img[:32, :48]
    d1 = np.ones((32, 48), bool)
    d1[:16, 16:32] = False
    d1[5, 20] = True
    d2 = d1.copy()
    d2[5, 21] = True
    return {"one_valid": (img, one, sane, (1, 0)), "two_valid": (img, two, sane, (2, 0)), "n_is_1": (img, few, sane, (84, 1)),
            "one_valid_n2": (dimg, d1, dense, (1, 2)), "two_valid_n3": (dimg, d2, dense, (2, 3))}


@pytest.mark.parametrize("name", ["one_valid", "two_valid", "n_is_1", "one_valid_n2", "two_valid_n3"])
def test_small_tiles(oracle, name):
    img, mask, kw, (nv, n_tile) = small_tile_cases()[name]
    info = []
    ref, n_ref = TR.create_tiled_segments(img, mask, tile_info=info, **kw)
    tile = [t for t in info if t["n_valid"] == nv]
    assert len(tile) == 1 and tile[0]["n"] == n_tile
    if name == "two_valid_n3":
        assert tile[0]["skipped"] is None and tile[0]["K"] == 2          # two valid pixels and n >= 2: seeded, two centroids
    else:
        assert tile[0]["skipped"] == ("small" if n_tile >= 1 else "empty")
        y0, x0, h, w = tile[0]["window"]
        assert (ref[y0:y0 + h, x0:x0 + w] == 0).all()
    same(*gpu(img, mask, seeding="skimage", **kw), ref, n_ref, name)


def test_both_kmeans_point_sets(oracle):
    """9 segments per full tile: a full tile draws 900 of its 1024 valid pixels as k-means points, a tile with 180 valid pixels
    (n = 2, 200 >= 180) runs k-means on all of them"""
    img = synth(64, 96, 4, seed=8)
    mask = np.ones((64, 96), bool)
    mask[0:32, 32:64] = False
    mask[6:18, 38:53] = True                        # 180 valid pixels in the white tile (0, 1)
    kw = dict(tile_size=32, buffer=0, n_segments=9, compactness=10.0)
    info = []
    ref, n_ref = TR.create_tiled_segments(img, mask, tile_info=info, **kw)
    seeded = [t for t in info if t["skipped"] is None]
    assert any(t["n_dense"] is None and t["n_valid"] <= 100 * t["n"] for t in seeded), "no tile ran k-means on every valid pixel"
    assert any(t["n_dense"] is not None and t["n_dense"] < t["n_valid"] for t in seeded), "no tile drew its k-means points"
    same(*gpu(img, mask, seeding="skimage", **kw), ref, n_ref, "dense branches")


def test_the_argument_is_not_ignored_and_grid_is_unchanged(board):
    lab, n = board["gpu"]
    glab, gn = gpu(board["img"], board["mask"], seeding="grid", **board["kw"])
    assert not np.array_equal(lab, glab), 'seeding="skimage" gave the grid rule\'s raster'
    same(glab, gn, *board["grid_ref"], "grid rule")
    dlab, dn = gpu(board["img"], board["mask"], **board["kw"])          # the default is the grid rule
    assert dn == gn and np.array_equal(dlab, glab)


def test_sharded_driver_on_one_rank(board):
    """The existing distributed GPU tests run the ranks as threads of one process on the one GPU (ThreadComm); so does this one, with a
    single rank: the session entry points (obia_tiler_set_seeding, obia_tiler_run) in the sharded driver's parity order."""
    from obia_amd import _lib
    from obia_amd.distributed import ShardedTiler, ThreadComm
    img, mask, kw = board["img"], board["mask"], board["kw"]
    t = ShardedTiler(torch.as_tensor(img).cuda(), torch.as_tensor(mask.astype(np.uint8)).cuda(), 96, 3, kw["tile_size"], kw["buffer"],
                     comm=ThreadComm.make(1)[0], ctx=_lib.Context(0), n_segments=kw["n_segments"], compactness=kw["compactness"],
                     seeding="skimage")
    try:
        lab, n = t.run()
        assert t.engine.picks.calls > 0 and t.engine.picks.error is None
    finally:
        t.close()
    same(lab.cpu().numpy(), n, *board["ref_parity"], "one rank, parity order")
    plab, pn = gpu(img, mask, seeding="skimage", white_order="parity", **kw)
    same(plab, pn, *board["ref_parity"], "one-shot call, parity order")


def test_two_runs_are_bit_identical(board):
    lab, n = board["gpu"]
    again, n2 = gpu(board["img"], board["mask"], seeding="skimage", **board["kw"])
    assert n2 == n and np.array_equal(again, lab)
    host, n3 = gpu(board["img"], board["mask"], device=False, seeding="skimage", **board["kw"])      # (the host-pointer entry)
    assert host.dtype == np.int32 and n3 == n and np.array_equal(host, lab)


def test_abi_refusals_and_a_failing_pick_function():
    import ctypes
    from obia_amd import _lib
    from obia_amd.segmentation import make_params
    lib, c = _lib.load(), _lib.default_context(0)
    img = torch.as_tensor(synth(32, 32, 2, seed=9)).cuda()
    out = torch.empty((32, 32), dtype=torch.int32, device="cuda")
    tp = _lib.TilingParams()
    tp.tile_size, tp.buffer, tp.crown_radius, tp.pixel_width, tp.pixel_height = 32, 0, 5.0, 1.0, 1.0
    params = make_params(n_segments=8, normalize_bands=True)
    n = ctypes.c_int64(0)

    def call(seeding, fn):
        return lib.obia_tiled_slic_seeded_f32_dev(c.handle, img.data_ptr(), None, 32, 32, 2, ctypes.byref(tp), ctypes.byref(params), seeding,
                                                  fn, None, out.data_ptr(), ctypes.byref(n))
    assert call(_lib.SEEDING_SKIMAGE, _lib.PickFn()) == _lib.E_INVALID and "pick function" in _lib.last_error()
    assert call(7, _lib.PickFn()) == _lib.E_INVALID
    assert call(_lib.SEEDING_SKIMAGE, _lib.PickFn(lambda *a: 1)) == _lib.E_INVALID and "pick function failed" in _lib.last_error()
    keep = np.arange(8, dtype=np.int64)[::-1].copy()      # eight ranks as asked for, not ascending

    def unsorted(user, n_valid, n_seg, idx, n_idx, dense, n_dense):
        idx[0], n_idx[0], dense[0], n_dense[0] = keep.ctypes.data, n_seg, None, 0
        return 0
    assert call(_lib.SEEDING_SKIMAGE, _lib.PickFn(unsorted)) == _lib.E_INVALID and "bad picks" in _lib.last_error()
    assert call(_lib.SEEDING_GRID, _lib.PickFn()) == _lib.OBIA_OK and n.value > 0      # the context is still good
