"""The training tiles, host side: the NumPy restatement (tests/training_restatement.py) against things outside it -- the blur against
SciPy's correlate1d in exact dyadic float64, the chamfer sweep against its closed form and against the Euclidean transform's bounds,
the tile windows against plain float arithmetic, the annotations against boxes worked out by hand --, the host functions of
obia_amd.training against the restatement, and the argument checks that fire before the device is touched.

cv2.GaussianBlur and cv2.distanceTransform are restated from OpenCV's algorithms and are NOT compared with cv2 anywhere."""
import numpy as np
import pytest

from tests import training_restatement as T

BLUR_SHAPES = ((1, 1), (2, 3), (3, 7), (9, 4), (13, 17), (70, 131))
BLUR_KERNELS = ((5, 5), (11, 11), (11, 5), (7, 31), (1, 9))


def random_mask(shape, density, seed):
    """uint8 plane, non-zero with probability `density`"""
    return (np.random.RandomState(seed).rand(*shape) < density).astype(np.uint8) * 255


# ---- weights and blur ------------------------------------------------------------------------------------------------------------
def test_weights():
    for k in range(1, 32, 2):
        w = T.gaussian_weights(k)
        assert len(w) == k and int(w.sum()) == 256 and np.array_equal(w, w[::-1]) and (w >= 0).all(), k
    for k, table in T.SMALL.items():
        assert T.gaussian_weights(k).tolist() == table
    assert T.gaussian_weights(11).tolist()[:6] == [2, 7, 17, 31, 45, 52]


def test_library_weights_are_the_restatements():
    pytest.importorskip("torch")
    from obia_amd.training import gaussian_weights
    for k in range(1, 32, 2):
        w = gaussian_weights(k)
        assert w.dtype == np.int32 and w.tolist() == T.gaussian_weights(k).tolist()
    for bad in (0, 2, 33, -3, 5.0, "5", None, True):
        with pytest.raises(ValueError, match="odd integer in 1..31"):
            gaussian_weights(bad)


@pytest.mark.parametrize("shape", BLUR_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in BLUR_SHAPES])
def test_blur_is_scipy_correlate1d_exactly(shape):
    """all terms are dyadic and below 2^24, so the float64 correlation is exact; 'mirror' is REFLECT_101, repeated"""
    ndi = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(shape[0] * 131 + shape[1])
    for nch in (1, 3):
        img = rs.randint(0, 256, shape + ((3,) if nch == 3 else ()), dtype=np.uint8)
        for kx, ky in BLUR_KERNELS:
            wx, wy = T.gaussian_weights(kx) / 256.0, T.gaussian_weights(ky) / 256.0
            p = img.astype(np.float64)
            want = np.floor(ndi.correlate1d(ndi.correlate1d(p, wx, axis=1, mode="mirror"), wy, axis=0, mode="mirror") + 0.5)
            got = T.blur_u8(img, (kx, ky))
            assert got.dtype == np.uint8 and got.shape == img.shape
            assert np.array_equal(got, want.astype(np.uint8)), (shape, nch, kx, ky)


def test_blur_by_hand():
    flat = np.full((6, 5, 3), 77, np.uint8)
    assert np.array_equal(T.blur_u8(flat, 11), flat)                          # the weights sum to 256 on each axis
    one = np.zeros((5, 5), np.uint8)
    one[2, 2] = 255
    want = (np.outer([64, 128, 64], [64, 128, 64]) * 255 + 32768) >> 16
    assert np.array_equal(T.blur_u8(one, 3)[1:4, 1:4], want)
    assert T.blur_u8(one, 0) is one and T.blur_u8(one, (0, 0)) is one
    assert [T.reflect101(p, 3) for p in range(-5, 8)] == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert [T.reflect101(p, 1) for p in (-2, 0, 5)] == [0, 0, 0]
    assert [T.reflect101(p, 2) for p in range(-3, 4)] == [1, 0, 1, 0, 1, 0, 1]


# ---- distance --------------------------------------------------------------------------------------------------------------------
SWEEP_CASES = [((7, 9), 0.5, 1), ((12, 5), 0.8, 2), ((1, 13), 0.7, 3), ((13, 1), 0.7, 4), ((20, 23), 0.95, 5), ((16, 16), 0.99, 6),
               ((9, 9), 1.1, 7), ((1, 1), 0.0, 8), ((1, 1), 1.1, 9), ((25, 31), 0.9, 10)]


@pytest.mark.parametrize("shape,density,seed", SWEEP_CASES)
def test_the_two_pass_sweep_is_its_closed_form(shape, density, seed):
    """what lets the kernels evaluate the minimum directly; density 1.1 is a plane without a zero pixel"""
    src = random_mask(shape, density, seed)
    sweep = T.chamfer_sweep_fixed(src)
    assert np.array_equal(sweep, T.chamfer_closed_form_fixed(src))
    if density > 1:
        assert (sweep == T.DIST_MAX).all() and (T.to_float(sweep) == 8192.0).all()
    assert (T.to_float(sweep)[src == 0] == 0).all()


def test_the_chamfer_distance_brackets_the_euclidean_one():
    """a = 0.955 along an axis, b = 1.3693 along a diagonal: a path of m diagonal and n - m axis steps measures between a times and
    sqrt(a^2 + (b - a)^2) times the Euclidean length of its offset"""
    ndi = pytest.importorskip("scipy.ndimage")
    for seed in range(4):
        src = random_mask((30, 37), 0.97, 20 + seed)
        src[3, 4] = 0
        t = T.chamfer_sweep_fixed(src) / 65536.0
        edt = ndi.distance_transform_edt(src)
        assert (t >= 0.9549 * edt).all() and (t <= 1.0411 * edt).all()


@pytest.mark.parametrize("R", [0, 1, 3, 6])
def test_the_window_changes_nothing_below_R_axis_steps(R):
    for seed, density in ((30, 0.9), (31, 0.99)):
        src = random_mask((21, 26), density, seed)
        src[10, 13] = 0
        full, win = T.chamfer_closed_form_fixed(src), T.chamfer_closed_form_fixed(src, R)
        near = full < R * T.HV
        assert np.array_equal(win[near], full[near]) and (win >= full).all()
        assert (win[~near] >= R * T.HV).all()
    alone = np.full((9, 9), 255, np.uint8)
    alone[0, 0] = 0                                                          # just outside the window of (4, 4) for R = 3
    assert T.chamfer_windowed(alone, 3)[4, 4] == 8192.0 and T.chamfer_windowed(alone, 4)[4, 4] == np.float32(4 * T.DG) / 65536


# ---- blends and min-max by hand --------------------------------------------------------------------------------------------------
def test_darken_blend_minmax_by_hand():
    b = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert T.darken(b, 0) is b and np.array_equal(T.darken(b, 1), b)
    assert T.darken(b, 0.8)[15, 15] == 204 and T.darken(b, 0.2)[0, 9] == 1
    tile = np.full((2, 2, 3), 200, np.uint8)
    bg = np.full((2, 2, 3), 40, np.uint8)
    mask = np.array([[1, 0], [0, 1]], np.uint8)
    assert T.blend_hard(tile, bg, mask)[:, :, 0].tolist() == [[200, 40], [40, 200]]
    dist = np.array([[0.0, 0.955], [1.91, 8192.0]], np.float32)
    out = T.blend_feather(tile, bg, dist, 0.955)
    assert out[:, :, 1].tolist() == [[200, 40], [40, 40]]                    # dist == feather: alpha is exactly 0
    assert T.blend_feather(tile, bg, dist, 1.91)[0, 1, 0] == 120             # alpha = 0.5
    x = np.array([[-3.0, 1.0], [5.0, 2.0]], np.float32)
    assert T.minmax_u8(x).tolist() == [[0, 127], [255, 159]]
    assert not T.minmax_u8(np.full((3, 2), 7.5, np.float32)).any()


# ---- tiling ----------------------------------------------------------------------------------------------------------------------
TILINGS = [((96, 120), [0.5, 0, 0, -0.5, 1000.0, 5000.0], 20.0, 5.0), ((50, 70), [2.0, 0, 0, -2.0, -300.0, 80.0], 40.0, 0.0),
           ((33, 17), [0.25, 0, 0, -0.5, 0.0, 0.0], 8.0, 4.0), ((10, 10), [1.0, 0, 0, -1.0, 5.0, 5.0], 64.0, 32.0)]


@pytest.mark.parametrize("shape,affine,tile_size,overlap", TILINGS)
def test_tile_windows_against_the_generator_in_floats(shape, affine, tile_size, overlap):
    pytest.importorskip("torch")
    from obia_amd import training as tr
    wins, transforms = tr.tile_windows(shape, affine, tile_size, overlap)
    want_w, want_t = T.windows(shape, affine, tile_size, overlap)
    assert wins == want_w and transforms == want_t
    a, _, _, e, xoff, yoff = affine
    bounds = (xoff, yoff + e * shape[0], xoff + a * shape[1], yoff)
    assert list(tr.generate_tiles(bounds, tile_size - overlap, tile_size)) == list(T.generate_tiles(bounds, tile_size - overlap, tile_size))
    assert len(wins) == len(list(T.generate_tiles(bounds, tile_size - overlap, tile_size)))
    covered = np.zeros(shape, bool)
    for r, c, h, w in wins:
        assert 0 <= r and r + h <= shape[0] and 0 <= c and c + w <= shape[1] and h > 0 and w > 0
        covered[r:r + h, c:c + w] = True
    assert covered.all()
    assert wins[0][0] + wins[0][2] == shape[0] and wins[0][1] == 0            # the first tile is the bottom-left one


def test_the_documented_tiling():
    """96 x 120 at 0.5 m, tile_size 20, overlap 5: 40-pixel tiles every 30 pixels; the last column is 30 wide, the top row 6 high"""
    wins, transforms = T.windows((96, 120), [0.5, 0, 0, -0.5, 1000.0, 5000.0], 20.0, 5.0)
    assert len(wins) == 16 and wins[0] == (56, 0, 40, 40) and wins[3] == (56, 90, 40, 30) and wins[12] == (0, 0, 6, 40)
    assert transforms[0] == [0.5, 0, 1000.0, 0, -0.5, 4972.0] and transforms[3][2] == 1045.0


def test_tile_windows_refusals():
    pytest.importorskip("torch")
    from obia_amd.training import tile_windows
    north_up = [0.5, 0, 0, -0.5, 0.0, 0.0]
    for affine in ([0.5, 0.1, 0, -0.5, 0, 0], [0.5, 0, 0.1, -0.5, 0, 0], [-0.5, 0, 0, -0.5, 0, 0], [0.5, 0, 0, 0.5, 0, 0]):
        with pytest.raises(ValueError, match="north-up"):
            tile_windows((10, 10), affine, 4.0, 1.0)
    for tile_size, overlap in ((4.0, 4.0), (4.0, 5.0), (0.0, -1.0)):
        with pytest.raises(ValueError, match="overlap must be smaller than tile_size"):
            tile_windows((10, 10), north_up, tile_size, overlap)
    for tile_size, overlap in ((4.2, 1.0), (4.0, 0.75), (0.3, 0.0)):
        with pytest.raises(ValueError, match="whole number of pixels"):
            tile_windows((10, 10), north_up, tile_size, overlap)
    with pytest.raises(ValueError, match="empty"):
        tile_windows((0, 10), north_up, 4.0, 1.0)
    assert len(tile_windows((10, 10), north_up, 4.0 + 1e-12, 1.0)[0]) == 4    # whole to within 1e-9 relative


def test_annotations_on_hand_made_boxes():
    """96 x 120 at 0.5 m from (1000, 5000): tile 1 covers x 1000..1020, y 4952..4972; tile 2 x 1015..1035, the same rows"""
    pytest.importorskip("torch")
    from obia_amd.training import tile_annotations, tile_windows
    shape, affine = (96, 120), [0.5, 0, 0, -0.5, 1000.0, 5000.0]
    bounds = np.array([[1002.3, 4960.2, 1006.8, 4966.9],         # inside tile 1 only
                       [1016.2, 4953.1, 1018.9, 4955.7],         # in the overlap of tiles 1 and 2
                       [1012.0, 4956.0, 1017.0, 4958.0],         # straddles the left edge of tile 2 (x = 1015): inside tile 1 only
                       [1019.0, 4960.0, 1021.0, 4962.0],         # straddles the right edge of tile 1 (x = 1020): inside tile 2 only
                       [1012.0, 4971.0, 1022.0, 4974.0],         # wider than the overlap and across it: within no tile of either row
                       [1030.1, 4953.1, 1030.4, 4953.4]])        # inside tiles 2 and 3, less than a pixel: degenerate
    want = T.annotations(bounds, shape, affine, 20.0, 5.0)
    wins, _ = tile_windows(shape, affine, 20.0, 5.0)
    got = tile_annotations(bounds, affine, wins, [f"img_{i + 1:03d}.jpg" for i in range(len(wins))])
    assert got == want
    assert sorted(got) == ["img_001", "img_002", "img_003"]
    assert got["img_001"] == {"file_name": "img_001.jpg", "boxes": [[4, 10, 13, 23], [32, 32, 37, 37], [24, 28, 34, 32]], "labels": [1, 1, 1]}
    assert got["img_002"]["boxes"] == [[2, 32, 7, 37], [8, 20, 12, 24]]
    assert got["img_003"] == {"file_name": "img_003.jpg", "boxes": [], "labels": []}      # the key exists: a polygon lies within
    assert all(isinstance(v, int) for b in got["img_001"]["boxes"] for v in b)


def test_restatement_tiles_are_at_least_8_by_8_in_the_end_to_end_case():
    """the raster of tests/test_gpu_training.py: CLAHE needs 8 x 8"""
    wins, _ = T.windows((98, 120), [0.5, 0, 0, -0.5, 1000.0, 5000.0], 20.0, 5.0)
    assert len(wins) == 16 and min(min(h, w) for _, _, h, w in wins) == 8
    assert {(h, w) for _, _, h, w in wins} == {(40, 40), (40, 30), (38, 40), (38, 30), (8, 40), (8, 30)}


# ---- argument checks: no device work ---------------------------------------------------------------------------------------------
def test_refusals_before_the_device_is_touched():
    pytest.importorskip("torch")
    from obia_amd import training as tr
    tile = np.zeros((16, 16, 3), np.float32)
    mask = np.ones((16, 16), np.uint8)
    for kw, match in ((dict(darken_factor=1.5), "darken_factor"), (dict(darken_factor=-0.1), "darken_factor"),
                      (dict(darken_factor=float("nan")), "darken_factor"), (dict(feather_radius=-1.0), "feather_radius"),
                      (dict(feather_radius=float("inf")), "feather_radius"), (dict(blur_kernel=4), "odd integer"),
                      (dict(blur_kernel=33), "odd integer"), (dict(blur_kernel=(5, 0)), "odd integer"), (dict(blur_kernel=5.0), "int or a"),
                      (dict(blur_kernel=(5, 5, 5)), "int or a")):
        with pytest.raises(ValueError, match=match):
            tr.process_tile(tile, mask, **kw)
    with pytest.raises(ValueError, match=r"\(h, w, 3\)"):
        tr.process_tile(np.zeros((16, 16), np.float32))
    with pytest.raises(TypeError, match="float64"):
        tr.process_tile(np.zeros((16, 16, 3), np.float64))
    with pytest.raises(ValueError, match="the mask is"):
        tr.process_tile(tile, np.ones((16, 15), np.uint8))
    with pytest.raises(ValueError, match="8 x 8"):
        tr.process_tile(np.zeros((7, 16, 3), np.float32))
    with pytest.raises(TypeError, match="uint8"):
        tr.gaussian_blur_u8(np.zeros((4, 4), np.float32), 3)
    with pytest.raises(ValueError, match="odd integer"):
        tr.gaussian_blur_u8(np.zeros((4, 4), np.uint8), (3, 2))
    img = np.zeros((4, 4), np.uint8)
    assert tr.gaussian_blur_u8(img, 0) is img and tr.gaussian_blur_u8(img, (0, 0)) is img
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        tr.chamfer_distance(np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(ValueError, match="radius"):
        tr.chamfer_distance(img, -1)
    with pytest.raises(NotImplementedError, match="4096"):
        tr.chamfer_distance(np.zeros((1, 4097), np.uint8))
    raster = np.zeros((40, 40, 5), np.float32)
    affine = [0.5, 0, 0, -0.5, 0.0, 0.0]
    with pytest.raises(IndexError, match="Band index 5 out of range"):
        tr.tile_and_process(raster, affine, "EPSG:32610", selected_bands=(5, 1, 0))
    with pytest.raises(ValueError, match="exactly three"):
        tr.tile_and_process(raster, affine, "EPSG:32610", selected_bands=(1, 0))
    with pytest.raises(ValueError, match="whole number of pixels"):
        tr.tile_and_process(raster, affine, "EPSG:32610", tile_size=10.3, overlap=2.0)
    with pytest.raises(ValueError, match="the mask is"):
        tr.tile_and_process(raster, affine, "EPSG:32610", mask=np.ones((40, 41), np.uint8), tile_size=10.0, overlap=2.0)
    with pytest.raises(ValueError, match=r"\(N, 4\)"):
        tr.tile_and_process(raster, affine, "EPSG:32610", boxes=np.zeros((3, 5)), tile_size=10.0, overlap=2.0)
    with pytest.raises(ValueError, match=r"img_003\.jpg: apply_clahe needs at least 8 x 8"):
        tr.tile_and_process(raster, affine, "EPSG:32610", tile_size=9.0, overlap=0.0)      # 18-pixel tiles, the third is 4 wide
    with pytest.raises(TypeError, match="float32"):
        tr.tile_and_process(raster.astype(np.float64), affine, "EPSG:32610")


def test_the_package_exports_the_module():
    pytest.importorskip("torch")
    import obia_amd
    assert obia_amd.tile_and_process is obia_amd.training.tile_and_process
    assert obia_amd.process_tile is obia_amd.training.process_tile and obia_amd.TrainingTiles is obia_amd.training.TrainingTiles
