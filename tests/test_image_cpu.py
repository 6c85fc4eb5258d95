"""Image previews, host side: the CPU restatement (tests/image_restatement.py) against NumPy, against the committed scikit-image
goldens and against answers worked out by hand; the argument checks of obia_amd.image / Segments.to_segmented_image that fire before
any device work.

The OpenCV parts (grey conversion, equalizeHist, CLAHE) are restated from OpenCV's algorithm and are NOT compared with cv2 anywhere."""
import glob
import os

import numpy as np
import pytest

from tests import image_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "boundaries", "*.npz")))


# ---- rescale_to_8bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.uint16, np.uint8, np.int16])
@pytest.mark.parametrize("pq", [(2, 98), (0, 100), (25, 25), (50, 50.0001)])
def test_restatement_rescale_is_the_reference_lines(dtype, pq):
    rs = np.random.RandomState(3)
    image = (rs.normal(900, 300, (7, 13, 3)).clip(0, 4000)).astype(dtype) if dtype != np.uint8 else rs.randint(0, 256, (7, 13, 3)).astype(dtype)
    p_min, p_max = np.percentile(image, pq)                                  # obia/utils/image.py:27-36, literally
    if p_min == p_max:
        want = np.zeros(image.shape, dtype=np.uint8)
    else:
        want = np.clip(255 * (image - p_min) / (p_max - p_min), 0, 255).astype(np.uint8)
    got = R.rescale_to_8bit(image, *pq)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    if dtype == np.float32:
        assert np.asarray(p_min).dtype == np.float64                         # NumPy >= 2: a float32 image gives float64 percentiles
    if pq == (25, 25):
        assert not got.any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 2, 5, 101, 4099])
def test_host_interpolation_is_np_percentile(dtype, n):
    """obia_amd._percentile.lerp turns the four order statistics the device selects into np.percentile(x, (p_lo, p_hi))"""
    from obia_amd import _percentile
    rs = np.random.RandomState(n)
    x = rs.normal(0, 50, n).astype(dtype)
    v = np.sort(x)
    for pq in [(2, 98), (0, 100), (25, 25), (50, 50.0001), (10, 75)]:        # n = 101: (n - 1) * q is an integer
        q = _percentile.quantiles(*pq)
        vi = (n - 1) * q
        ia = np.where(vi >= n - 1, n - 1, np.floor(vi)).astype(np.int64)
        ib = np.where(vi >= n - 1, n - 1, ia + 1)
        got = _percentile.lerp(n, v[ia], v[ib], dtype, q)
        want = np.percentile(x, pq)
        assert got.dtype == np.float64 and want.dtype == np.float64
        assert np.array_equal(got, want), (pq, got, want)


# ---- boundaries against scikit-image 0.18.3 -----------------------------------------------------------------------------------
def test_goldens_are_there():
    assert len(GOLDENS) >= 8
    assert all(os.path.getsize(p) < 16 * 1024 for p in GOLDENS)


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_restatement_boundaries_match_skimage(path):
    g = np.load(path)
    assert str(g["skimage_version"]) == "0.18.3"
    lab = g["labels"]
    assert lab.dtype == np.int32
    assert np.array_equal(R.find_boundaries(lab).astype(np.uint8), g["boundaries"])
    assert np.array_equal(R.find_boundaries(lab.astype(np.int64)).astype(np.uint8), g["boundaries"])    # the reference's int64 labels
    assert np.array_equal(R.mark_u8(g["image"], lab), g["marked"])


def test_mark_table_is_not_the_identity_and_matches_skimage():
    """away from the boundaries the overlay is trunc(v * (1 / 255) * 255) in float64 (img_as_float multiplies by the reciprocal):
    24 of the 256 values come back one lower"""
    from obia_amd.image import mark_table
    t = mark_table()
    assert np.array_equal(t, R.mark_table())
    v = np.arange(256)
    assert int((t != v).sum()) == 24 and np.all((t == v) | (t == v - 1))
    g = np.load(os.path.join(ROOT, "tests", "golden", "boundaries", "allvalues_rgb_16x16.npz"))
    inside = g["boundaries"] == 0
    assert set(g["image"][inside].ravel().tolist()) >= set(np.flatnonzero(t != v).tolist())  # the golden sees every such value
    assert np.array_equal(g["marked"][inside], t[g["image"][inside]])


def test_neighbours_outside_the_raster_do_not_count():
    assert not R.find_boundaries(np.full((3, 4), 7, np.int32)).any()
    assert not R.find_boundaries(np.full((1, 1), -1, np.int32)).any()


# ---- equalisation by hand ----------------------------------------------------------------------------------------------------
def test_gray_weights():
    rgb = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]], np.uint8)
    # (9798 R + 19235 G + 3735 B + 16384) >> 15: 9798 + 19235 + 3735 = 32768, so white stays 255
    want = [255, 0, (9798 * 255 + 16384) >> 15, (19235 * 255 + 16384) >> 15, (3735 * 255 + 16384) >> 15,
            (97980 + 384700 + 112050 + 16384) >> 15]
    assert R.rgb_to_gray(rgb)[0].tolist() == want == [255, 0, 76, 150, 29, 18]


def test_equalize_two_values():
    img = np.array([[10, 10, 10, 200], [10, 200, 200, 200]], np.uint8)     # first bin 10 holds 4 of 8: scale = 255 / 4
    out = R.equalize_hist(img)                                             # lut[10] = 0, lut[200] = round(4 * 63.75) = 255
    assert np.array_equal(out, np.where(img == 10, 0, 255))
    three = np.array([[5, 6, 7, 7]], np.uint8)                             # scale = 255 / 3: lut[6] = 85, lut[7] = 255
    assert R.equalize_hist(three).tolist() == [[0, 85, 255, 255]]
    assert np.array_equal(R.apply_histogram_equalization(three), np.stack([R.equalize_hist(three)] * 3, -1))


def test_equalize_constant_is_unchanged():
    img = np.full((5, 4), 93, np.uint8)
    assert np.array_equal(R.equalize_hist(img), img)
    assert R.equalize_lut(np.bincount(img.ravel(), minlength=256)) is None


def test_library_table_equals_the_restatement():
    from obia_amd.image import equalization_table
    rs = np.random.RandomState(5)
    for k in range(20):
        hist = rs.randint(0, 5000, 256) * (rs.rand(256) < rs.rand())
        hist[rs.randint(256)] += 1
        a, b = equalization_table(hist), R.equalize_lut(hist)
        assert (a is None) == (b is None)
        assert a is None or np.array_equal(a, b)
    big = np.zeros(256, np.int64)
    big[[3, 100, 255]] = [2 ** 30, 2 ** 29 + 1, 7]                           # sums past 2^24: int -> float32 rounds
    assert np.array_equal(equalization_table(big), R.equalize_lut(big))
    assert equalization_table(np.eye(256, dtype=np.int64)[9] * 12) is None


# ---- CLAHE by hand -----------------------------------------------------------------------------------------------------------
def test_clahe_8x8_tiles_of_one_pixel():
    """8 x 8: every tile is one pixel, clip = max(int(2 * 1 / 256), 1) = 1, lutScale = 255: the table of the tile holding value c is
    the step 0 below c, 255 from c on.  Pixel x lies half way between the tiles x - 1 and x (clamped at the border), so its result is
    255 * k / 4 with k = the number of the four tiles (y - 1 | y, x - 1 | x) whose value is <= its own: 63.75 -> 64, 127.5 -> 128
    (half to even), 191.25 -> 191, 255."""
    rs = np.random.RandomState(11)
    img = rs.randint(0, 256, (8, 8)).astype(np.uint8)
    luts, th, tw = R.clahe_luts(img)
    assert (th, tw) == (1, 1)
    for ty in range(8):
        for tx in range(8):
            assert np.array_equal(luts[ty, tx], np.where(np.arange(256) >= img[ty, tx], 255, 0))
    want = np.zeros((8, 8), np.uint8)
    for y in range(8):
        for x in range(8):
            k = sum(int(img[max(y - dy, 0), max(x - dx, 0)] <= img[y, x]) for dy in (0, 1) for dx in (0, 1))
            want[y, x] = {1: 64, 2: 128, 3: 191, 4: 255}[k]
    assert np.array_equal(R.clahe_plane(img), want)


@pytest.mark.parametrize("shape", [(8, 8), (16, 24), (37, 41), (40, 41), (9, 9)])
def test_clahe_constant_image_stays_constant(shape):
    out = R.clahe_plane(np.full(shape, 100, np.uint8))
    assert (out == out[0, 0]).all()


def test_clahe_lut_is_monotone():
    rs = np.random.RandomState(2)
    img = rs.randint(0, 256, (37, 41)).astype(np.uint8)
    img[5:30, 5:30] = 77
    luts, th, tw = R.clahe_luts(img)
    assert (th, tw) == (5, 6)                                                # 37 -> 40, 41 -> 48
    assert (np.diff(luts.astype(np.int64), axis=-1) >= 0).all() and (luts[..., -1] == 255).all()


def test_clahe_geometry_pads_a_full_eight():
    assert R.clahe_geometry(16, 24)[:4] == (16, 24, 2, 3)
    assert R.clahe_geometry(40, 41)[:4] == (48, 48, 6, 6)                    # 40 divides by 8 and still gains 8 rows
    assert R.clahe_geometry(41, 40)[:4] == (48, 48, 6, 6)
    assert R.clahe_geometry(9, 9)[:4] == (16, 16, 2, 2)
    assert [R.reflect101(p, 9) for p in range(9, 16)] == [7, 6, 5, 4, 3, 2, 1]
    assert [R.reflect101(p, 8) for p in range(8, 16)] == [6, 5, 4, 3, 2, 1, 0, 1]


def test_clahe_16x16_worked_out():
    """16 x 16, columns 0..8 hold 100, columns 9..15 hold 150: tiles of 2 x 2, clip = 1, lutScale = 255 / 4 = 63.75.
      * a tile of four 100s: excess 3, residual 3, step 85 -> one count each in bins {0, 85, 100, 170}: lut[100] = round(3 * 63.75) = 191,
        lut[150] = 191;
      * a tile of four 150s: bins {0, 85, 150, 170}: lut[100] = round(127.5) = 128, lut[150] = 191;
      * tile column 4 (columns 8, 9) holds two 100s and two 150s: excess 2, step 128 -> bins {0, 100, 128, 150}: lut[100] = 128, lut[150] = 255.
    Column 2 t lies half way between tile columns t - 1 and t, column 2 t + 1 on tile column t.  So columns 0..7 give 191; column 8
    (100) = 191 / 2 + 128 / 2 = 159.5 -> 160 (half to even); column 9 (150) = 255; column 10 (150) = 255 / 2 + 191 / 2 = 223; columns
    11..15 give 191.  All rows are alike."""
    img = np.full((16, 16), 100, np.uint8)
    img[:, 9:] = 150
    row = [191] * 8 + [160, 255, 223] + [191] * 5
    assert np.array_equal(R.clahe_plane(img), np.tile(np.array(row, np.uint8), (16, 1)))
    rgb = np.stack([img, img.T, np.full((16, 16), 100, np.uint8)], -1)
    out = R.apply_clahe(rgb)
    assert np.array_equal(out[..., 0], R.clahe_plane(img)) and np.array_equal(out[..., 1], R.clahe_plane(img).T)
    assert (out[..., 2] == 191).all()


# ---- argument checks: no device work -------------------------------------------------------------------------------------------
def test_to_image_argument_checks():
    pytest.importorskip("torch")
    from obia_amd.image import Image, to_image
    raster = np.zeros((10, 12, 5), np.float32)
    for bands in ([0, 1], (0, 1, 2, 3), "012", None):
        with pytest.raises(ValueError, match="'bands' should be a list or tuple of exactly three elements"):
            to_image(raster, bands)
    with pytest.raises(IndexError, match=r"Band index 5 out of range. Available bands indices: 0 to 4\."):
        to_image(raster, [0, 5, 1])
    with pytest.raises(IndexError, match=r"Band index -1 out of range. Available bands indices: 0 to 4\."):
        Image(raster).to_image((0, 1, -1))
    with pytest.raises(ValueError, match="Unknown stretch_type: linear"):
        Image(raster, crs="EPSG:32610").to_image([0, 1, 2], stretch_type="linear")
    with pytest.raises(ValueError, match="8 x 8"):
        to_image(np.zeros((7, 20, 3), np.float32), [0, 1, 2], stretch_type="clahe")
    holder = Image(raster, "EPSG:4326", [1, 0, 0, -1, 0, 0], "t", "r")
    assert (holder.crs, holder.affine_transformation, holder.transform, holder.rasterio_obj) == ("EPSG:4326", [1, 0, 0, -1, 0, 0], "t", "r")


def test_stretch_argument_checks():
    pytest.importorskip("torch")
    from obia_amd import image as I
    with pytest.raises(TypeError, match="int32"):
        I.rescale_to_8bit(np.zeros((3, 3), np.int32))
    with pytest.raises(TypeError, match="float32"):
        I.apply_histogram_equalization(np.zeros((9, 9), np.float32))
    with pytest.raises(TypeError, match="uint16"):
        I.apply_clahe(np.zeros((9, 9), np.uint16))
    with pytest.raises(ValueError, match="8 x 8"):
        I.apply_clahe(np.zeros((7, 20), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        I.apply_clahe(np.zeros((9, 9, 4), np.uint8))
    with pytest.raises(NotImplementedError, match="outer"):
        I.find_boundaries(np.zeros((4, 4), np.int32), mode="inner")
    with pytest.raises(NotImplementedError, match="background"):
        I.find_boundaries(np.zeros((4, 4), np.int32), background=1)
    with pytest.raises(ValueError, match="color"):
        I.mark_boundaries_u8(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.int32), color=(1.0, 300, 0))


def test_to_segmented_image_argument_checks():
    pytest.importorskip("torch")
    PIL = pytest.importorskip("PIL.Image")
    from obia_amd.segmentation import Segments
    seg = Segments(np.ones((6, 9), np.int32), None, "slic")
    with pytest.raises(TypeError, match="Input must be a PIL Image"):
        seg.to_segmented_image(np.zeros((6, 9, 3), np.uint8))
    with pytest.raises(ValueError, match="6 x 9"):
        seg.to_segmented_image(PIL.fromarray(np.zeros((9, 6, 3), np.uint8)))
    with pytest.raises(ValueError, match="mode 'F'"):
        seg.to_segmented_image(PIL.fromarray(np.zeros((6, 9), np.float32)))
    with pytest.raises(ValueError, match="mode 'RGBA'"):
        seg.to_segmented_image(PIL.fromarray(np.zeros((6, 9, 4), np.uint8)))
