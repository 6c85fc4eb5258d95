"""The sharpness raster, host side: the NumPy restatement (tests/sharpness_restatement.py) against the committed SciPy 1.15.3 goldens
of the box filter (and against SciPy itself where it is installed), the Laplacian against answers worked out by hand, the grey
expression and the stretch against the reference's NumPy lines; the argument checks of obia_amd.image.rgb_to_gray / box_filter /
variance_of_laplacian / laplacian that fire before any device work.

The Laplacian is cv2.Laplacian(gray, CV_32F, ksize=3) restated from OpenCV's algorithm and is NOT compared with cv2 anywhere."""
import glob
import hashlib
import os

import numpy as np
import pytest

from tests import sharpness_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "sharpness", "*.npz")))


def golden_cases(path):
    """(plane, [(win, expected float32 plane or None, sha256 of its bytes)]) of one golden file"""
    g = np.load(path)
    data, shp = os.path.basename(path)[:-4].split("_")
    shape = tuple(int(v) for v in shp.split("x"))
    plane = g["plane"] if "plane" in g else S.golden_plane(data, shape)
    assert plane.dtype == np.float32 and plane.shape == shape
    assert hashlib.sha256(plane.tobytes()).hexdigest() == str(g["sha_plane"])
    cases = []
    for w in g["wins"]:
        key = f"out_{int(w)}"
        want = g[key] if key in g else None
        cases.append((int(w), want, hashlib.sha256(want.tobytes()).hexdigest() if want is not None else str(g[f"sha_{int(w)}"])))
    return plane, cases


# ---- the box filter against SciPy ------------------------------------------------------------------------------------------------
def test_goldens_are_there():
    assert len(GOLDENS) == 13
    assert all(os.path.getsize(p) < 160 * 1024 for p in GOLDENS)
    assert all(str(np.load(p)["scipy_version"]) == "1.15.3" for p in GOLDENS)


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_restatement_box_filter_is_scipy_bit_for_bit(path):
    plane, cases = golden_cases(path)
    for win, want, digest in cases:
        got = S.box_filter(plane, win)
        assert got.dtype == np.float32
        assert hashlib.sha256(got.tobytes()).hexdigest() == digest, (os.path.basename(path), win)
        if want is not None:
            assert np.array_equal(S.bits(got), S.bits(want))


def test_goldens_cover_windows_longer_than_twice_the_line():
    seen = set()
    for p in GOLDENS:
        plane, cases = golden_cases(p)
        seen |= {(plane.shape, w) for w, _, _ in cases if w > 2 * max(plane.shape)}
    assert ((9, 4), 30) in seen and ((67, 130), 300) in seen


@pytest.mark.parametrize("shape,win", [((67, 130), 3), ((67, 130), 4), ((130, 517), 15), ((5, 3), 40), ((1, 7), 2)])
def test_restatement_box_filter_is_scipy_itself(shape, win):
    ndi = pytest.importorskip("scipy.ndimage")
    for data in ("n50", "wide"):
        plane = S.golden_plane(data, shape)
        assert np.array_equal(S.bits(S.box_filter(plane, win)), S.bits(ndi.uniform_filter(plane, size=win)))


def test_the_wide_plane_tells_the_serial_sum_from_a_direct_one():
    """what the wide-range goldens are for: summing each window on its own (in double, both axes) is NOT SciPy's result"""
    plane = np.load(os.path.join(ROOT, "tests", "golden", "sharpness", "wide_67x130.npz"))

    def direct(p, win, axis):
        x = np.moveaxis(p, axis, 0).astype(np.float64)
        n, s1 = x.shape[0], win // 2
        out = np.empty(x.shape, np.float32)
        for i in range(n):
            t = np.zeros(x.shape[1:])
            for l in range(-s1, win - s1):
                t = t + x[S.reflect_sym(i + l, n)]
            out[i] = (t / win).astype(np.float32)
        return np.moveaxis(out, 0, axis)

    for win in (3, 4):
        d = direct(direct(plane["plane"], win, 0), win, 1)
        assert int((S.bits(d) != S.bits(plane[f"out_{win}"])).sum()) > 30
    n50 = S.golden_plane("n50", (33, 17))                                    # exact double sums: every order agrees
    assert np.array_equal(S.bits(direct(direct(n50, 3, 0), 3, 1)), S.bits(S.box_filter(n50, 3)))


# ---- the Laplacian by hand -------------------------------------------------------------------------------------------------------
def test_laplacian_of_an_impulse():
    g = np.zeros((5, 7), np.float32)
    g[2, 3] = 1
    want = np.zeros((5, 7), np.float32)
    want[2, 3] = -8
    want[1, 2] = want[1, 4] = want[3, 2] = want[3, 4] = 2                    # the four diagonal neighbours see it once
    assert np.array_equal(S.laplacian3(g), want)
    corner = np.zeros((4, 4), np.float32)
    corner[0, 0] = 1                                                        # REFLECT_101 never reads the corner back: only (1, 1) sees it
    want = np.zeros((4, 4), np.float32)
    want[0, 0], want[1, 1] = -8, 2
    assert np.array_equal(S.laplacian3(corner), want)
    edge = np.zeros((4, 4), np.float32)
    edge[1, 1] = 1                                                          # (0, 0) reads (1, 1) at all four diagonals: row -1 -> 1, column -1 -> 1
    want = np.zeros((4, 4), np.float32)
    want[1, 1] = -8
    want[0, 0] = 8
    want[0, 2] = want[2, 0] = 4                                             # twice: through the reflected row (column) and the real one
    want[2, 2] = 2
    assert np.array_equal(S.laplacian3(edge), want)


def test_laplacian_of_a_ramp():
    """g = x: inside 2 (x - 1) + 2 (x + 1) - 8 x + 2 (x - 1) + 2 (x + 1) = 0; column 0 reads column 1 on both sides: 8; the last
    column reads W - 2 on both sides: -8.  A ramp down the rows likewise."""
    W = 9
    g = np.tile(np.arange(W, dtype=np.float32), (6, 1))
    want = np.zeros((6, W), np.float32)
    want[:, 0], want[:, -1] = 8, -8
    assert np.array_equal(S.laplacian3(g), want)
    assert np.array_equal(S.laplacian3(g.T.copy()), want.T)


def test_laplacian_of_a_line_and_of_2x2():
    """1 x n: both neighbour rows are the row itself, so lap[x] = 4 g[x - 1] + 4 g[x + 1] - 8 g[x] with REFLECT_101 at the ends;
    1 x 1: 8 g - 8 g = 0; 2 x 2: every diagonal of a pixel is the opposite corner: 8 (opposite - own)."""
    g = np.array([[1, 4, 9, 16, 25]], np.float32)
    want = np.array([[8 * 4 - 8 * 1, 4 * 1 + 4 * 9 - 32, 4 * 4 + 4 * 16 - 72, 4 * 9 + 4 * 25 - 128, 8 * 16 - 200]], np.float32)
    assert np.array_equal(S.laplacian3(g), want)
    assert np.array_equal(S.laplacian3(g.T.copy()), want.T)
    assert np.array_equal(S.laplacian3(np.array([[3.5]], np.float32)), np.zeros((1, 1), np.float32))
    q = np.array([[1, 2], [5, 11]], np.float32)
    assert np.array_equal(S.laplacian3(q), np.array([[80, 24], [-24, -80]], np.float32))


def test_laplacian_sums_in_opencv_order():
    """((((2a + 2b) + (-8c)) + 2d) + 2e) in float32: with a = 2^24 and e = -2^24 the small taps are lost on the way"""
    g = np.zeros((3, 3), np.float32)
    g[0, 0], g[0, 2], g[1, 1], g[2, 0], g[2, 2] = 2.0 ** 24, 0.5, 0.0, 0.25, -2.0 ** 24
    f = np.float32
    want = (((f(2) * f(2.0 ** 24) + f(2) * f(0.5)) + f(-8) * f(0)) + f(2) * f(0.25)) + f(2) * f(-2.0 ** 24)
    assert S.laplacian3(g)[1, 1] == want == 0.0                              # exact arithmetic would give 1.5


# ---- grey, normalisation, stretch: the reference's lines ----------------------------------------------------------------------------
def test_gray_is_the_numpy_expression():
    rs = np.random.RandomState(4)
    for rgb in (rs.rand(13, 29, 3).astype(np.float32), (rs.standard_normal((7, 5, 3)) * 1e4).astype(np.float32)):
        coeffs = np.array([0.299, 0.587, 0.114], dtype=np.float32)           # obia/utils/image.py:99-100, literally
        want = (rgb * coeffs).sum(axis=-1)
        assert want.dtype == np.float32 and np.array_equal(S.bits(S.rgb_to_gray(rgb)), S.bits(want))


def test_normalisation_is_the_reference_lines():
    rs = np.random.RandomState(6)
    arr = rs.randint(0, 4000, (3, 11, 9)).astype(np.uint16).astype(np.float32)       # bands first, as src.read gives them
    arr[1] = 77                                                                        # a constant band
    band_min = arr.min(axis=(1, 2), keepdims=True)                                     # image.py:120-122
    band_rng = np.ptp(arr, axis=(1, 2), keepdims=True) + 1e-8
    want = np.transpose((arr - band_min) / band_rng, (1, 2, 0))
    got = S.normalise_bands(np.transpose(arr, (1, 2, 0)))
    assert want.dtype == np.float32 and np.array_equal(S.bits(got), S.bits(want))
    assert not got[..., 1].any() and got.min() == 0 and got.max() <= 1


def test_stretch_is_the_reference_lines():
    rs = np.random.RandomState(8)
    sharp = (rs.standard_normal((17, 23)) ** 2).astype(np.float32)
    lo, hi = np.percentile(sharp, [2, 98])                                   # image.py:130-131, :136
    want = np.clip((sharp - lo) / (hi - lo), 0, 1).astype("float32")
    assert np.asarray(lo).dtype == np.float64 and np.array_equal(S.bits(S.stretch(sharp)), S.bits(want))
    flat = np.full((4, 5), 2.5, np.float32)                                  # hi == lo: 0 / 0
    assert np.isnan(S.stretch(flat)).all()
    step = np.full((10, 10), 1.0, np.float32)                                # 2nd and 98th percentile both 1: below 0, above 1, NaN at 1
    step[0, 0], step[9, 9] = 0.0, 3.0
    out = S.stretch(step)
    assert out[0, 0] == 0 and out[9, 9] == 1 and np.isnan(out[5, 5]) and int(np.isnan(out).sum()) == 98


def test_restatement_laplacian_end_to_end_shapes():
    rs = np.random.RandomState(9)
    img = rs.rand(12, 15, 5).astype(np.float32)
    out = S.laplacian(img, 3)
    assert out.dtype == np.float32 and out.shape == (12, 15) and out.min() == 0 and out.max() == 1
    assert np.isnan(S.laplacian(np.ones((6, 6, 5), np.float32), 3)).all()    # a constant raster: the literal all-NaN result


# ---- argument checks: no device work -------------------------------------------------------------------------------------------
def test_laplacian_argument_checks(tmp_path):
    pytest.importorskip("torch")
    from obia_amd.image import Image, laplacian
    raster = np.zeros((10, 12, 5), np.float32)
    with pytest.raises(NotImplementedError, match="GeoTIFF I/O stays with the caller"):
        laplacian(raster, str(tmp_path / "sharp.tif"), 3)
    with pytest.raises(NotImplementedError, match="GeoTIFF I/O stays with the caller"):
        laplacian("scene.tif", None, 3)
    with pytest.raises(NotImplementedError, match="GeoTIFF I/O stays with the caller"):
        laplacian(tmp_path / "scene.tif", None, 3)
    for win in (0, -3, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="win must be an integer >= 1"):
            laplacian(raster, None, win)
    with pytest.raises(ValueError, match="'bands' should be a list or tuple of exactly three elements"):
        laplacian(raster, None, 3, bands=[0, 1])
    with pytest.raises(IndexError, match=r"Band index 5 out of range. Available bands indices: 0 to 4\."):
        laplacian(raster, None, 3, bands=(0, 5, 1))
    with pytest.raises(IndexError, match=r"Band index 4 out of range. Available bands indices: 0 to 3\."):
        laplacian(np.zeros((10, 12, 4), np.float32), None, 3)                # the default bands need five
    with pytest.raises(IndexError, match=r"Band index -1 out of range"):
        Image(raster).laplacian(3, bands=(0, 1, -1))
    with pytest.raises(ValueError, match="shape"):
        laplacian(np.zeros((10, 12), np.float32), None, 3)
    with pytest.raises(ValueError, match="empty"):
        laplacian(np.zeros((0, 12, 5), np.float32), None, 3)
    with pytest.raises(TypeError, match="int32"):
        laplacian(np.zeros((10, 12, 5), np.int32), None, 3)
    with pytest.raises(NotImplementedError, match="GeoTIFF"):
        Image(raster).laplacian(3, "out.tif")


def test_lower_functions_argument_checks():
    pytest.importorskip("torch")
    from obia_amd import image as I
    plane = np.zeros((6, 7), np.float32)
    for fn in (I.box_filter, I.variance_of_laplacian):
        for win in (0, -1, 1.5, "2", None, False):
            with pytest.raises(ValueError, match="win must be an integer >= 1"):
                fn(plane, win)
        for bad in (np.zeros((6, 7, 3), np.float32), np.zeros(6, np.float32), np.zeros((0, 7), np.float32), np.zeros((6, 0), np.float32)):
            with pytest.raises(ValueError, match="shape"):
                fn(bad, 3)
        with pytest.raises(TypeError, match="int64"):
            fn(np.zeros((6, 7), np.int64), 3)
        with pytest.raises(NotImplementedError, match="larger than 65536"):
            fn(plane, 65537)
    for bad in (plane, np.zeros((6, 7, 4), np.float32), np.zeros((6, 7, 3, 1), np.float32)):
        with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
            I.rgb_to_gray(bad)
    with pytest.raises(TypeError, match="int32"):
        I.rgb_to_gray(np.zeros((6, 7, 3), np.int32))
