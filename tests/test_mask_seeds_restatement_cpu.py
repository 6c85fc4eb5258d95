"""The NumPy restatement of scikit-image's maskSLIC seeding (tests/mask_seeds_restatement.py) against what scikit-image 0.18.3 itself
returned (the fixtures' `seeds_yx` / `seed_steps_all`) and against the local SciPy, bit for bit; and what the host side of
``seeding="skimage"`` refuses before it touches a device.  No GPU."""
import ast
import os
import re
import warnings

import numpy as np
import pytest

from tests import mask_seeds_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, ast.literal_eval(str(z["params"]))["n_segments"]


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_equals_the_fixtures_bit_for_bit(name):
    z, n = fixture(name)
    cent, steps = R.mask_centroids(z["mask"], n)
    assert cent.dtype == np.float64 and cent.shape == (len(z["seeds_yx"]), 3) and not cent[:, 0].any()
    assert np.array_equal(cent[:, 1:], z["seeds_yx"]), f"{name}: centroids"
    assert np.array_equal(steps, z["seed_steps_all"]), f"{name}: steps"


@pytest.mark.parametrize("name", R.FIXTURES)
def test_steps_are_a_row_by_row_sum(name):
    """``abs(...).mean(0)`` on a C-ordered (K, 3) array: one running sum per column in row order, then one division -- the order the
    library's host loop uses."""
    z, n = fixture(name)
    cent, _ = R.mask_centroids(z["mask"], n)
    acc = np.zeros(3)
    for a, b in zip(cent, cent[R.closest_other(cent)]):
        acc = acc + np.abs(a - b)
    assert np.array_equal(acc / len(cent), z["seed_steps_all"])


def scipy_centroids(mask, n):
    """The routine's own calls on the local SciPy: kmeans2 on the picked points, pdist + argmin."""
    from scipy.cluster.vq import kmeans2
    from scipy.spatial.distance import pdist, squareform
    yy, xx = np.nonzero(mask)
    coord = np.stack([np.zeros(len(yy)), yy, xx], 1).astype(np.float64)
    idx, dense = R.picks(len(coord), n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # (an empty cluster: kmeans2 warns and keeps the centroid)
        cent, _ = kmeans2(coord if dense is None else coord[dense], coord[idx], iter=5)
    dist = squareform(pdist(cent))
    np.fill_diagonal(dist, np.inf)
    return cent, dist.argmin(-1)


@pytest.mark.parametrize("name", R.FIXTURES + tuple(c for c in R.EDGE_CASES if c != "blob_k1000"))
def test_restatement_equals_scipy(name):
    pytest.importorskip("scipy")
    if name in R.FIXTURES:
        z, n = fixture(name)
        mask = z["mask"]
    else:
        mask, n = R.edge_case(name)
    want, closest = scipy_centroids(mask, n)
    got, steps = R.mask_centroids(mask, n)
    assert np.array_equal(got, want), f"{name}: k-means"
    assert np.array_equal(R.closest_other(got), closest), f"{name}: nearest other centroid"
    assert np.array_equal(steps, np.abs(want - want[closest]).mean(0)), f"{name}: steps"


def test_edge_cases_are_what_they_claim():
    info = {n: {} for n in R.EDGE_CASES if n != "blob_k1000"}
    for n, i in info.items():
        R.mask_centroids(*R.edge_case(n), info=i)
    assert info["no_dense_draw"]["n_dense"] is None and info["no_dense_draw"]["n_valid"] <= 100 * 30
    assert info["n_above_n_valid"]["K"] == info["n_above_n_valid"]["n_valid"] == 7 < R.edge_case("n_above_n_valid")[1]
    assert sum(info["empty_cluster"]["empty_per_iter"]) > 0
    assert info["ties"]["ties_first_iter"] > 0 and info["ties"]["n_dense"] == 1600
    assert info["chunk_plus_one"]["K"] == 1025 and info["two"]["K"] == 2
    assert np.flatnonzero(R.edge_case("single_row")[0].any(1)).tolist() == [4]


def test_library_draws_the_same_picks():
    from obia_amd.segmentation import _mask_seed_picks
    for n_valid, n in [(9065, 60), (7, 20), (6001, 60), (6000, 60), (107465, 1000)]:
        a, b = _mask_seed_picks(n_valid, n), R.picks(n_valid, n)
        assert a[0].dtype == np.int64 and np.array_equal(a[0], b[0])
        assert (a[1] is None) == (b[1] is None) == (n_valid <= 100 * n)
        if b[1] is not None:
            assert a[1].dtype == np.int64 and np.array_equal(a[1], b[1]) and len(b[1]) == 100 * n


def test_chunk_constant_matches_the_header():
    from obia_amd import _lib
    txt = open(os.path.join(ROOT, "include", "obia_hip.h")).read()
    assert int(re.search(r"#define OBIA_MASK_SEEDS_CHUNK (\d+)", txt).group(1)) == _lib.MASK_SEEDS_CHUNK


def test_host_side_refusals():
    """Everything the Python layer refuses before a device is touched."""
    from obia_amd.segmentation import create_segments, mask_centroids, segment, slic
    img = np.random.RandomState(0).rand(12, 14, 3).astype(np.float32)
    mask = np.ones((12, 14), bool)
    one = np.zeros((12, 14), bool)
    one[3, 4] = True
    seeds = (np.array([[2.0, 2.0], [8.0, 9.0]]), (1.0, 6.0, 7.0))
    with pytest.raises(ValueError, match="needs a mask"):
        slic(img, n_segments=4, seeding="skimage")
    with pytest.raises(ValueError, match="seeds="):
        slic(img, n_segments=4, mask=mask, seeds=seeds, seeding="skimage")
    with pytest.raises(ValueError, match="n_segments >= 2"):
        slic(img, n_segments=1, mask=mask, seeding="skimage")
    with pytest.raises(ValueError, match="two valid pixels"):
        slic(img, n_segments=4, mask=one, seeding="skimage")
    with pytest.raises(ValueError, match="two valid pixels"):
        slic(img, n_segments=4, mask=np.zeros((12, 14), bool), seeding="skimage")
    with pytest.raises(ValueError, match="same shape"):
        slic(img, n_segments=4, mask=np.ones((12, 13), bool), seeding="skimage")
    with pytest.raises(ValueError, match='"grid" or "skimage"'):
        slic(img, n_segments=4, mask=mask, seeding="kmeans")
    with pytest.raises(ValueError, match="two valid pixels"):
        mask_centroids(one, 4)
    with pytest.raises(ValueError, match="at least 2"):
        mask_centroids(mask, 1)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        mask_centroids(np.ones((2, 3, 4), bool), 4)
    # the same keyword one and two layers up
    with pytest.raises(ValueError, match="needs a mask"):
        create_segments(img, seeding="skimage", n_segments=4)
    with pytest.raises(ValueError, match="quickshift has no seeds"):
        create_segments(img, method="quickshift", seeding="skimage")
    with pytest.raises(ValueError, match='"grid" or "skimage"'):
        create_segments(img, seeding="random")
    with pytest.raises(ValueError, match="needs a mask"):
        segment(img, seeding="skimage", n_segments=4)
