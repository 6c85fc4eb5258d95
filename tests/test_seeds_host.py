"""Seeds, host side: the checks of obia_amd.seeds that fire before any device work, the new entry points in the binding
table, and the point layers of obia_amd.geopackage."""
import numpy as np
import pytest

from tests import seeds_restatement as R


def _seeds(n=3, col="ch_max"):
    return {"x": np.arange(n, dtype=np.float64), "y": np.zeros(n), col: np.full(n, 5, np.float32)}


@pytest.fixture()
def no_device(monkeypatch):
    """Any use of the library fails the test."""
    from obia_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device library was used")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "default_context", boom)


def test_public_names():
    import obia_amd
    from obia_amd import seeds
    for name in ("make_chm_seeds", "make_density_seeds", "make_canonical_seeds"):
        assert getattr(obia_amd, name) is getattr(seeds, name)


def test_new_symbols_are_in_the_binding_table():
    from obia_amd import _lib
    for s in ("obia_seeds_peaks_dev", "obia_seeds_peaks_gather_dev", "obia_seeds_pair_link_dev", "obia_seeds_pair_stats_dev",
              "obia_seeds_pair_matrix_dev"):
        assert s in _lib.EXPORTED_SYMBOLS


@pytest.mark.parametrize("kw,name", [(dict(keep_all_stage1=False), "keep_all_stage1"), (dict(z_thresh=0), "z_thresh"),
                                     (dict(z_thresh=2.5), "z_thresh"), (dict(dz_merge=1.0), "dz_merge"),
                                     (dict(max_per_cluster=2), "max_per_cluster"), (dict(nms_base=1.0), "nms_base"),
                                     (dict(nms_scale=0.1), "nms_scale")])
def test_table_options_raise_before_device_use(no_device, kw, name):
    from obia_amd.seeds import make_canonical_seeds
    with pytest.raises(NotImplementedError, match=name):
        make_canonical_seeds(_seeds(), _seeds(col="den_max"), np.zeros((4, 4), np.float32), **kw)


def test_seeds_without_heights_raise_before_device_use(no_device):
    from obia_amd.seeds import make_canonical_seeds
    bare = {"x": np.zeros(2), "y": np.zeros(2)}
    with pytest.raises(NotImplementedError, match="_add_chm_height"):
        make_canonical_seeds(bare, _seeds(col="den_max"), np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="dict with x and y"):
        make_canonical_seeds([1, 2, 3], _seeds(col="den_max"), np.zeros((4, 4), np.float32))


def test_canonical_argument_checks(no_device):
    from obia_amd.seeds import make_canonical_seeds
    with pytest.raises(ValueError, match="cost_surface must be"):
        make_canonical_seeds(_seeds(), _seeds(col="den_max"), np.zeros((4, 4, 2), np.float32))
    with pytest.raises(ValueError, match="singular"):
        make_canonical_seeds(_seeds(), _seeds(col="den_max"), np.zeros((4, 4), np.float32), cost_affine=[1, 1, 1, 1, 0, 0])


@pytest.mark.parametrize("fn", ["make_chm_seeds", "make_density_seeds"])
def test_peak_argument_checks(no_device, fn):
    from obia_amd import seeds
    f = getattr(seeds, fn)
    with pytest.raises(ValueError, match=r"must be \(H, W\)"):
        f(np.zeros((4, 4, 2), np.float32))
    with pytest.raises(ValueError, match="is empty"):
        f(np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError, match="min_dist_px"):
        f(np.zeros((4, 4), np.float32), min_dist_px=-1)
    with pytest.raises(ValueError, match="min_dist_px"):
        f(np.zeros((4, 4), np.float32), min_dist_px=33)
    with pytest.raises(ValueError, match="min_dist_px"):
        f(np.zeros((4, 4), np.float32), min_dist_px=2.5)
    with pytest.raises(ValueError, match="gauss_sigma"):
        f(np.zeros((4, 4), np.float32), gauss_sigma=-1)


def test_pair_argument_checks(no_device):
    from obia_amd import seeds
    cost = np.zeros((4, 4), np.float32)
    inv = [1, 0, 0, 0, 1, 0]
    with pytest.raises(ValueError, match="1-D"):
        seeds.merge_clusters(np.zeros(3), np.zeros(4), cost, inv, 0.5, 0.8, 1.5)
    with pytest.raises(ValueError, match="no seeds"):
        seeds.merge_clusters(np.zeros(0), np.zeros(0), cost, inv, 0.5, 0.8, 1.5)
    with pytest.raises(ValueError, match="cost must be"):
        seeds.pair_distances(np.zeros(3), np.zeros(3), np.zeros(4, np.float32), inv, 0.5, 0.8)
    with pytest.raises(ValueError, match="six values"):
        seeds.pair_stats(np.zeros(3), np.zeros(3), cost, inv[:5], 0.5, 0.8)
    with pytest.raises(ValueError, match="zero-size"):
        seeds.pair_stats(np.zeros(1), np.zeros(1), cost, inv, 0.5, 0.8)


def test_line_samples_and_inverse_match_the_restatement():
    from obia_amd import seeds
    for s in (1, 8, 12, 128):
        assert np.array_equal(seeds.line_samples(s), R.line_ts(s).astype(np.float64))
    for aff in (R.pixel_affine(0.5, 77), [0.3, 0.01, -0.02, -0.3, 431000.7, 5012345.1]):
        assert seeds.invert_affine(aff) == R.inverse6(aff)


def test_seed_points_round_trip_through_a_geopackage(tmp_path):
    from obia_amd import seeds
    from obia_amd.geopackage import read_geopackage
    tab = {"id": np.arange(4), "row": np.arange(4, dtype=np.int32), "col": np.arange(4, dtype=np.int32),
           "x": np.array([0.5, 1.25, -3.0, 1e6 + 0.1]), "y": np.array([2.0, -1.5, 0.0, 7.75]),
           "ch_max": np.array([3.5, 2.5, np.nan, 9.0], np.float32), "origin": np.array(["chm", "chm", "density", "density"])}
    p = tmp_path / "sub" / "chm_seeds.gpkg"
    seeds.write_seed_points(p, tab)
    wkbs, cols, srs = read_geopackage(str(p), table="chm_seeds")
    assert srs == -1 and len(wkbs) == 4 and cols["origin"] == ["chm", "chm", "density", "density"]
    back = seeds.read_seed_points(p)
    assert np.array_equal(back["x"], tab["x"]) and np.array_equal(back["y"], tab["y"])
    assert list(back["id"]) == [0, 1, 2, 3] and back["ch_max"][1] == 2.5 and back["ch_max"][2] is None
    assert "row" not in back
