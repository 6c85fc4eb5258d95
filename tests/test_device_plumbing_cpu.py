"""The wrappers' device plumbing without a device (obia_amd/_device.py): a CPU tensor in any array argument of any public wrapper is
refused before the library is loaded or a context made, ``device_of`` makes no context, and the band-list and label-count helpers of
statistics.py and the torch-free NumPy path of ``zonal_stats`` do what the three copies they replace did."""
from importlib import import_module

import numpy as np
import pytest

torch = pytest.importorskip("torch")

K, U, T, P, S, G, Z, L = (import_module("obia_amd." + m) for m in ("classify", "consumers", "cost", "polygons", "seeds", "segmentation",
                                                                    "statistics", "tiling"))
from obia_amd import _device, _lib  # noqa: E402

AFF = [0.5, 0.0, 0.0, -0.5, 100.0, 200.0]
INV = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "default_context", boom)


def _forest():
    return K.Forest(threshold=[0.5, 0, 0], feature=[0, -2, -2], left=[1, -1, -1], right=[2, -1, -1], missing_go_to_left=[0, 0, 0], tree_offset=[0],
                    value=[[0.5, 0.5], [1, 0], [0, 1]], classes_=[0, 1], n_features=2, cover=[3, 1, 2])


def _mlp():
    return K.MLP(np.zeros(12), np.zeros(5), [2, 3, 2], "relu", "softmax", [0, 1])


def _calls():
    """(wrapper, call(*arrays), the array arguments): every argument that may be a tensor, valid otherwise, so that only the CPU
    tensor put in one position at a time can be what is refused"""
    f, m = _forest(), _mlp()
    img, rgb, plane = np.ones((4, 5, 2), np.float32), np.ones((4, 5, 3), np.float32), np.ones((4, 5), np.float32)
    lab, mask = np.arange(20, dtype=np.int32).reshape(4, 5) // 5 + 1, np.ones((4, 5), np.uint8)
    X, acc, masks = np.zeros((3, 2)), np.ones((3, 2), bool), np.array([[False, False], [True, False], [False, True], [True, True]])
    xs, pts = np.array([1.0, 2.0, 3.0]), np.array([[100.5, 199.5]])
    seeds = ({"x": xs, "y": xs, "ch_max": xs.astype(np.float32)}, {"x": xs, "y": xs, "den_max": xs.astype(np.float32)})
    table = K.ClassifiedImage({"predicted_class": np.arange(4)}, None, None, None, None, None, {})
    pair = (INV, 0.5, 0.8)
    return [
        ("standard_scale", lambda t: K.standard_scale(t), [X]),
        ("forest_predict", lambda x, a: K.forest_predict(f, x, acceptable=a), [X.astype(np.float32), acc]),
        ("forest_shap", lambda x: K.forest_shap(f, x), [X.astype(np.float32)]),
        ("mlp_predict", lambda x, a: K.mlp_predict(m, x, acceptable=a), [X, acc]),
        ("mlp_coalition_values", lambda x, b, k: K.mlp_coalition_values(m, x, b, k), [X, X[:2], masks]),
        ("shapley_combine", lambda v: K.shapley_combine(v), [np.zeros((3, 4, 2))]),
        ("mlp_shap", lambda x, b: K.mlp_shap(m, x, b), [X, X[:2]]),
        ("to_raster", lambda x: table.to_raster(x), [lab]),
        ("zonal_stats", lambda r, x: Z.zonal_stats(r, x), [img, lab]),
        ("texture_stats", lambda r, x: Z.texture_stats(r, x), [img, lab]),
        ("slic_edge", lambda x: U.slic_edge(x), [lab]),
        ("sample_labels", lambda x: U.sample_labels(x, AFF, pts), [lab]),
        ("label_segments", lambda x: U.label_segments(x, AFF, pts, [1]), [lab]),
        ("polygonize", lambda x: P.polygonize(x), [lab]),
        ("slic", lambda r, k: G.slic(r, n_segments=4, mask=k), [img, mask]),
        ("slic_skimage", lambda r, k: G.slic(r, n_segments=4, mask=k, seeding="skimage"), [img, mask]),
        ("quickshift", lambda r: G.quickshift(r), [rgb]),
        ("mask_centroids", lambda k: G.mask_centroids(k, 4), [mask]),
        ("create_segments", lambda r: G.create_segments(r, n_segments=4), [img]),
        ("create_tiled_segments", lambda r, k: L.create_tiled_segments(r, input_mask=k), [img, mask]),
        ("normalise", lambda x: T.normalise(x), [plane]),
        ("chm_gradient", lambda x: T.chm_gradient(x), [plane]),
        ("ndvi", lambda r, n: T.ndvi(r, n), [plane, plane]),
        ("texture_entropy", lambda x: T.texture_entropy(x), [plane]),
        ("make_cost_surface", lambda w, c, s: T.make_cost_surface(w, c, slic=s, weights=(0.4, 0.3, 0.2, 0.1)), [np.ones((4, 5, 8), np.float32), plane, lab]),
        ("detect_peaks", lambda x: S.detect_peaks(x, 0.5, 1), [plane]),
        ("make_chm_seeds", lambda x: S.make_chm_seeds(x), [plane]),
        ("make_density_seeds", lambda x: S.make_density_seeds(x), [plane]),
        ("pair_distances", lambda x, y, c: S.pair_distances(x, y, c, *pair), [xs, xs, plane]),
        ("merge_clusters", lambda x, y, c: S.merge_clusters(x, y, c, *pair, 1.5), [xs, xs, plane]),
        ("pair_stats", lambda x, y, c: S.pair_stats(x, y, c, *pair), [xs, xs, plane]),
        ("make_canonical_seeds", lambda c: S.make_canonical_seeds(*seeds, c, debug_dist=False), [plane]),
    ]


CONVERTED = ("standard_scale forest_predict forest_shap mlp_predict mlp_coalition_values shapley_combine mlp_shap to_raster zonal_stats "
             "texture_stats slic_edge sample_labels label_segments polygonize slic quickshift mask_centroids create_tiled_segments normalise "
             "chm_gradient ndvi texture_entropy make_cost_surface detect_peaks make_chm_seeds make_density_seeds pair_distances merge_clusters "
             "pair_stats make_canonical_seeds").split()


def test_the_list_names_every_converted_wrapper():
    names = [c[0] for c in _calls()]
    assert names and set(CONVERTED) <= set(names)
    assert "sample_labels" in names and "label_segments" in names


@pytest.mark.parametrize("name", [c[0] for c in _calls()])
def test_a_cpu_tensor_is_refused_before_the_library_is_touched(no_device, name):
    _, call, arrays = next(c for c in _calls() if c[0] == name)
    for i in range(len(arrays)):
        args = [torch.as_tensor(a) if j == i else a for j, a in enumerate(arrays)]
        with pytest.raises(ValueError, match="must live on the GPU"):
            call(*args)


def test_the_two_wrappers_with_a_refusal_of_their_own(no_device):
    """rasterize takes its three ring arrays all as NumPy or all as CUDA tensors; enforce_connectivity takes a CUDA tensor only"""
    xy, off, shape = np.array([[0.0, 0], [3, 0], [3, 3], [0, 0]]), np.array([0, 4]), np.array([0])
    for i in range(3):
        rings = tuple(torch.as_tensor(a) if j == i else a for j, a in enumerate((xy, off, shape)))
        with pytest.raises(ValueError, match="all NumPy arrays or all CUDA tensors"):
            P.rasterize(rings, (4, 4))
    for labels in (torch.zeros((4, 4), dtype=torch.int32), np.zeros((4, 4), np.int32)):
        with pytest.raises(ValueError, match="needs an int32 CUDA tensor"):
            G.enforce_connectivity(labels, 1, 9)


def test_device_of_makes_no_context(no_device):
    class Ctx:
        device = 3
    a = np.zeros(3)
    assert _device.device_of(Ctx(), a) == 3 and _device.device_of(Ctx(), a, None, [1, 2]) == 3
    assert _device.device_of(None, a) == 0 and _device.device_of(None) == 0
    with pytest.raises(ValueError, match="must live on the GPU$"):
        _device.device_of(Ctx(), a, torch.zeros(2))
    with pytest.raises(ValueError, match="must live on the GPU; pass a NumPy array for host data$"):
        _device.device_of(None, torch.zeros(2), hint="; pass a NumPy array for host data")


def test_band_list():
    want = [2, 0, 1]
    for bands in (want, tuple(want), np.array(want), np.array(want, np.int64), np.array(want, np.uint8)):
        got = Z._band_list(bands, 3)
        assert got == want and all(type(b) is int for b in got)
    assert Z._band_list(None, 4) == [0, 1, 2, 3] and Z._band_list([], 4) == []
    for bad in (3, -1):
        with pytest.raises(IndexError, match=f"^Band index {bad} out of range. Available bands indices: 0 to 2.$"):
            Z._band_list([0, bad], 3)


def test_n_labels():
    lab = np.array([[0, 3], [7, -1]], np.int32)
    assert Z._n_labels(None, lab, 1) == 7 and Z._n_labels(None, lab, 0) == 8 and Z._n_labels(None, lab, 9) == 0
    assert Z._n_labels(5, lab, 1) == 5 and Z._n_labels(-3, lab, 1) == 0 and Z._n_labels(np.int64(4), lab, 1) == 4
    assert Z._n_labels(None, np.zeros((0, 4), np.int32), 1) == 0
    assert Z._n_labels(None, torch.as_tensor(lab), 1) == 7


def test_zonal_stats_of_arrays_needs_no_torch(monkeypatch):
    """the NumPy path calls the host entry points and never asks for torch: with the module's torch gone and the library stubbed, the
    call goes through and hands back the buffers it allocated (count 0, the rest NaN: the stub fills nothing)"""
    called = []

    class Lib:
        def obia_zonal_stats_f32(self, *a):
            called.append(("stats", len(a)))
            return 0

        def obia_zonal_moments_f32(self, *a):
            called.append(("moments", len(a)))
            return 0

    class Ctx:
        handle, device = None, 0
    monkeypatch.setattr(Z, "torch", None)
    monkeypatch.setattr(_device, "torch", None)
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    monkeypatch.setattr(_lib, "default_context", lambda dev=0: Ctx())
    raw = np.arange(24, dtype=np.float64).reshape(2, 3, 4)[:, :, ::2]
    lab = np.array([[1, 1, 2], [2, 3, 3]], np.int64)
    st = Z.zonal_stats(raw, lab, moments=True)
    assert called == [("stats", 15), ("moments", 13)]
    assert st["bands"] == [0, 1] and set(st) == {"count", "mean", "variance", "min", "max", "bands", "skewness", "kurtosis"}
    assert st["count"].dtype == np.int64 and st["count"].tolist() == [0, 0, 0]
    for k, dt in (("mean", np.float64), ("variance", np.float64), ("min", np.float32), ("max", np.float32), ("skewness", np.float64),
                  ("kurtosis", np.float64)):
        assert st[k].dtype == dt and st[k].shape == (3, 2) and np.isnan(st[k]).all()
    with pytest.raises(ImportError, match="^obia_amd.statistics.texture_stats needs torch for device memory$"):
        Z.texture_stats(raw, lab)
