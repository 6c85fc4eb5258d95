"""The Python wrappers' device plumbing (obia_amd/_device.py): every public wrapper gets one small input four ways -- (a) contiguous
NumPy of the ABI dtype, (b) a non-contiguous NumPy view of a wider dtype, (c) a CUDA tensor, (d) a non-contiguous CUDA tensor of the
wider dtype -- and must return (a)'s result bit for bit (NaNs by position), in the kind that came in, on the input's device.  (b) and
(d) are upcasts of (a) (float32 -> float64, int32 -> int64), every second column of a padded buffer, so the values are the same.
Plumbing goes wrong on dtype, stride and device, not on size: the inputs are the smallest the operators' own tests use."""
import numpy as np
import pytest

from tests import forest_restatement as fr
from tests import mlp_restatement as mr
from tests import mlp_shap_restatement as sr
from tests import shap_restatement as tr

pytestmark = pytest.mark.gpu

H, W, C = 33, 37, 5
AFF = [0.5, 0.0, 0.0, -0.5, 100.0, 200.0]
_WIDER = {np.dtype(np.float32): np.float64, np.dtype(np.int32): np.int64}


def _padded(a):
    """`a` upcast, in every second column of a buffer twice as wide: `buffer[..., ::2] == a`, and that view is not contiguous"""
    buf = np.zeros(a.shape[:-1] + (2 * a.shape[-1],), _WIDER.get(a.dtype, a.dtype))
    buf[..., ::2] = a
    return buf


def variant(a, kind, device=0):
    import torch
    if kind == "a":
        return a
    if kind == "c":
        return torch.as_tensor(a).to(f"cuda:{device}")
    view = _padded(a)[..., ::2] if kind == "b" else torch.as_tensor(_padded(a)).to(f"cuda:{device}")[..., ::2]
    assert not (view.is_contiguous() if kind == "d" else view.flags.c_contiguous)
    return view


def leaves(out):
    """the arrays and tensors of a result, in a fixed order; anything else (a list of bands, a count) as it is"""
    from obia_amd.polygons import PolygonTable
    if isinstance(out, PolygonTable):
        return [out.xy, out.ring_offset, out.ring_label, out.ring_is_hole, out.ring_part]
    if isinstance(out, dict):
        return [sorted(out, key=str)] + [v for k in sorted(out, key=str) for v in leaves(out[k])]
    if isinstance(out, (tuple, list)) and any(hasattr(v, "shape") or isinstance(v, (tuple, list, dict)) for v in out):
        return [v for item in out for v in leaves(item)]
    return [out]


def same(x, y):
    """bit for bit, NaNs by position; tensors are compared by their host copies"""
    import torch
    if not hasattr(x, "shape") or not hasattr(y, "shape"):
        return type(x) is type(y) and x == y
    x, y = (np.ascontiguousarray(v.cpu().numpy() if torch.is_tensor(v) else v) for v in (x, y))
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if x.dtype.kind != "f":
        return x.tobytes() == y.tobytes()
    nx, ny = np.isnan(x), np.isnan(y)
    return bool((nx == ny).all()) and x[~nx].tobytes() == y[~ny].tobytes()


@pytest.fixture(scope="module")
def data():
    """Every input once.  Nothing in here is modified by a test."""
    rs = np.random.RandomState(7)
    yy, xx = np.mgrid[0:H, 0:W]
    d = {}
    d["raw"] = np.stack([300 + 200 * np.sin(xx / (9 + 2 * b)) * np.cos(yy / (7 + b)) + rs.normal(0, 15, (H, W)) for b in range(C)], -1).astype(np.float32)
    d["rawnan"] = d["raw"].copy()
    d["rawnan"][5, 6, 1] = np.nan
    d["rgb"] = np.ascontiguousarray(rs.rand(H, W, 3).astype(np.float32))
    d["labels"] = ((yy // 12) * 5 + xx // 8 + 1).astype(np.int32)                 # 15 segments, 1..15
    d["mask"] = ((yy - 16) ** 2 + (xx - 18) ** 2 < 14 ** 2).astype(np.int32)
    d["chm"] = np.maximum(0, 20 * np.sin(xx / 5.0) * np.sin(yy / 4.0) + rs.normal(0, 1, (H, W))).astype(np.float32)
    d["chm"][8:11, 12:15] = np.nan
    d["chm64"] = d["chm"].astype(np.float64)
    d["wv3"] = np.stack([300 + 200 * np.sin(xx[:17, :19] / (3 + b)) + rs.normal(0, 15, (17, 19)) for b in range(8)], -1).astype(np.float32)
    d["cost"] = rs.rand(H, W).astype(np.float32)
    d["xs"], d["ys"] = rs.uniform(1, W - 1, 12), rs.uniform(1, H - 1, 12)         # 12 seeds, float64
    d["points"] = np.stack([100 + 0.5 * rs.uniform(-2, W + 2, 12), 200 - 0.5 * rs.uniform(-2, H + 2, 12)], 1)
    fc = fr.load_case("c")
    d["forest"], d["X32"] = fr.forest_of(fc), fc["transformed"].astype(np.float32)
    tc = tr.load_case("c")                                                        # (the same forest with the nodes' cover)
    d["forest_cover"], d["X32_shap"] = tr.forest_of(tc), tc["X32"]
    mc = sr.load_case("r1")
    d["mlp"], d["X"], d["background"], d["values"] = mr.mlp_of(mc), mc["X"], mc["background"], mc["values_ld"]
    d["masks"] = np.ascontiguousarray(sr.all_masks(5))
    d["table"] = fc["table"]
    d["ring_xy"] = np.array([[2, 2], [20, 3], [18, 25], [3, 20], [2, 2], [10, 10], [30, 12], [25, 30], [10, 10]], np.float64) + 0.25
    d["ring_off"], d["ring_shape"] = np.array([0, 5, 9], np.int64), np.array([0, 1], np.int32)
    return d


def _seed_dicts(d):
    chm = {"x": d["xs"][:7], "y": d["ys"][:7], "ch_max": np.arange(7, dtype=np.float32)}
    den = {"x": d["xs"][7:], "y": d["ys"][7:], "den_max": np.arange(5, dtype=np.float32)}
    return chm, den


def _to_raster(labels):
    from obia_amd.classify import ClassifiedImage
    return ClassifiedImage({"predicted_class": np.arange(15) % 4}, None, None, None, None, None, {}).to_raster(labels)


def _cases():
    """name -> (names of the array arguments, call(d, *arrays), kind of the result: "in" (follows the input) or "numpy" (always
    host), kinds the wrapper accepts)"""
    from importlib import import_module
    K, U, T, P, S, G, Z, L = (import_module("obia_amd." + m) for m in ("classify", "consumers", "cost", "polygons", "seeds", "segmentation",
                                                                        "statistics", "tiling"))
    inv = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    pair = (inv, 0.5, 0.8)
    all4 = "abcd"
    return {
        "standard_scale": (["table"], lambda d, t: K.standard_scale(t), "in", all4),
        "standard_scale_f64": (["table"], lambda d, t: K.standard_scale(t, dtype=np.float64), "in", all4),
        "forest_predict": (["X32"], lambda d, x: K.forest_predict(d["forest"], x), "in", all4),
        "forest_shap": (["X32_shap"], lambda d, x: K.forest_shap(d["forest_cover"], x), "in", all4),
        "mlp_predict": (["X"], lambda d, x: K.mlp_predict(d["mlp"], x), "in", all4),
        "mlp_coalition_values": (["X", "background"], lambda d, x, b: K.mlp_coalition_values(d["mlp"], x, b, d["masks"]), "in", all4),
        "shapley_combine": (["values"], lambda d, v: K.shapley_combine(v), "in", all4),
        "mlp_shap": (["X", "background"], lambda d, x, b: K.mlp_shap(d["mlp"], x, b), "in", all4),
        "to_raster": (["labels"], lambda d, lab: _to_raster(lab), "in", all4),
        "zonal_stats": (["rawnan", "labels"], lambda d, r, lab: Z.zonal_stats(r, lab, moments=True), "in", all4),
        "zonal_stats_bands": (["raw", "labels"], lambda d, r, lab: Z.zonal_stats(r, lab, bands=np.array([3, 0]), n_labels=17), "in", all4),
        "texture_stats": (["raw", "labels"], lambda d, r, lab: Z.texture_stats(r, lab, bands=[1, 4]), "in", all4),
        "slic_edge": (["labels"], lambda d, lab: U.slic_edge(lab), "in", all4),
        "sample_labels": (["labels"], lambda d, lab: U.sample_labels(lab, AFF, d["points"]), "numpy", all4),
        "label_segments": (["labels"], lambda d, lab: U.label_segments(lab, AFF, d["points"], np.arange(12) % 3), "numpy", all4),
        "polygonize": (["labels"], lambda d, lab: P.polygonize(lab, affine_transformation=AFF, start_label=1), "numpy", all4),
        "rasterize": (["ring_xy", "ring_off", "ring_shape"], lambda d, xy, off, rs: P.rasterize((xy, off, rs), (H, W), values=np.array([7, 9])),
                      "numpy", all4),
        "slic": (["raw"], lambda d, r: G.slic(r, n_segments=12, compactness=10.0, _normalize_bands=True), "in", all4),
        "slic_mask": (["raw", "mask"], lambda d, r, m: G.slic(r, n_segments=8, mask=m, _normalize_bands=True), "in", all4),
        "slic_skimage": (["raw", "mask"], lambda d, r, m: G.slic(r, n_segments=8, mask=m, seeding="skimage", _normalize_bands=True), "in", all4),
        "quickshift": (["rgb"], lambda d, r: G.quickshift(r, kernel_size=3, max_dist=6, random_seed=42), "in", all4),
        "mask_centroids": (["mask"], lambda d, m: G.mask_centroids(m, 6), "numpy", all4),
        "enforce_connectivity": (["labels"], lambda d, lab: G.enforce_connectivity(lab, 4, 400), "in", "cd"),
        "create_segments": (["raw"], lambda d, r: G.create_segments(r, n_segments=12), "in", all4),
        "create_tiled_segments": (["raw", "mask"], lambda d, r, m: L.create_tiled_segments(r, input_mask=m, tile_size=16, buffer=4, crown_radius=2),
                                  "in", all4),
        "normalise": (["chm64"], lambda d, x: T.normalise(x), "in", all4),
        "chm_gradient": (["chm"], lambda d, x: T.chm_gradient(x), "in", all4),
        "ndvi": (["chm", "cost"], lambda d, r, n: T.ndvi(r, n), "in", all4),
        "texture_entropy": (["cost"], lambda d, x: T.texture_entropy(x), "in", all4),
        "make_cost_surface": (["wv3", "chm17", "labels17"], lambda d, w, c, s: T.make_cost_surface(w, c, slic=s, weights=(0.4, 0.3, 0.2, 0.1)),
                              "in", all4),
        "detect_peaks": (["chm"], lambda d, x: S.detect_peaks(x, 2.0, 2, 1), "in", all4),
        "make_chm_seeds": (["chm"], lambda d, x: S.make_chm_seeds(x, h_min_m=2.0, min_dist_px=2, affine_transformation=AFF), "in", all4),
        "make_density_seeds": (["chm"], lambda d, x: S.make_density_seeds(x, d_min=2.0, min_dist_px=2, gauss_sigma=0), "in", all4),
        "pair_distances": (["xs", "ys", "cost"], lambda d, x, y, c: S.pair_distances(x, y, c, *pair), "in", all4),
        "merge_clusters": (["xs", "ys", "cost"], lambda d, x, y, c: S.merge_clusters(x, y, c, *pair, 6.0), "in", all4),
        "pair_stats": (["xs", "ys", "cost"], lambda d, x, y, c: S.pair_stats(x, y, c, *pair), "numpy", all4),
        "make_canonical_seeds": (["cost"], lambda d, c: S.make_canonical_seeds(*_seed_dicts(d), c, merge_radius=6.0, debug_dist=False), "in", all4),
    }


# what a CUDA tensor input returns where it is not the NumPy call's dtype: scikit-image's intp for arrays, the kernel's int32 on the device
_TENSOR_DTYPE = {"slic": np.int32, "slic_mask": np.int32, "slic_skimage": np.int32, "quickshift": np.int32, "create_segments": np.int32}


def _names():
    return list(_cases())


def _args(d, names, kind, device=0):
    d = dict(d, chm17=d["chm"][:17, :19].copy(), labels17=d["labels"][:17, :19].copy())
    return [variant(d[n], kind, device) for n in names]


def _check(name, want, got, kind, result_kind, device=0):
    import torch
    lw, lg = leaves(want), leaves(got)
    assert len(lw) == len(lg), (name, kind)
    for i, (x, y) in enumerate(zip(lw, lg)):
        if hasattr(y, "shape") and not isinstance(y, np.generic) and not (isinstance(y, np.ndarray) and y.dtype.kind in "US"):   # (text stays NumPy)
            as_tensor = result_kind == "in" and kind in "cd"
            assert torch.is_tensor(y) == as_tensor, (name, kind, i, type(y))
            if as_tensor:
                assert y.device == torch.device(f"cuda:{device}"), (name, kind, i, y.device)
                if name in _TENSOR_DTYPE:
                    assert y.dtype == getattr(torch, np.dtype(_TENSOR_DTYPE[name]).name), (name, kind, i, y.dtype)
                    y = y.cpu().numpy().astype(x.dtype)
        assert same(x, y), (name, kind, i)


@pytest.fixture(scope="module")
def results(data):
    """(a)'s result of every wrapper, computed when first asked for and shared"""
    cases, cache = _cases(), {}

    def get(name):
        if name not in cache:
            names, call, _, kinds = cases[name]
            cache[name] = call(data, *_args(data, names, "a" if "a" in kinds else "c"))
        return cache[name]
    return get


@pytest.mark.parametrize("name", _names())
def test_four_input_kinds_one_result(data, results, name):
    names, call, result_kind, kinds = _cases()[name]
    want = results(name)
    first = kinds[0]
    _check(name, want, want, first, result_kind)
    for kind in kinds[1:]:
        _check(name, want, call(data, *_args(data, names, kind)), kind, result_kind)


def test_every_converted_wrapper_is_listed():
    listed = set(_names())
    assert len(listed) >= 35
    for need in ("standard_scale", "forest_predict", "forest_shap", "mlp_predict", "mlp_coalition_values", "shapley_combine", "mlp_shap",
                 "to_raster", "zonal_stats", "texture_stats", "slic_edge", "sample_labels", "label_segments", "polygonize", "rasterize",
                 "slic", "quickshift", "mask_centroids", "enforce_connectivity", "create_tiled_segments", "normalise", "chm_gradient",
                 "ndvi", "texture_entropy", "make_cost_surface", "detect_peaks", "make_chm_seeds", "make_density_seeds", "pair_distances",
                 "merge_clusters", "pair_stats", "make_canonical_seeds"):
        assert need in listed, need


@pytest.mark.parametrize("name", ["zonal_stats", "slic_edge", "forest_predict"])
def test_a_tensor_on_the_second_device_stays_there(data, results, name):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    names, call, result_kind, _ = _cases()[name]
    _check(name, results(name), call(data, *_args(data, names, "c", device=1)), "c", result_kind, device=1)
