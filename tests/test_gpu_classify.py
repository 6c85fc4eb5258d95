"""Classification on the GPU (csrc/classify.hip): forest_predict against scikit-learn's stored answers bit for bit,
standard_scale against exactly rounded column sums, the zone mask, to_raster and the composed classify().  The fixtures come from
tests/golden/gen_goldens_forest.py; only the composition test needs scikit-learn."""
import math

import numpy as np
import pytest

from tests import forest_restatement as fr
from tests.forest_restatement import ARRAYS, CASES, forest_of, load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    """Every fixture once: arrays, the Forest and its float32 input.  Nothing in here is modified by a test."""
    out = {}
    for name in CASES:
        c = load_case(name)
        out[name] = dict(c, forest=forest_of(c), X32=c["transformed"].astype(np.float32))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def synthetic(seed, n_trees, n_features, n_classes, depth, leaf_only=False):
    return forest_of(fr.random_forest(np.random.RandomState(seed), n_trees, n_features, n_classes, depth, leaf_only=leaf_only))


def rows(seed, n, n_features, nan=0.1):
    rs = np.random.RandomState(seed)
    x = rs.normal(0, 1, (n, n_features)).astype(np.float32)
    x[rs.rand(n, n_features) < nan] = np.nan
    return x


@pytest.mark.parametrize("name", CASES)
def test_forest_predict_equals_sklearn_bit_for_bit(cases, name):
    from obia_amd.classify import forest_predict
    c = cases[name]
    pred, margin, proba = forest_predict(c["forest"], c["X32"])
    assert proba.dtype == np.float64 and pred.dtype == np.int32 and margin.dtype == np.float64
    assert same_bits(proba, c["proba"])
    assert np.array_equal(c["classes_"][pred], c["predict"])
    top = np.sort(c["proba"], axis=1)
    assert same_bits(margin, top[:, -1] - top[:, -2])
    again = forest_predict(c["forest"], c["X32"])
    assert all(same_bits(u, v) for u, v in zip((pred, margin, proba), again))


@pytest.mark.parametrize("name", ["a", "c"])
def test_forest_predict_with_a_mask(cases, name):
    """A random mask with at least two acceptable classes per row, a third of the rows unmasked (all classes acceptable)."""
    import torch
    from obia_amd.classify import forest_predict
    c = cases[name]
    N, K = c["proba"].shape
    rs = np.random.RandomState(11)
    acc = rs.rand(N, K) < 0.5
    for i in np.flatnonzero(acc.sum(1) < 2):
        acc[i, rs.choice(K, 2, replace=False)] = True
    acc[rs.rand(N) < 0.33] = True
    free = np.argmax(c["proba"], axis=1)
    assert (~acc[np.arange(N), free]).sum() > 10           # rows whose mask excludes the overall winner are in the data
    assert (acc.sum(1) >= 2).all() and acc.all(1).any()
    want_pred, want_margin = fr.choose(c["proba"], acc)
    pred, margin, proba = forest_predict(c["forest"], c["X32"], acceptable=acc)
    assert same_bits(proba, c["proba"])                     # never filtered
    assert np.array_equal(pred, want_pred) and same_bits(margin, want_margin)
    # CUDA tensors in -> CUDA tensors out, same values
    tp, tm, tq = forest_predict(c["forest"], torch.as_tensor(c["X32"]).cuda(), acceptable=torch.as_tensor(acc).cuda())
    assert tp.is_cuda and tm.is_cuda and tq.is_cuda
    assert np.array_equal(tp.cpu().numpy(), want_pred) and same_bits(tm.cpu().numpy(), want_margin)


def exact_columns(table):
    """Per column over its non-NaN values, with math.fsum (correctly rounded sums): n, mean, variance (two-pass with the
    correction term, on the rounded differences) and mean |x|."""
    n, mean, var, mabs = [], [], [], []
    for col in table.T:
        v = [float(x) for x in col[~np.isnan(col)]]
        k = len(v)
        n.append(k)
        if k == 0:
            mean.append(float("nan")), var.append(float("nan")), mabs.append(float("nan"))
            continue
        m = math.fsum(v) / k
        d = [x - m for x in v]
        mean.append(m)
        var.append((math.fsum(x * x for x in d) - math.fsum(d) ** 2 / k) / k)
        mabs.append(math.fsum(abs(x) for x in v) / k)
    return np.array(n), np.array(mean), np.array(var), np.array(mabs)


@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_standard_scale(cases, name):
    """Bounds (derived, not measured): any float64 summation of n terms is within n 2^-53 sum|x| of the exact sum, so the mean is
    within n 2^-52 mean|x| of the exactly rounded one (both sides round once more); the variance -- sums of squared ROUNDED
    differences, the correction term, two divisions -- within n 2^-50 relative; the scale is its square root, which halves a
    relative error and rounds once: n 2^-51 + 2^-52 relative.  n <= 3000 here."""
    from obia_amd.classify import standard_scale
    c = cases[name]
    table = c["table"]
    X32, mean, scale = standard_scale(table)
    assert X32.dtype == np.float32 and X32.shape == table.shape and mean.dtype == scale.dtype == np.float64
    n, m_ref, v_ref, mabs = exact_columns(table)
    empty = n == 0
    const = c["scale_"] == 1.0                                 # the columns scikit-learn treats as constant
    assert np.isnan(mean[empty]).all() and np.isnan(scale[empty]).all() and np.isnan(X32[:, empty]).all()
    live = ~empty
    print("mean error / bound:", np.nanmax(np.abs(mean[live] - m_ref[live]) / (n[live] * 2.0 ** -52 * mabs[live])))
    assert (np.abs(mean[live] - m_ref[live]) <= n[live] * 2.0 ** -52 * mabs[live]).all()
    assert (scale[const] == 1.0).all() and (v_ref[const] == 0.0).all()
    assert (X32[:, const][~np.isnan(table[:, const])] == 0.0).all()
    reg = live & ~const
    s_ref = np.sqrt(v_ref[reg])
    print("scale error / bound:", np.max(np.abs(scale[reg] - s_ref) / ((n[reg] * 2.0 ** -51 + 2.0 ** -52) * s_ref)))
    assert (np.abs(scale[reg] - s_ref) <= (n[reg] * 2.0 ** -51 + 2.0 ** -52) * s_ref).all()
    if name == "a":
        assert empty[3] and const[5] and const.sum() == 1 and empty.sum() == 1
    if name == "e":
        assert list(np.flatnonzero(empty)) == [96, 97, 98, 99, 100]      # the reference's point-cloud columns pass through
    # the transform alone: from the kernel's own mean and scale, bit for bit
    with np.errstate(invalid="ignore"):
        want = ((table - mean) / scale).astype(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(X32), nan) and np.array_equal(nan, np.isnan(table) | empty[None, :])
    assert same_bits(np.where(nan, np.float32(0), X32), np.where(nan, np.float32(0), want))
    again = standard_scale(table)
    assert all(same_bits(u, v) for u, v in zip((X32, mean, scale), again))
    # scikit-learn's own numbers obey the same bounds, so the two agree within twice them; what the forest sees is the same table
    assert np.allclose(mean[live], c["mean_"][live], rtol=0, atol=float(np.max(n[live] * 2.0 ** -51 * mabs[live])))
    assert np.allclose(scale[live], c["scale_"][live], rtol=float(np.max(n[live])) * 2.0 ** -50, atol=0)


def test_standard_scale_tensor_in_tensor_out(cases):
    import torch
    from obia_amd.classify import standard_scale
    table = cases["b"]["table"]
    X32, mean, scale = standard_scale(table)
    tx, tm, ts = standard_scale(torch.as_tensor(table).cuda())
    assert tx.is_cuda and tm.is_cuda and ts.is_cuda
    assert same_bits(tx.cpu().numpy(), X32) and same_bits(tm.cpu().numpy(), mean) and same_bits(ts.cpu().numpy(), scale)
    with pytest.raises(ValueError, match="no rows"):
        standard_scale(torch.zeros((0, 3), dtype=torch.float64).cuda())


@pytest.mark.parametrize("n_rows,n_trees,n_features,n_classes,depth,leaf_only", [
    (1, 5, 4, 3, 4, False),          # one row
    (65, 5, 4, 3, 4, False),         # one row more than a workgroup takes
    (130, 37, 7, 64, 5, False),      # the most classes; more trees than one chunk of 32, not a multiple of it
    (70, 3, 160, 5, 6, False),       # the first table width whose rows are not staged in LDS (159 is the last that is)
    (70, 3, 159, 5, 6, False),
    (40, 6, 3, 4, 0, True),          # every tree a single leaf
])
def test_forest_predict_edges(n_rows, n_trees, n_features, n_classes, depth, leaf_only):
    from obia_amd.classify import forest_predict
    f = synthetic(5, n_trees, n_features, n_classes, depth, leaf_only)
    X = rows(6, n_rows, n_features)
    want = fr.predict_proba(f, X)
    want_pred, want_margin = fr.choose(want)
    pred, margin, proba = forest_predict(f, X)
    assert same_bits(proba, want) and np.array_equal(pred, want_pred) and same_bits(margin, want_margin)
    if leaf_only:
        assert (f.left < 0).all() and f.n_nodes == n_trees


def test_forest_predict_refusals():
    from obia_amd.classify import forest_predict
    with pytest.raises(NotImplementedError):
        forest_predict(synthetic(1, 2, 3, 65, 2), rows(1, 4, 3))
    with pytest.raises(ValueError, match="no rows"):
        forest_predict(synthetic(1, 2, 3, 4, 2), rows(1, 4, 3)[:0])


def test_abi_refuses_what_python_would_not_send():
    """The C entry points check for themselves: 65 classes is OBIA_E_UNSUPPORTED, a child index outside its tree is
    OBIA_E_INVALID and is never followed, an empty table is OBIA_E_INVALID."""
    import ctypes
    import torch
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    d = fr.random_forest(np.random.RandomState(2), 2, 3, 4, 3)
    x = torch.as_tensor(rows(3, 10, 3, nan=0)).cuda()

    def call(arr, n_classes=4, n_rows=10):
        t = {k: torch.as_tensor(np.ascontiguousarray(arr[k])).cuda() for k in ARRAYS}
        off = np.ascontiguousarray(arr["tree_offset"], np.int64)
        fs = _lib.Forest(*(t[k].data_ptr() for k in ARRAYS[:6]), off.ctypes.data, t["value"].data_ptr(), len(arr["threshold"]), len(off), n_classes)
        proba = torch.zeros((10, max(n_classes, 4)), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        return lib.obia_forest_predict_dev(ctx.handle, x.data_ptr(), n_rows, 3, ctypes.byref(fs), None, proba.data_ptr(), None, None)

    assert call(d) == _lib.OBIA_OK
    assert call(d, n_classes=65) == _lib.E_UNSUPPORTED
    bad = dict(d, right=d["right"].copy())
    bad["right"][0] = 10 ** 6
    assert call(bad) == _lib.E_INVALID and "out of range" in _lib.last_error()
    t = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    o = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    assert lib.obia_table_scale_dev(ctx.handle, t.data_ptr(), 0, 3, t.data_ptr(), t.data_ptr(), o.data_ptr()) == _lib.E_INVALID


# -------------------------------------------------------------------------------------------- zones, raster, composition
def quadrants():
    lab = np.zeros((8, 8), np.int32)
    lab[:4, :4], lab[:4, 4:], lab[4:, :4], lab[4:, 4:] = 1, 2, 3, 4
    return lab


def test_zone_mask_on_the_label_raster():
    """Four 4 x 4 segments, two rectangular zones on pixel edges (pixel coordinates).  Zone 0 = [0, 4] x [0, 6] covers segment 1
    and the two upper pixel rows of segment 3; it touches segments 2 and 4 along x = 4 without covering a pixel centre.
    Zone 1 = [2, 8] x [4, 8] covers segment 4 and the right half of segment 3, where it overlaps zone 0 (the first row wins the
    pixel, and the lowest row index wins the segment); it touches segment 2 along y = 4 only.  Segment 2 lies under no zone."""
    from obia_amd.classify import acceptable_mask
    rect = lambda x0, y0, x1, y1: np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)], np.float64)   # noqa: E731
    zones = {"geometry": [rect(0, 0, 4, 6), rect(2, 4, 8, 8)], "acceptable_classes": [[10, 30], [20, 30, 99]]}
    mask = acceptable_mask(zones, np.array([10, 20, 30]), quadrants())
    assert mask.dtype == bool and mask.tolist() == [[True, False, True],      # segment 1: zone 0
                                                    [True, True, True],       # segment 2: no zone
                                                    [True, False, True],      # segment 3: zones 0 and 1 -> the first
                                                    [False, True, True]]      # segment 4: zone 1 (99 is no class of the forest)
    # the same zones as WKB, given in map coordinates
    import struct
    wkb = [struct.pack("<BII", 1, 3, 1) + struct.pack("<I", 5) + (r * [2.0, -2.0] + [100.0, 50.0]).astype("<f8").tobytes()
           for r in zones["geometry"]]
    mask2 = acceptable_mask({"geometry": wkb, "acceptable_classes": zones["acceptable_classes"]}, np.array([10, 20, 30]), quadrants(),
                            affine_transformation=[2.0, 0.0, 0.0, -2.0, 100.0, 50.0])
    assert np.array_equal(mask2, mask)


def test_to_raster():
    import torch
    from obia_amd.classify import ClassifiedImage
    lab = quadrants()
    lab[0, 0] = 0                                                     # a masked pixel
    ci = ClassifiedImage({"predicted_class": np.array([10, 20, 30, 20])}, None, None, None, None, None, {})
    want = np.where(lab == 0, -1, np.array([0, 10, 20, 30, 20])[lab]).astype(np.int32)
    out = ci.to_raster(lab, fill=-1)
    assert out.dtype == np.int32 and np.array_equal(out, want)
    t = ci.to_raster(torch.as_tensor(lab).cuda(), fill=-1)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), want)
    # labels need not be consecutive: the rows are the labels that exist, ascending
    assert np.array_equal(ci.to_raster(np.where(lab > 0, lab * 3, 0), fill=-1), want)
    with pytest.raises(ValueError):
        ClassifiedImage({"predicted_class": np.array(["a", "b", "c", "d"])}, None, None, None, None, None, {}).to_raster(lab)
    with pytest.raises(ValueError):
        ClassifiedImage({"predicted_class": np.array([1, 2, 3])}, None, None, None, None, None, {}).to_raster(lab)


def test_classify_composes_the_stages():
    """Wiring: a 64 x 80 raster segmented, described and labelled by this package, then classify().  predicted_class and
    prediction_margin equal scikit-learn's predict_proba of the same forest on the table standard_scale returned."""
    pytest.importorskip("sklearn")
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import train_test_split
    from sklearn.preprocessing import StandardScaler
    from obia_amd import create_objects, slic
    from obia_amd.classify import ClassifiedImage, classify, standard_scale
    from obia_amd.consumers import label_segments
    rs = np.random.RandomState(0)
    H, W = 64, 80
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([300 * np.sin(xx / (7 + 2 * c)) * np.cos(yy / (9 + c)) + 1000 + rs.normal(0, 15, (H, W)) for c in range(3)], -1).astype(np.float32)
    labels = slic(img, n_segments=60, compactness=0.5, _normalize_bands=True)
    table = create_objects(labels, img, geometry=False)
    affine = [1.0, 0.0, 0.0, -1.0, 0.0, float(H)]
    py, px = np.mgrid[2:H:5, 2:W:5]
    pts = np.stack([px.ravel() + 0.5, H - (py.ravel() + 0.5)], 1)
    cls = np.digitize(img[py.ravel(), px.ravel(), 0], [900, 1100]) * 10 + 10          # classes 10 / 20 / 30 from band 0
    labelled, _ = label_segments(labels, affine, pts, cls)
    assert len(labelled) >= 20 and len(set(labelled.values())) == 3
    training = table[table["segment_id"].isin(list(labelled))].copy()
    training["feature_class"] = [labelled[int(s)] for s in training["segment_id"]]
    kw = dict(n_estimators=12, random_state=3)
    segments = table.copy()
    res = classify(segments, training, compute_reports=True, **kw)
    assert isinstance(res, ClassifiedImage) and res.classified is segments and res.params["n_estimators"] == 12
    assert res.report is not None and res.confusion_matrix.shape[0] >= 2 and res.shap_values is None
    # the reference's host steps, again
    x = training.drop(["feature_class", "geometry", "segment_id"], axis=1)
    x_train, _, y_train, _ = train_test_split(x, training["feature_class"], test_size=0.2, random_state=42)
    rf = RandomForestClassifier(**kw).fit(StandardScaler().fit_transform(x_train), y_train)
    x_pred = table.drop(["geometry", "segment_id"], axis=1).to_numpy(dtype=np.float64)
    X32, _, _ = standard_scale(x_pred)
    proba = rf.predict_proba(X32)
    top = np.sort(proba, axis=1)
    assert np.array_equal(np.asarray(segments["predicted_class"], dtype=np.int64), rf.classes_[np.argmax(proba, axis=1)])
    assert same_bits(np.asarray(segments["prediction_margin"], dtype=np.float64), top[:, -1] - top[:, -2])
    assert str(segments["predicted_class"].dtype) == "Int64" and len(set(segments["predicted_class"])) >= 2
    # class per pixel, and a zone that forbids class 10 everywhere
    ras = res.to_raster(labels)
    assert ras.shape == (H, W) and set(np.unique(ras)) <= {10, 20, 30}
    zones = {"geometry": [np.array([(0, 0), (W, 0), (W, H), (0, H)], np.float64)], "acceptable_classes": [[20, 30]]}
    res2 = classify(table.copy(), training, zones, labels=labels, affine_transformation=affine, **kw)
    assert 10 not in set(res2.classified["predicted_class"])
    sub = proba[:, 1:]
    assert np.array_equal(np.asarray(res2.classified["predicted_class"], dtype=np.int64), rf.classes_[1:][np.argmax(sub, axis=1)])
