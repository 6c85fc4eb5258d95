"""MLP prediction on the GPU (csrc/mlp.hip): mlp_predict against the NumPy restatement of its arithmetic contract bit for bit
where the activations are exact, against scikit-learn's stored answers within a tolerance derived from scikit-learn's own error,
the class filter, the kernel's thresholds, the refusals, standard_scale(dtype=float64) and predict_segments.  The fixtures come
from tests/golden/gen_goldens_mlp.py; only the composition test needs scikit-learn."""
import numpy as np
import pytest

from tests import forest_restatement as fr
from tests import mlp_restatement as mr
from tests.mlp_restatement import CASES, load_case, mlp_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    """Every fixture once: arrays, the MLP, the restatement's logits and the pooled E.  Nothing in here is modified by a test."""
    out = {}
    for name in CASES:
        c = load_case(name)
        out[name] = dict(c, mlp=mlp_of(c), logits=mr.logits(c, c["transformed"]))
    return out


@pytest.fixture(scope="module")
def E():
    return mr.pooled_e_ref()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["a", "b", "e", "f"])
def test_logits_equal_the_restatement_bit_for_bit(cases, name):
    """relu and identity are exact, so the last layer before its activation is the ordered sums alone."""
    from obia_amd.classify import mlp_predict
    c = cases[name]
    pred, margin, proba, logits = mlp_predict(c["mlp"], c["transformed"], _logits=True)
    assert proba.dtype == np.float64 and pred.dtype == np.int32 and margin.dtype == np.float64 and logits.dtype == np.float64
    assert proba.shape == c["proba"].shape and logits.shape == c["logits"].shape
    assert same_bits(logits, c["logits"])
    again = mlp_predict(c["mlp"], c["transformed"], _logits=True)
    assert all(same_bits(u, v) for u, v in zip((pred, margin, proba, logits), again))


@pytest.mark.parametrize("name", CASES)
def test_proba_within_eight_times_sklearns_own_error(cases, E, name):
    """E = max over all fixtures of max|scikit-learn's proba - the longdouble forward pass|: where scikit-learn's own float64
    result sits.  Ours adds a different but equally long summation order and the device's exp / tanh (a few ulp): 8 E.  Measured
    ratios: DESIGN.md 3.5j.  The fixtures' top-two margins are at least 1e-6, so no row is left out of the class comparison."""
    from obia_amd.classify import mlp_predict
    c = cases[name]
    pred, margin, proba = mlp_predict(c["mlp"], c["transformed"])
    err = float(np.abs(proba - c["proba_ld"]).max())
    print(f"{name}: max|proba - proba_ld| / E = {err / E:.3f}")
    assert err <= 8 * E
    assert np.array_equal(c["classes_"][pred], c["predict"])
    top = np.sort(c["proba"], axis=1)
    merr = float(np.abs(margin - (top[:, -1] - top[:, -2])).max())
    print(f"{name}: max|margin - scikit-learn's| / E = {merr / E:.3f}")
    assert merr <= 16 * E


@pytest.mark.parametrize("name", ["a", "e"])
def test_mlp_predict_with_a_mask(cases, name):
    """A random mask with at least two acceptable classes per row, a third of the rows unmasked (all classes acceptable)."""
    import torch
    from obia_amd.classify import mlp_predict
    c = cases[name]
    X = c["transformed"]
    _, _, own = mlp_predict(c["mlp"], X)
    N, K = own.shape
    rs = np.random.RandomState(11)
    acc = rs.rand(N, K) < 0.5
    for i in np.flatnonzero(acc.sum(1) < 2):
        acc[i, rs.choice(K, 2, replace=False)] = True
    acc[rs.rand(N) < 0.33] = True
    free = np.argmax(own, axis=1)
    assert (~acc[np.arange(N), free]).sum() > 5             # rows whose mask excludes the overall winner are in the data
    assert (acc.sum(1) >= 2).all() and acc.all(1).any()
    want_pred, want_margin = fr.choose(own, acc)
    pred, margin, proba = mlp_predict(c["mlp"], X, acceptable=acc)
    assert same_bits(proba, own)                            # never filtered
    assert np.array_equal(pred, want_pred) and same_bits(margin, want_margin)
    tp, tm, tq = mlp_predict(c["mlp"], torch.as_tensor(X).cuda(), acceptable=torch.as_tensor(acc).cuda())
    assert tp.is_cuda and tm.is_cuda and tq.is_cuda
    assert np.array_equal(tp.cpu().numpy(), want_pred) and same_bits(tm.cpu().numpy(), want_margin) and same_bits(tq.cpu().numpy(), own)


# (layer sizes, rows, (rows a workgroup takes, features staged at a time) the kernel must choose for them)
EDGES = [
    ([5, 16, 3], 1, (64, 5)),                     # one row
    ([5, 16, 3], 65, (64, 5)),                    # one row more than a workgroup takes
    ([5, 16, 3], 135, (64, 5)),                   # two workgroups and a partial one
    ([94, 16, 3], 70, (64, 94)),                  # the widest input layer this network stages in one piece ...
    ([95, 16, 3], 70, (64, 94)),                  # ... and the first that comes in two
    ([300, 100, 5], 33, (32, 54)),                # 32 rows per workgroup, six pieces, the last one shorter
    ([6, 1, 4], 70, (64, 6)),                     # hidden width 1
    ([10, 200, 3], 33, (16, 10)),                 # 16 rows per workgroup
    ([10, 300, 3], 17, (8, 10)),                  # 8
    ([10, 512, 3], 9, (4, 10)),                   # hidden width 512: 4 rows per workgroup
    ([7, 9, 10, 11, 12, 13, 14, 15, 4], 70, (64, 7)),   # 8 weight matrices
    ([5, 20, 64], 70, (32, 5)),                   # the most classes: the output layer is the widest, 32 rows per workgroup
    ([5, 8, 2], 70, (64, 5)),                     # two classes with softmax
]


@pytest.mark.parametrize("sizes,n_rows,plan", EDGES, ids=[f"{'-'.join(map(str, s))}x{n}" for s, n, _ in EDGES])
def test_mlp_predict_edges(E, sizes, n_rows, plan):
    """Synthetic relu networks against the restatement: logits bit for bit, proba within 8 E of the restatement's (the same
    logits; only exp differs, by a few ulp of values that are at most 1), class and margin by the selection rule on own proba."""
    from obia_amd.classify import _mlp_plan, mlp_predict
    assert _mlp_plan(sizes) == plan
    net = mr.random_mlp(np.random.RandomState(5), sizes)
    X = np.random.RandomState(6).normal(0, 1, (n_rows, sizes[0]))
    want = mr.logits(net, X)
    pred, margin, proba, logits = mlp_predict(mlp_of(net), X, _logits=True)
    assert same_bits(logits, want)
    assert np.abs(proba - mr.proba_of_logits(want, "softmax")).max() <= 8 * E
    want_pred, want_margin = fr.choose(proba)
    assert np.array_equal(pred, want_pred) and same_bits(margin, want_margin)


def test_refusals():
    """The C entry points check for themselves: 65 classes is OBIA_E_UNSUPPORTED, an empty table is OBIA_E_INVALID on the float64
    scaler; through mlp_predict a NaN or an infinity anywhere in the table raises ValueError."""
    import ctypes
    import torch
    from obia_amd import _lib
    from obia_amd.classify import mlp_predict
    lib, ctx = _lib.load(), _lib.default_context(0)
    x = torch.zeros((10, 3), dtype=torch.float64, device="cuda")

    def call(sizes, n_classes):
        ls = np.asarray(sizes, np.int32)
        w = torch.zeros((int((ls[:-1] * ls[1:]).sum()),), dtype=torch.float64, device="cuda")
        b = torch.zeros((int(ls[1:].sum()),), dtype=torch.float64, device="cuda")
        ms = _lib.Mlp(w.data_ptr(), b.data_ptr(), ls.ctypes.data, len(sizes) - 1, 1, 0, n_classes)
        proba = torch.zeros((10, n_classes), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        return lib.obia_mlp_predict_dev(ctx.handle, x.data_ptr(), 10, 3, ctypes.byref(ms), None, proba.data_ptr(), None, None, None)

    assert call([3, 4, 5], 5) == _lib.OBIA_OK
    assert call([3, 4, 65], 65) == _lib.E_UNSUPPORTED
    assert call([3, 513, 5], 5) == _lib.E_UNSUPPORTED
    assert call([3, 4, 5], 4) == _lib.E_INVALID             # softmax: one output per class
    t = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    o = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    assert lib.obia_table_scale_f64_dev(ctx.handle, t.data_ptr(), 0, 3, t.data_ptr(), t.data_ptr(), o.data_ptr()) == _lib.E_INVALID

    net = mlp_of(mr.random_mlp(np.random.RandomState(1), [6, 8, 3]))
    X = np.random.RandomState(2).normal(0, 1, (200, 6))
    mlp_predict(net, X)
    for value in (np.nan, np.inf):
        Xb = X.copy()
        Xb[137, 4] = value
        with pytest.raises(ValueError, match="NaN"):
            mlp_predict(net, Xb)


@pytest.mark.parametrize("source", ["forest/a", "mlp/c"])
def test_standard_scale_float64(source):
    """The same mean and scale as the float32 call, bit for bit; the table is (table - mean) / scale in float64 and its cast is
    the float32 call's table.  forest/a has an all-NaN column, a constant one and scattered NaNs."""
    from obia_amd.classify import standard_scale
    kind, name = source.split("/")
    table = (fr.load_case(name) if kind == "forest" else load_case(name))["table"]
    X32, mean32, scale32 = standard_scale(table)
    X64, mean, scale = standard_scale(table, dtype=np.float64)
    assert X64.dtype == np.float64 and X64.shape == table.shape
    assert same_bits(mean, mean32) and same_bits(scale, scale32)
    with np.errstate(invalid="ignore"):
        want = (table - mean) / scale
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(X64), nan) and (kind == "mlp" or nan.any())
    assert same_bits(np.where(nan, 0.0, X64), np.where(nan, 0.0, want))
    assert np.array_equal(np.isnan(X32), nan) and same_bits(np.where(nan, np.float32(0), X64.astype(np.float32)), np.where(nan, np.float32(0), X32))


def test_standard_scale_float64_tensor_in_tensor_out():
    import torch
    from obia_amd.classify import standard_scale
    table = load_case("b")["table"]
    X64, mean, scale = standard_scale(table, dtype=np.float64)
    tx, tm, ts = standard_scale(torch.as_tensor(table).cuda(), dtype=np.float64)
    assert tx.is_cuda and tx.dtype == torch.float64 and tm.is_cuda and ts.is_cuda
    assert same_bits(tx.cpu().numpy(), X64) and same_bits(tm.cpu().numpy(), mean) and same_bits(ts.cpu().numpy(), scale)


def test_predict_segments_composes_the_stages(E):
    """Wiring: the 64 x 80 raster of test_classify_composes_the_stages segmented, described and labelled by this package.  An
    MLPClassifier fitted on the host, then predict_segments(): classes equal scikit-learn's on the float64 table standard_scale
    returns wherever scikit-learn's own margin exceeds 16 E (twice what two probabilities, each 8 E off, can move their
    difference), margins within 16 E.  A fitted forest through predict_segments() reproduces classify() bit for bit."""
    pytest.importorskip("sklearn")
    import warnings
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import train_test_split
    from sklearn.neural_network import MLPClassifier
    from sklearn.preprocessing import StandardScaler
    from obia_amd import create_objects, predict_segments, slic
    from obia_amd.classify import MLP, ClassifiedImage, classify, standard_scale
    from obia_amd.consumers import label_segments
    rs = np.random.RandomState(0)
    H, W = 64, 80
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([300 * np.sin(xx / (7 + 2 * c)) * np.cos(yy / (9 + c)) + 1000 + rs.normal(0, 15, (H, W)) for c in range(3)], -1).astype(np.float32)
    labels = slic(img, n_segments=60, compactness=0.5, _normalize_bands=True)
    full = create_objects(labels, img, geometry=False)
    affine = [1.0, 0.0, 0.0, -1.0, 0.0, float(H)]
    py, px = np.mgrid[2:H:5, 2:W:5]
    pts = np.stack([px.ravel() + 0.5, H - (py.ravel() + 0.5)], 1)
    cls = np.digitize(img[py.ravel(), px.ravel(), 0], [900, 1100]) * 10 + 10          # classes 10 / 20 / 30 from band 0
    labelled, _ = label_segments(labels, affine, pts, cls)

    def training_of(table):
        t = table[table["segment_id"].isin(list(labelled))].copy()
        t["feature_class"] = [labelled[int(s)] for s in t["segment_id"]]
        return t

    # ---- MLP: the table without its all-NaN columns (MLPClassifier takes no NaN)
    all_nan = [c for c in full.columns if c not in ("geometry", "segment_id") and full[c].isna().all()]
    assert len(all_nan) == 5                                                          # the point-cloud columns
    table = full.drop(columns=all_nan)
    feats = table.drop(["geometry", "segment_id"], axis=1)
    assert not feats.isna().any().any()
    training = training_of(table)
    clf = MLPClassifier(hidden_layer_sizes=(16,), random_state=0, max_iter=500)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf.fit(StandardScaler().fit_transform(training.drop(["feature_class", "geometry", "segment_id"], axis=1)), training["feature_class"])
    segments = table.copy()
    res = predict_segments(clf, segments)
    assert isinstance(res, ClassifiedImage) and res.classified is segments and res.params["hidden_layer_sizes"] == (16,)
    assert res.report is None and res.confusion_matrix is None
    X64, _, _ = standard_scale(feats.to_numpy(dtype=np.float64), dtype=np.float64)
    proba = clf.predict_proba(X64)
    top = np.sort(proba, axis=1)
    sk_margin = top[:, -1] - top[:, -2]
    clear = sk_margin > 16 * E
    print(f"rows whose scikit-learn margin exceeds 16 E: {clear.mean():.3f} of {len(clear)}")
    assert clear.mean() >= 0.95
    got = np.asarray(segments["predicted_class"], dtype=np.int64)
    assert np.array_equal(got[clear], clf.predict(X64)[clear])
    assert np.abs(np.asarray(segments["prediction_margin"], dtype=np.float64) - sk_margin).max() <= 16 * E
    assert str(segments["predicted_class"].dtype) == "Int64"
    # the container instead of the estimator: the same numbers, no params
    res_m = predict_segments(MLP.from_sklearn(clf), table.copy())
    assert res_m.params == {} and np.array_equal(np.asarray(res_m.classified["predicted_class"], dtype=np.int64), got)
    assert same_bits(np.asarray(res_m.classified["prediction_margin"], dtype=np.float64), np.asarray(segments["prediction_margin"], dtype=np.float64))

    # ---- forest: classify() and predict_segments() with the forest classify() fitted
    training = training_of(full)
    kw = dict(n_estimators=12, random_state=3)
    want = classify(full.copy(), training, **kw).classified
    x = training.drop(["feature_class", "geometry", "segment_id"], axis=1)
    x_train, _, y_train, _ = train_test_split(x, training["feature_class"], test_size=0.2, random_state=42)
    rf = RandomForestClassifier(**kw).fit(StandardScaler().fit_transform(x_train), y_train)
    res_f = predict_segments(rf, full.copy())
    assert res_f.params["n_estimators"] == 12
    assert np.array_equal(np.asarray(res_f.classified["predicted_class"], dtype=np.int64), np.asarray(want["predicted_class"], dtype=np.int64))
    assert same_bits(np.asarray(res_f.classified["prediction_margin"], dtype=np.float64), np.asarray(want["prediction_margin"], dtype=np.float64))
