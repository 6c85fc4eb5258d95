"""forest_shap without a GPU: the restatement (tests/shap_restatement.py) against the definition in exact rational arithmetic,
the fixtures of tests/golden/gen_goldens_shap.py against it and against scikit-learn's stored ``proba``, and the host side of
``Forest.cover`` / ``forest_shap``."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import forest_restatement as fr
from tests import shap_restatement as S


@pytest.fixture(scope="module")
def cases():
    """Every fixture once.  Nothing in here is modified by a test."""
    return {name: S.load_case(name) for name in S.CASES}


def same_exact(a, b):
    return a.shape == b.shape and all(u == v for u, v in zip(a.ravel(), b.ravel()))


@pytest.mark.parametrize("name", ["b", "c", "d"])
def test_fraction_restatement_equals_the_definition_on_fixtures(cases, name):
    c = cases[name]
    phi, base = S.shap_values(c, c["X32"], num=Fraction)
    for i in range(c["X32"].shape[0]):
        p, b = S.brute_force(c, c["X32"][i])
        assert same_exact(p, phi[i]) and same_exact(b, base), i
    # the stored answer is this one, rounded
    assert np.array_equal(S.to_float(phi), c["phi_exact"]) and np.array_equal(S.to_float(base), c["base_exact"])


@pytest.mark.parametrize("seed,n_trees,n_features,depth", [(1, 3, 4, 5), (2, 2, 6, 7), (3, 5, 2, 4)])
def test_fraction_restatement_equals_the_definition_on_synthetic_trees(seed, n_trees, n_features, depth):
    """Random trees whose children are not node + 1, random missing_go_to_left, NaNs in the rows, features repeated on a path
    (depth above the number of features); any element order gives the same exact answer."""
    rs = np.random.RandomState(seed)
    f = S.with_cover(fr.random_forest(rs, n_trees, n_features, 3, depth), rs)
    X = rs.normal(0, 1, (6, n_features)).astype(np.float32)
    X[rs.rand(6, n_features) < 0.2] = np.nan
    phi, base = S.shap_values(f, X, num=Fraction)
    assert any(len(e[4]) > 1 for p in S.paths(f) for e in p["elems"]) or n_features > depth
    for i in range(6):
        p, b = S.brute_force(f, X[i])
        assert same_exact(p, phi[i]) and same_exact(b, base)
    again, _ = S.shap_values(f, X, num=Fraction, order=7)
    assert same_exact(again, phi)


@pytest.mark.parametrize("name", S.CASES)
def test_float64_restatement_within_e_ref(cases, name):
    c = cases[name]
    phi, base = S.shap_values(c, c["X32"], num=float)
    e_ref = float(c["e_ref"])
    assert 2.0 ** -52 <= e_ref < 1e-9
    err = max(float(np.abs(phi - c["phi_exact"]).max()), float(np.abs(base - c["base_exact"]).max()))
    print(f"{name}: float64 restatement {err:.3e} from exact, e_ref {e_ref:.3e}")
    assert err <= e_ref
    used = np.unique(c["feature"][c["left"] >= 0])
    unused = np.setdiff1d(np.arange(c["X32"].shape[1]), used)
    assert (phi[:, unused, :] == 0.0).all() and (c["phi_exact"][:, unused, :] == 0.0).all()


@pytest.mark.parametrize("name", S.FOREST_CASES)
def test_exact_values_add_up_to_sklearn_proba(cases, name):
    """sum_f phi + base = v(all features) = the forest's prediction; scikit-learn's float64 mean of T leaf rows is within
    T 2^-53 of it (values in [0, 1])."""
    c = cases[name]
    g = fr.load_case(name)
    assert np.array_equal(g["transformed"][c["rows"]].astype(np.float32), c["X32"], equal_nan=True)
    N, F, K = c["phi_exact"].shape
    # math.fsum: the stored values added without a rounding of the sum's own
    total = np.array([[math.fsum(list(c["phi_exact"][i, :, k]) + [c["base_exact"][k]]) for k in range(K)] for i in range(N)])
    T = len(c["tree_offset"])
    err = float(np.abs(total - g["proba"][c["rows"]]).max())
    print(f"{name}: sum of the exact values {err:.3e} from scikit-learn's proba, bound {T * 2.0 ** -53:.3e}")
    assert err <= T * 2.0 ** -53


def test_exact_values_add_up_in_rationals(cases):
    """The same identity without any rounding on our side: forest c in Fractions against the restated prediction."""
    c = cases["c"]
    phi, base = S.shap_values(c, c["X32"][:6], num=Fraction)
    total = phi.sum(axis=1) + base[None, :]
    lv = fr.leaves(c, c["X32"][:6])
    T = lv.shape[0]
    for i in range(6):
        for k in range(c["value"].shape[1]):
            assert total[i, k] == sum(Fraction(float(c["value"][lv[t, i], k])) for t in range(T)) / T


def test_a_tree_that_is_one_leaf():
    f = {"threshold": np.array([-2.0]), "feature": np.array([-2], np.int32), "left": np.array([-1], np.int32),
         "right": np.array([-1], np.int32), "missing_go_to_left": np.zeros(1, np.uint8), "tree_offset": np.zeros(1, np.int64),
         "value": np.array([[0.25, 0.75]]), "cover": np.array([5.0])}
    for num in (float, Fraction):
        phi, base = S.shap_values(f, np.zeros((3, 4), np.float32), num=num)
        assert phi.shape == (3, 4, 2) and (phi == 0).all()
        assert [float(v) for v in base] == [0.25, 0.75]


def test_comb_fixtures_are_what_they_claim(cases):
    for name, n in (("comb16", 16), ("comb32", 32)):
        c = cases[name]
        ps = S.paths(c)
        assert max(len(p["elems"]) for p in ps) == n
        assert any(len(e[4]) > 3 for p in ps for e in p["elems"])                # the second tree repeats features
        inner = c["left"] >= 0
        size = np.diff(np.r_[c["tree_offset"], len(inner)])
        base = np.repeat(c["tree_offset"], size)
        assert (c["cover"] == np.round(c["cover"])).all()
        assert (c["cover"][inner] == c["cover"][(base + c["left"])[inner]] + c["cover"][(base + c["right"])[inner]]).all()
        # some rows reach the deepest leaf of the chain
        deepest = max(p["leaf"] for p in ps if p["tree"] == 0)
        assert (fr.leaves(c, c["X32"])[0] == deepest).sum() >= 2


def test_forest_carries_cover_through_save_and_load(tmp_path, cases):
    from obia_amd.classify import Forest
    c = cases["c"]
    f = S.forest_of(c)
    assert f.cover.dtype == np.float64 and np.array_equal(f.cover, c["cover"])
    g = Forest.load(f.save(str(tmp_path / "with_cover.npz")))
    assert np.array_equal(g.cover, c["cover"]) and np.array_equal(g.threshold, f.threshold)
    old = fr.forest_of(fr.load_case("c"))
    assert old.cover is None
    assert Forest.load(old.save(str(tmp_path / "without.npz"))).cover is None
    assert Forest.load(os.path.join(fr.GOLDEN, "forest", "c.npz")).cover is None      # a file written before there was a cover
    with pytest.raises(ValueError, match="cover"):
        Forest(classes_=c["classes_"], cover=c["cover"][:-1], **{k: c[k] for k in S.ARRAYS})


def test_from_sklearn_fills_cover():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import RandomForestClassifier
    from obia_amd.classify import Forest
    rs = np.random.RandomState(0)
    x, y = rs.normal(0, 1, (80, 4)), rs.randint(0, 3, 80)
    rf = RandomForestClassifier(n_estimators=3, random_state=0).fit(x, y)
    f = Forest.from_sklearn(rf)
    assert np.array_equal(f.cover, np.concatenate([e.tree_.weighted_n_node_samples for e in rf.estimators_]))
    assert f.cover[0] == 80.0


def test_host_refusals_happen_before_device_use(monkeypatch, cases):
    """No cover, a wrong shape, too many classes: refused before the library is loaded."""
    import importlib
    C = importlib.import_module("obia_amd.classify")
    if C.torch is None:
        pytest.skip("torch is not installed")

    def boom(*a, **k):
        raise AssertionError("the device was touched before the argument checks finished")
    monkeypatch.setattr(C._lib, "load", boom)
    monkeypatch.setattr(C._lib, "default_context", boom)
    c = cases["c"]
    X = c["X32"]
    with pytest.raises(ValueError, match="Forest.from_sklearn"):
        C.forest_shap(fr.forest_of(fr.load_case("c")), X)
    f = S.forest_of(c)
    with pytest.raises(TypeError):
        C.forest_shap(c, X)
    with pytest.raises(ValueError, match="rows, features"):
        C.forest_shap(f, X[0])
    with pytest.raises(ValueError, match="no rows"):
        C.forest_shap(f, X[:0])
    with pytest.raises(ValueError, match="columns"):
        C.forest_shap(f, X[:, :3])
    big = dict(c, value=np.zeros((len(c["left"]), 65)), classes_=np.arange(65))
    with pytest.raises(NotImplementedError, match="64 classes"):
        C.forest_shap(S.forest_of(big), X)


def test_classify_still_refuses_compute_shap_and_names_the_way():
    from obia_amd import ClassifiedImage, classify, forest_shap  # noqa: F401
    with pytest.raises(NotImplementedError, match="predict_segments.*compute_shap=True.*forest_shap"):
        classify(None, None, compute_shap=True)
    res = ClassifiedImage(None, None, None, None, None, None, {})
    assert res.shap_values is None and res.shap_base_values is None


def test_predict_segments_refuses_shap_for_an_mlp_and_unknown_keywords():
    pd = pytest.importorskip("pandas")
    from obia_amd.classify import MLP, predict_segments
    mlp = MLP(np.zeros(4), np.zeros(2), [2, 2], "relu", "softmax", np.arange(2))
    seg = pd.DataFrame({"a": [0.0, 1.0], "b": [1.0, 2.0]})
    with pytest.raises(NotImplementedError, match="forests only"):
        predict_segments(mlp, seg, compute_shap=True)
    with pytest.raises(TypeError, match="compute_sharp"):
        predict_segments(mlp, seg, compute_sharp=True)
