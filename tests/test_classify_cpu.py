"""Classification, CPU side (no GPU): the NumPy restatement of scikit-learn's forest prediction equals scikit-learn's stored
answers bit for bit, Forest reads / saves / loads the flat arrays, and the class filter and its errors behave like the
reference's loop (classify.py:135-158).  The fixtures come from tests/golden/gen_goldens_forest.py."""
import importlib.util
import os

import numpy as np
import pytest

from tests import forest_restatement as fr
from tests.forest_restatement import ARRAYS, CASES, GOLDEN, forest_of, load_case


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_sklearn_bit_for_bit(name):
    c = load_case(name)
    proba = fr.predict_proba(c, c["transformed"])
    assert proba.dtype == np.float64 and np.array_equal(proba, c["proba"])
    pred, margin = fr.choose(proba)
    assert np.array_equal(c["classes_"][pred], c["predict"])
    top = np.sort(c["proba"], axis=1)
    assert np.array_equal(margin, top[:, -1] - top[:, -2])


def test_fixtures_reach_what_they_are_for():
    a, c = load_case("a"), load_case("c")
    top = np.sort(a["proba"], axis=1)
    assert (top[:, -1] == top[:, -2]).sum() > 100                    # ties at the top: the first-maximum rule decides
    assert np.isnan(a["table"][:, 3]).all() and np.ptp(a["table"][:, 5]) == 0 and a["scale_"][5] == 1.0
    assert 0 < np.isnan(a["table"][:, 7]).mean() < 0.3 and np.isnan(a["table"][:, 9]).any()
    assert a["missing_go_to_left"].any() and not a["missing_go_to_left"].all()
    inner = c["left"] >= 0
    local = np.arange(len(c["left"])) - np.repeat(c["tree_offset"], np.diff(np.r_[c["tree_offset"], len(c["left"])]))
    assert (c["left"][inner] != local[inner] + 1).any()              # best-first trees
    assert load_case("e")["table"].shape == (1000, 101) and len(load_case("d")["tree_offset"]) == 200


@pytest.mark.parametrize("name", ["b", "c"])
def test_from_sklearn_equals_the_stored_arrays(name):
    sklearn = pytest.importorskip("sklearn")
    from obia_amd.classify import Forest
    spec = importlib.util.spec_from_file_location("gen_goldens_forest", os.path.join(GOLDEN, "gen_goldens_forest.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rf, fresh = gen.main(only=name, write=False)
    f = Forest.from_sklearn(rf)
    # against the estimator itself (any version), and against the stored fixture with the version that wrote it
    for ref in [fresh] + ([load_case(name)] if sklearn.__version__ == "1.7.2" else []):
        for k in ARRAYS + ("classes_",):
            assert np.array_equal(getattr(f, k), ref[k]) and getattr(f, k).dtype == ref[k].dtype, k
    assert f.n_features == int(fresh["n_features"])
    assert np.array_equal(fr.predict_proba(f, fresh["transformed"]), rf.predict_proba(fresh["transformed"]))


def test_forest_save_load_round_trip(tmp_path):
    f = forest_of(load_case("c"))
    path = f.save(str(tmp_path / "forest.npz"))
    with np.load(path, allow_pickle=False) as z:                      # plain arrays: loads with pickling refused
        assert set(z.files) == set(ARRAYS) | {"classes_", "n_features"}
    from obia_amd.classify import Forest
    g = Forest.load(path)
    for k in ARRAYS + ("classes_",):
        assert np.array_equal(getattr(f, k), getattr(g, k)) and getattr(f, k).dtype == getattr(g, k).dtype
    assert g.n_features == f.n_features == 6 and (g.n_trees, g.n_classes, g.n_nodes) == (3, 9, 99)
    strs = Forest(classes_=np.array(["oak", "pine"]), **{k: v for k, v in fr.random_forest(np.random.RandomState(0), 2, 3, 2, 2).items()
                                                       if k in ARRAYS})
    assert list(Forest.load(strs.save(str(tmp_path / "s.npz"))).classes_) == ["oak", "pine"]


def test_forest_rejects_arrays_a_walk_could_leave():
    from obia_amd.classify import Forest
    base = {k: v for k, v in fr.random_forest(np.random.RandomState(1), 2, 4, 3, 3).items() if k in ARRAYS}
    inner = int(np.flatnonzero(base["left"] >= 0)[0])
    for key, bad in (("left", 10 ** 6), ("right", -1), ("feature", -3)):
        broken = {k: v.copy() for k, v in base.items()}
        broken[key][inner] = bad
        with pytest.raises(ValueError):
            Forest(classes_=np.arange(3), **broken)
    with pytest.raises(ValueError):
        Forest(classes_=np.arange(3), n_features=1, **base)           # a node tests a feature beyond the table
    with pytest.raises(ValueError):
        Forest(classes_=np.arange(3), **dict(base, tree_offset=np.array([1, 2])))


def test_mask_rule_on_the_restatement():
    proba = np.array([[0.5, 0.3, 0.2], [0.2, 0.4, 0.4], [0.1, 0.1, 0.8], [0.25, 0.5, 0.25]])
    pred, margin = fr.choose(proba)
    assert list(pred) == [0, 1, 2, 1] and np.array_equal(margin, [0.5 - 0.3, 0.0, 0.8 - 0.1, 0.25])
    acc = np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0], [1, 1, 1]], bool)
    pred, margin = fr.choose(proba, acc)
    assert list(pred) == [1, 2, 0, 1]                                 # rows 0 and 2 lose their overall winner; row 2 ties: first wins
    assert np.array_equal(margin, [0.3 - 0.2, 0.4 - 0.2, 0.0, 0.25])
    with pytest.raises(ValueError):
        fr.choose(proba, np.array([[1, 1, 1], [0, 1, 0], [1, 1, 1], [1, 1, 1]], bool))   # one candidate: np.partition(..., -2) raises
    with pytest.raises(ValueError):
        fr.choose(proba, np.array([[1, 1, 1], [0, 0, 0], [1, 1, 1], [1, 1, 1]], bool))   # none: idxmax raises
    with pytest.raises(ValueError):
        fr.choose(np.ones((3, 1)))                                    # one class, no mask


def test_host_checks_come_before_the_device():
    """forest_predict / standard_scale / classify refuse what the reference refuses (and what the kernel does not support)
    before they touch the device: these raise on a machine without a GPU as well."""
    from obia_amd.classify import Forest, classify, forest_predict, standard_scale
    c = load_case("c")
    f = forest_of(c)
    X = c["transformed"].astype(np.float32)
    acc = np.ones((len(X), 9), bool)
    acc[17, 1:] = False
    with pytest.raises(ValueError, match="row 17"):
        forest_predict(f, X, acceptable=acc)
    with pytest.raises(ValueError):
        forest_predict(f, X, acceptable=np.ones((len(X), 8), bool))
    with pytest.raises(ValueError, match="no rows"):
        forest_predict(f, X[:0])
    with pytest.raises(ValueError, match="no rows"):
        standard_scale(np.zeros((0, 4)))
    with pytest.raises(ValueError):
        forest_predict(f, X[:, :3])                                   # the forest tests columns the table does not have
    one = Forest(classes_=[7], **{k: v for k, v in fr.random_forest(np.random.RandomState(0), 2, 3, 1, 2).items() if k in ARRAYS})
    with pytest.raises(ValueError, match="two classes"):
        forest_predict(one, np.zeros((4, 3), np.float32))
    wide = Forest(classes_=np.arange(65), **{k: v for k, v in fr.random_forest(np.random.RandomState(0), 2, 3, 65, 2).items() if k in ARRAYS})
    with pytest.raises(NotImplementedError):
        forest_predict(wide, np.zeros((4, 3), np.float32))
    with pytest.raises(NotImplementedError):
        classify(None, None, method="mlp")
    with pytest.raises(NotImplementedError):
        classify(None, None, compute_shap=True)
    with pytest.raises(ValueError):
        classify(None, None, method="svm")


def test_classify_keeps_the_reference_signature():
    import inspect
    from obia_amd.classify import ClassifiedImage, classify
    sig = inspect.signature(classify)
    pos = [(p.name, p.default) for p in sig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert pos == [("segments", inspect.Parameter.empty), ("training_classes", inspect.Parameter.empty), ("acceptable_classes_gdf", None),
                   ("method", "rf"), ("test_size", 0.2), ("compute_reports", False), ("compute_shap", False), ("sample_shap", False)]
    assert any(p.kind == p.VAR_KEYWORD for p in sig.parameters.values())
    ci = ClassifiedImage("t", "cm", "rep", None, None, None, {"n_estimators": 3})
    assert (ci.classified, ci.confusion_matrix, ci.report, ci.shap_values, ci.transform, ci.crs, ci.params) == \
        ("t", "cm", "rep", None, None, None, {"n_estimators": 3})
