"""MLP prediction, CPU side (no GPU): the NumPy restatement of the arithmetic contract (tests/mlp_restatement.py) against
scikit-learn's stored answers, the MLP container (validation, save / load, from_sklearn), the refusals at the limits and the host
checks of mlp_predict that come before the device is touched.  The fixtures come from tests/golden/gen_goldens_mlp.py."""
import importlib.util
import os

import numpy as np
import pytest

from tests import mlp_restatement as mr
from tests.mlp_restatement import ARRAYS, CASES, load_case, mlp_of


@pytest.mark.parametrize("name", CASES)
def test_restatement_against_sklearn(name):
    """scikit-learn's own float64 result lies E from the longdouble forward pass (E pooled over all fixtures, so that a lucky
    small case does not set the bar); the restatement adds in another order of the same length and must stay within 8 E."""
    c = load_case(name)
    E = mr.pooled_e_ref()
    assert 1e-16 < E < 1e-14 and float(c["e_ref"]) <= E
    proba = mr.predict_proba(c, c["transformed"])
    assert proba.dtype == np.float64 and proba.shape == c["proba"].shape
    err = float(np.abs(proba - c["proba_ld"]).max())
    print(f"{name}: max|proba - proba_ld| / E = {err / E:.3f}")
    assert err <= 8 * E
    assert np.array_equal(c["classes_"][np.argmax(proba, axis=1)], c["predict"])


def test_fixtures_reach_what_they_are_for():
    sizes = {n: load_case(n)["layer_sizes"].tolist() for n in CASES}
    assert sizes == {"a": [20, 100, 5], "b": [12, 100, 1], "c": [96, 64, 32, 7], "d": [30, 50, 4], "e": [3, 7, 9], "f": [6, 3]}
    acts = {n: (str(load_case(n)["hidden_activation"]), str(load_case(n)["out_activation"])) for n in CASES}
    assert acts["b"] == ("relu", "logistic") and acts["c"][0] == "tanh" and acts["d"][0] == "logistic" and acts["e"][0] == "identity"
    assert load_case("e")["classes_"].tolist() == [3, 5, 8, 13, 21, 34, 55, 89, 144] and len(load_case("e")["table"]) == 65
    for n in CASES:
        c = load_case(n)
        top = np.sort(c["proba"], axis=1)
        assert (top[:, -1] - top[:, -2]).min() >= 1e-6 and len(c["table"]) <= 1000 and c["transformed"].dtype == np.float64


def test_from_sklearn_equals_the_stored_arrays():
    sklearn = pytest.importorskip("sklearn")
    from obia_amd.classify import MLP
    spec = importlib.util.spec_from_file_location("gen_goldens_mlp", os.path.join(os.path.dirname(mr.GOLDEN), "gen_goldens_mlp.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for name in ("b", "e"):
        clf, fresh = gen.main(only=name, write=False)
        m = MLP.from_sklearn(clf)
        for ref in [fresh] + ([load_case(name)] if sklearn.__version__ == "1.7.2" else []):
            for k in ARRAYS + ("classes_",):
                assert np.array_equal(getattr(m, k), ref[k]) and getattr(m, k).dtype == ref[k].dtype, k
            assert (m.hidden_activation, m.out_activation) == (str(ref["hidden_activation"]), str(ref["out_activation"]))
        assert (m.n_features, m.n_layers, m.n_classes) == (int(fresh["layer_sizes"][0]), 2, len(clf.classes_))
    # float32 coefficients become float64, as NumPy promotes them against a float64 table
    clf.coefs_ = [w.astype(np.float32) for w in clf.coefs_]
    m32 = MLP.from_sklearn(clf)
    assert m32.weights.dtype == np.float64 and np.array_equal(m32.weights, np.concatenate([w.ravel() for w in clf.coefs_]).astype(np.float64))
    # multilabel: several logistic outputs
    from sklearn.neural_network import MLPClassifier
    rs = np.random.RandomState(0)
    multi = MLPClassifier(hidden_layer_sizes=(4,), max_iter=20, random_state=0)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        multi.fit(rs.normal(0, 1, (40, 3)), rs.randint(0, 2, (40, 3)))
    with pytest.raises(NotImplementedError, match="multilabel"):
        MLP.from_sklearn(multi)


def test_mlp_save_load_round_trip(tmp_path):
    from obia_amd.classify import MLP
    for name in ("c", "b"):
        m = mlp_of(load_case(name))
        path = m.save(str(tmp_path / f"{name}.npz"))
        with np.load(path, allow_pickle=False) as z:                  # plain arrays: loads with pickling refused
            assert set(z.files) == set(ARRAYS) | {"classes_", "hidden_activation", "out_activation"}
        g = MLP.load(path)
        for k in ARRAYS + ("classes_",):
            assert np.array_equal(getattr(m, k), getattr(g, k)) and getattr(m, k).dtype == getattr(g, k).dtype
        assert (g.hidden_activation, g.out_activation) == (m.hidden_activation, m.out_activation)
    assert (g.n_features, g.n_layers, g.n_classes) == (12, 2, 2)
    strs = MLP(classes_=np.array(["oak", "pine", "yew"]), **{k: v for k, v in mr.random_mlp(np.random.RandomState(0), [4, 5, 3]).items()
                                                              if k != "classes_"})
    assert list(MLP.load(strs.save(str(tmp_path / "s.npz"))).classes_) == ["oak", "pine", "yew"]
    assert [w.shape for w, _ in strs.layers()] == [(4, 5), (5, 3)] and [b.shape for _, b in strs.layers()] == [(5,), (3,)]


def test_mlp_rejects_arrays_that_do_not_fit():
    from obia_amd.classify import MLP
    base = mr.random_mlp(np.random.RandomState(1), [4, 5, 3])
    MLP(**base)
    for key, bad in (("weights", base["weights"][:-1]), ("biases", np.r_[base["biases"], 0.0]), ("layer_sizes", [4, 5]),
                     ("layer_sizes", [4, 0, 3]), ("layer_sizes", [4]), ("hidden_activation", "gelu"), ("out_activation", "identity"),
                     ("classes_", np.arange(4)), ("classes_", np.array([1, "a", None], dtype=object))):
        with pytest.raises(ValueError):
            MLP(**dict(base, **{key: bad}))
    with pytest.raises(ValueError):                                   # the logistic output is one unit for two classes
        MLP(**dict(base, out_activation="logistic"))
    with pytest.raises(ValueError):
        MLP(**dict(mr.random_mlp(np.random.RandomState(1), [4, 5, 1], out_activation="logistic"), classes_=np.arange(3)))


def test_refusals_at_the_limits():
    """Width 513, 65 classes, 9 weight matrices: NotImplementedError before the device is touched (512, 64 and 8 pass these
    checks: tests/test_gpu_mlp.py runs them)."""
    from obia_amd.classify import MLP, mlp_predict
    rs = np.random.RandomState(0)
    for sizes in ([3, 513, 4], [3, 8, 65], [3] + [4] * 9, [3, 4, 513, 4, 2]):
        with pytest.raises(NotImplementedError):
            mlp_predict(MLP(**mr.random_mlp(rs, sizes)), np.zeros((4, 3)))
    with pytest.raises(NotImplementedError):
        mlp_predict(MLP(**mr.random_mlp(rs, [4097, 2])), np.zeros((2, 4097)))


def test_host_checks_come_before_the_device():
    from obia_amd.classify import MLP, mlp_predict, standard_scale
    c = load_case("e")
    m = mlp_of(c)
    X = c["transformed"]
    acc = np.ones((len(X), 9), bool)
    acc[17, 1:] = False
    with pytest.raises(ValueError, match="row 17"):
        mlp_predict(m, X, acceptable=acc)
    with pytest.raises(ValueError):
        mlp_predict(m, X, acceptable=np.ones((len(X), 8), bool))
    with pytest.raises(ValueError, match="no rows"):
        mlp_predict(m, X[:0])
    with pytest.raises(ValueError, match="columns"):
        mlp_predict(m, X[:, :2])                                      # too few columns
    with pytest.raises(ValueError):
        mlp_predict(m, X[0])
    with pytest.raises(TypeError):
        mlp_predict(c, X)
    with pytest.raises(ValueError, match="dtype"):
        standard_scale(np.zeros((3, 2)), dtype=np.float16)
    with pytest.raises(ValueError, match="no rows"):
        standard_scale(np.zeros((0, 4)), dtype=np.float64)


def test_public_names_and_the_pinned_refusal():
    from obia_amd import MLP, classify, mlp_predict, predict_segments  # noqa: F401
    import inspect
    sig = inspect.signature(predict_segments)
    assert [p.name for p in sig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD] == ["classifier", "segments", "acceptable_classes_gdf"]
    assert [p.name for p in sig.parameters.values() if p.kind == p.KEYWORD_ONLY] == ["acceptable", "labels", "affine_transformation",
                                                                                      "start_label", "ctx"]
    with pytest.raises(NotImplementedError, match="predict_segments"):
        classify(None, None, method="mlp")
    with pytest.raises(TypeError):
        predict_segments(object.__new__(type("NotAClassifier", (), {"get_params": lambda self: {}})), None)
