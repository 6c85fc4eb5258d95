"""mlp_shap without a GPU: the restatement (tests/mlp_shap_restatement.py) against the definition in exact rational arithmetic, the
fixtures of tests/golden/gen_goldens_mlp_shap.py against it, and the host side of ``mlp_coalition_values`` / ``shapley_combine`` /
``mlp_shap`` / ``predict_segments(shap_background=...)``."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import mlp_restatement as mr
from tests import mlp_shap_restatement as S


@pytest.fixture(scope="module")
def cases():
    """Every fixture once.  Nothing in here is modified by a test."""
    return {name: S.load_case(name) for name in S.CASES}


def same_exact(a, b):
    return a.shape == b.shape and all(u == v for u, v in zip(a.ravel(), b.ravel()))


def test_public_names_are_exported():
    from obia_amd import mlp_coalition_values, mlp_shap, shapley_combine  # noqa: F401
    import importlib
    C = importlib.import_module("obia_amd.classify")       # (obia_amd.classify the attribute is the function)
    assert C.SHAP_MAX_FEATURES == 16 and C._SHAP_VALUES_BYTES == 256 << 20


@pytest.mark.parametrize("F,K", [(1, 2), (2, 1), (3, 3), (4, 2), (5, 3)])
def test_subset_formula_equals_the_permutation_definition(F, K):
    rs = np.random.RandomState(100 + F)
    values = rs.rand(2, 1 << F, K)
    phi = S.shapley(values, num=Fraction)
    for n in range(2):
        assert same_exact(phi[n], S.shapley_by_permutations(values[n]))


@pytest.mark.parametrize("name", ["r1", "r2"])
def test_subset_formula_equals_the_permutation_definition_on_fixtures(cases, name):
    c = cases[name]
    phi = S.shapley(c["values_ld"], num=Fraction)
    for n in range(c["X"].shape[0]):
        assert same_exact(phi[n], S.shapley_by_permutations(c["values_ld"][n]))


def test_size_weights_are_rounded_rationals_that_sum_to_one():
    from obia_amd.classify import _size_weights
    for F in (1, 2, 9, 16):
        w = S.size_weights(F, Fraction)
        assert sum(math.comb(F - 1, s) * w[s] for s in range(F)) == 1
        assert _size_weights(F).tolist() == [float(v) for v in w] == S.size_weights(F).tolist()


@pytest.mark.parametrize("name", S.CASES)
def test_efficiency_holds_exactly(cases, name):
    """sum_f phi[f] = v(all features) - v(no feature), in Fractions."""
    v = cases[name]["values_ld"]
    phi = S.shapley(v, num=Fraction)
    for n in range(v.shape[0]):
        for k in range(v.shape[2]):
            assert sum(phi[n, :, k]) == Fraction(float(v[n, -1, k])) - Fraction(float(v[n, 0, k]))


def test_a_null_feature_gets_exactly_zero(cases):
    """Row 0 of r1 equals every background row in column 2: the two hybrid rows of a coalition are the same bits."""
    c = cases["r1"]
    assert (c["background"][:, 2] == c["X"][0, 2]).all() and not (c["background"][:, 2] == c["X"][1, 2]).all()
    bit = 1 << 2
    m = np.arange(32)
    m = m[m & bit == 0]
    assert np.array_equal(c["values_ld"][0, m], c["values_ld"][0, m | bit])
    assert all(t == 0 for t in S.shapley(c["values_ld"], num=Fraction)[0, 2])
    got = S.shapley(c["values_ld"], num=float)
    assert got[0, 2].tobytes() == np.zeros(3).tobytes() and (c["phi_exact"][0, 2] == 0).all() and (got[1, 2] != 0).all()
    v = S.coalition_values(c, c["X"][:1], c["background"], S.all_masks(5))
    assert np.array_equal(v[0, m], v[0, m | bit])


def test_a_duplicated_feature_gets_the_same_value_exactly():
    """A game that does not change when features 1 and 3 are exchanged (built so, on a grid where the sums are exact)."""
    rs = np.random.RandomState(5)
    F, i, j = 4, 1, 3
    u = np.round(rs.rand(1, 1 << F, 2) * 2 ** 20) / 2 ** 20
    m = np.arange(1 << F)
    bi, bj = (m >> i) & 1, (m >> j) & 1
    swapped = (m & ~((1 << i) | (1 << j))) | (bi << j) | (bj << i)
    v = u + u[:, swapped, :]
    assert np.array_equal(v, v[:, swapped, :])
    phi = S.shapley(v, num=Fraction)
    assert same_exact(phi[:, i, :], phi[:, j, :]) and not same_exact(phi[:, 0, :], phi[:, 2, :])
    assert same_exact(phi[0], S.shapley_by_permutations(v[0]))


@pytest.mark.parametrize("name", S.CASES)
def test_fixtures_are_what_they_claim(cases, name):
    """phi_exact / base_exact / e_comb recomputed from values_ld, and the float64 restatement of the coalition values within the
    bar of DESIGN.md 3.5j -- 8 E, E the pooled distance of scikit-learn's own proba from the longdouble forward pass -- of values_ld:
    a mean of numbers within 8 E is within 8 E."""
    c = cases[name]
    N, F = c["X"].shape
    K = len(c["classes_"])
    assert c["values_ld"].shape == (N, 1 << F, K) and c["phi_exact"].shape == (N, F, K) and c["base_exact"].shape == (K,)
    assert np.array_equal(S.to_float(S.shapley(c["values_ld"], num=Fraction)), c["phi_exact"])
    assert np.array_equal(c["base_exact"], c["values_ld"][0, 0]) and (c["values_ld"][:, 0] == c["base_exact"]).all()
    e_comb = max(2.0 ** -52, float(np.abs(S.shapley(c["values_ld"], num=float) - c["phi_exact"]).max()))
    assert e_comb == float(c["e_comb"]) and e_comb < 1e-14
    E = mr.pooled_e_ref()
    v = S.coalition_values(c, c["X"], c["background"], S.all_masks(F))
    err = float(np.abs(v - c["values_ld"]).max())
    print(f"{name}: float64 restatement of the coalition values {err:.3e} from the longdouble ones = {err / E:.2f} E")
    assert err <= 8 * E
    if name == "author":
        assert c["layer_sizes"].tolist() == [9, 100, 50, 30, 6] and str(c["hidden_activation"]) == "relu"


def test_hybrid_rows_and_ordered_mean():
    x, bg = np.array([1.0, 2.0, 3.0]), np.array([[10.0, 20.0, 30.0], [40.0, 50.0, 60.0]])
    h = S.hybrid_rows(x, bg, S.all_masks(3))
    assert h.shape == (8, 2, 3)
    assert h[0].tolist() == bg.tolist() and h[7].tolist() == [[1.0, 2.0, 3.0]] * 2 and h[5].tolist() == [[1.0, 20.0, 3.0], [1.0, 50.0, 3.0]]
    p = np.array([[[0.1], [0.2], [0.3]]])
    assert S.ordered_mean(p)[0, 0] == ((0.0 + 0.1) + 0.2 + 0.3) / 3.0


def test_host_refusals_happen_before_device_use(monkeypatch, cases):
    """17 features, an empty background, wrong column counts, a CPU tensor, bad masks and bad values: refused before the library is
    loaded.  ``shap_background`` with a forest is a ValueError: the forest's explainer takes no background data, so the value of
    the argument is what is wrong, not its name."""
    import importlib
    pd = pytest.importorskip("pandas")
    C = importlib.import_module("obia_amd.classify")
    if C.torch is None:
        pytest.skip("torch is not installed")

    def boom(*a, **k):
        raise AssertionError("the device was touched before the argument checks finished")
    monkeypatch.setattr(C._lib, "load", boom)
    monkeypatch.setattr(C._lib, "default_context", boom)
    c = cases["r1"]
    mlp, X, B = mr.mlp_of(c), c["X"], c["background"]
    masks = S.all_masks(5)
    wide = mr.mlp_of(mr.random_mlp(np.random.RandomState(0), [17, 4, 3]))
    with pytest.raises(NotImplementedError, match="16 features.*mlp_coalition_values"):
        C.mlp_shap(wide, np.zeros((2, 17)), np.zeros((3, 17)))
    for fn, extra in ((C.mlp_shap, ()), (C.mlp_coalition_values, (masks,))):
        with pytest.raises(TypeError):
            fn(c, X, B, *extra)
        with pytest.raises(ValueError, match="background has no rows"):
            fn(mlp, X, B[:0], *extra)
        with pytest.raises(ValueError, match="no rows"):
            fn(mlp, X[:0], B, *extra)
        with pytest.raises(ValueError, match="X has 4 columns"):
            fn(mlp, X[:, :4], B, *extra)
        with pytest.raises(ValueError, match="background has 6 columns"):
            fn(mlp, X, np.zeros((3, 6)), *extra)
        with pytest.raises(ValueError, match="rows, features"):
            fn(mlp, X[0], B, *extra)
        with pytest.raises(ValueError, match="must live on the GPU"):
            fn(mlp, C.torch.as_tensor(X), B, *extra)
        with pytest.raises(ValueError, match="must live on the GPU"):
            fn(mlp, X, C.torch.as_tensor(B), *extra)
    with pytest.raises(ValueError, match="masks must be"):
        C.mlp_coalition_values(mlp, X, B, masks[:, :4])
    with pytest.raises(ValueError, match="masks must be"):
        C.mlp_coalition_values(mlp, X, B, masks[:0])
    big = mr.mlp_of(mr.random_mlp(np.random.RandomState(0), [3, 513, 2]))
    with pytest.raises(NotImplementedError, match="512 units"):
        C.mlp_coalition_values(big, np.zeros((1, 3)), np.zeros((1, 3)), S.all_masks(3))
    with pytest.raises(ValueError, match="2\\^F coalitions"):
        C.shapley_combine(np.zeros((2, 6, 3)))
    with pytest.raises(ValueError, match="2\\^F coalitions"):
        C.shapley_combine(np.zeros((2, 1, 3)))
    with pytest.raises(ValueError, match="must live on the GPU"):
        C.shapley_combine(C.torch.zeros((2, 4, 3), dtype=C.torch.float64))
    with pytest.raises(NotImplementedError, match="16 features"):
        C.shapley_combine(np.zeros((1, 1 << 17, 1)))

    seg = pd.DataFrame({"a": [0.0, 1.0], "b": [1.0, 2.0]})
    leaf = np.array([-1], np.int32)
    forest = C.Forest(np.array([-2.0]), np.array([-2], np.int32), leaf, leaf, np.zeros(1, np.uint8), np.zeros(1, np.int64),
                      np.array([[0.25, 0.75]]), np.arange(2), n_features=2, cover=np.array([5.0]))
    with pytest.raises(ValueError, match="shap_background.*MLP"):
        C.predict_segments(forest, seg, compute_shap=True, shap_background=np.zeros((2, 2)))
    two = C.MLP(np.zeros(4), np.zeros(2), [2, 2], "relu", "softmax", np.arange(2))
    with pytest.raises(ValueError, match="compute_shap=True"):
        C.predict_segments(two, seg, shap_background=np.zeros((2, 2)))
    with pytest.raises(NotImplementedError, match="forests only"):
        C.predict_segments(two, seg, compute_shap=True)
    with pytest.raises(TypeError, match="shap_backgrounds"):
        C.predict_segments(two, seg, compute_shap=True, shap_backgrounds=np.zeros((2, 2)))
    wide_seg = pd.DataFrame(np.zeros((2, 17)), columns=[f"f{i}" for i in range(17)])
    with pytest.raises(NotImplementedError, match="16 features"):
        C.predict_segments(wide, wide_seg, compute_shap=True, shap_background=np.zeros((2, 17)))
