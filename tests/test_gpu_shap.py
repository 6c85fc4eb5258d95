"""SHAP values of a forest on the GPU (csrc/shap.hip): forest_shap against exact rational arithmetic.  The fixtures come from
tests/golden/gen_goldens_shap.py (``phi_exact`` / ``base_exact``: the answer in Fractions, rounded; ``e_ref``: how far the float64
algorithm strays from it over nine element orders); the small edge cases are evaluated in Fractions here.  The bar everywhere is
8 e_ref: the kernel's order of operations is a tenth order.  Nothing here needs scikit-learn."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

from tests import forest_restatement as fr
from tests import shap_restatement as S

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cases():
    """Every fixture once with its Forest and the GPU's answer for its rows.  Nothing in here is modified by a test."""
    from obia_amd.classify import forest_shap
    out = {}
    for name in S.CASES:
        c = S.load_case(name)
        forest = S.forest_of(c)
        phi, base = forest_shap(forest, c["X32"])
        out[name] = dict(c, forest=forest, phi=phi, base=base)
    return out


def exact_of(arrays, X32):
    """(phi_exact, base_exact, e): the Fraction answer rounded to float64 and the distance of the float64 restatement (natural
    order) from it, floored at 2^-52 -- e_ref of a case evaluated here instead of stored."""
    phi_q, base_q = S.shap_values(arrays, X32, num=Fraction)
    phi_x, base_x = S.to_float(phi_q), S.to_float(base_q)
    phi_f, base_f = S.shap_values(arrays, X32, num=float)
    e = max(2.0 ** -52, float(np.abs(phi_f - phi_x).max()), float(np.abs(base_f - base_x).max()))
    return phi_x, base_x, e


def check(arrays, X32, label):
    from obia_amd.classify import forest_shap
    phi_x, base_x, e = exact_of(arrays, X32)
    phi, base = forest_shap(S.forest_of(arrays), X32)
    assert phi.dtype == np.float64 and phi.shape == phi_x.shape and base.dtype == np.float64 and base.shape == base_x.shape
    err_phi, err_base = float(np.abs(phi - phi_x).max()), float(np.abs(base - base_x).max())
    print(f"{label}: phi {err_phi:.3e}, base {err_base:.3e} from exact; bar {8 * e:.3e}")
    assert err_phi <= 8 * e and err_base <= 8 * e
    return phi, base


def synthetic(seed, n_trees, n_features, n_classes, depth, leaf_only=False):
    rs = np.random.RandomState(seed)
    return S.with_cover(fr.random_forest(rs, n_trees, n_features, n_classes, depth, leaf_only=leaf_only), rs)


def rows(seed, n, n_features, nan=0.1):
    rs = np.random.RandomState(seed)
    x = rs.normal(0, 1, (n, n_features)).astype(np.float32)
    x[rs.rand(n, n_features) < nan] = np.nan
    return x


def joined(a, b):
    """Two dicts of flat arrays as one forest: the trees of ``a``, then those of ``b``."""
    out = {k: np.concatenate([a[k], b[k]]) for k in S.ARRAYS + ("cover",) if k != "tree_offset"}
    out["tree_offset"] = np.concatenate([a["tree_offset"], b["tree_offset"] + len(a["left"])])
    out["classes_"] = a["classes_"]
    out["n_features"] = max(int(a["n_features"]), int(b["n_features"]))
    return out


@pytest.mark.parametrize("name", S.CASES)
def test_forest_shap_within_8_e_ref_of_exact(cases, name):
    c = cases[name]
    N, F = c["X32"].shape
    assert c["phi"].dtype == np.float64 and c["phi"].shape == (N, F, c["value"].shape[1]) and c["base"].shape == (c["value"].shape[1],)
    e_ref = float(c["e_ref"])
    err_phi = float(np.abs(c["phi"] - c["phi_exact"]).max())
    err_base = float(np.abs(c["base"] - c["base_exact"]).max())
    print(f"{name}: phi {err_phi:.3e}, base {err_base:.3e} from exact; e_ref {e_ref:.3e}, bar {8 * e_ref:.3e}")
    assert err_phi <= 8 * e_ref and err_base <= 8 * e_ref
    used = np.unique(c["feature"][c["left"] >= 0])
    unused = np.setdiff1d(np.arange(F), used)
    assert same_bits(c["phi"][:, unused, :], np.zeros((N, len(unused), c["phi"].shape[2])))


@pytest.mark.parametrize("name", S.CASES)
def test_values_add_up_to_the_prediction(cases, name):
    """|sum_f phi + base - proba| <= (F + 1) 8 e_ref + T 2^-53: F + 1 terms each within 8 e_ref of exact, whose exact sum is the
    exact prediction, from which forest_predict's float64 mean of T leaf rows is T 2^-53 away at most."""
    from obia_amd.classify import forest_predict
    c = cases[name]
    _, _, proba = forest_predict(c["forest"], c["X32"])
    F, T = c["X32"].shape[1], len(c["tree_offset"])
    gap = float(np.abs(c["phi"].sum(axis=1) + c["base"][None, :] - proba).max())
    bound = (F + 1) * 8 * float(c["e_ref"]) + T * 2.0 ** -53
    print(f"{name}: additivity gap {gap:.3e}, bound {bound:.3e}")
    assert gap <= bound


def test_repeatable_and_independent_of_the_other_rows(cases):
    import torch
    from obia_amd.classify import forest_shap
    c = cases["a"]
    phi, base = forest_shap(c["forest"], c["X32"])
    assert same_bits(phi, c["phi"]) and same_bits(base, c["base"])
    part, base_part = forest_shap(c["forest"], c["X32"][3:5])
    assert same_bits(part, c["phi"][3:5]) and same_bits(base_part, c["base"])
    tphi, tbase = forest_shap(c["forest"], torch.as_tensor(c["X32"]).cuda())
    assert tphi.is_cuda and tbase.is_cuda and tphi.dtype == torch.float64
    assert same_bits(tphi.cpu().numpy(), c["phi"]) and same_bits(tbase.cpu().numpy(), c["base"])


@pytest.fixture(scope="module")
def small():
    """A forest of 3 random trees over 5 features (repeats on the paths, children that are not node + 1, random
    missing_go_to_left) with 65 rows and their exact answer."""
    arrays = synthetic(21, 3, 5, 3, 6)
    X = rows(22, 65, 5)
    return arrays, X, exact_of(arrays, X)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_row_counts_around_a_wave(small, n):
    from obia_amd.classify import forest_shap
    arrays, X, (phi_x, base_x, e) = small
    phi, base = forest_shap(S.forest_of(arrays), X[:n])
    err = max(float(np.abs(phi - phi_x[:n]).max()), float(np.abs(base - base_x).max()))
    print(f"N = {n}: {err:.3e} from exact, bar {8 * e:.3e}")
    assert phi.shape == (n, 5, 3) and err <= 8 * e


def test_leaf_only_forest():
    arrays = synthetic(23, 3, 4, 3, 3, leaf_only=True)
    phi, base = check(arrays, rows(24, 5, 4), "leaf-only forest")
    assert same_bits(phi, np.zeros((5, 4, 3)))


def test_one_tree_is_a_single_leaf_among_split_trees():
    arrays = joined(joined(synthetic(25, 1, 4, 3, 4), synthetic(26, 1, 4, 3, 3, leaf_only=True)), synthetic(27, 2, 4, 3, 5))
    assert len(arrays["tree_offset"]) == 4 and arrays["left"][arrays["tree_offset"][1]] < 0
    check(arrays, rows(28, 20, 4), "a single leaf among split trees")


def test_more_columns_than_any_tree_tests():
    arrays = synthetic(29, 3, 5, 3, 5)
    X = rows(30, 12, 9)
    phi, _ = check(dict(arrays, n_features=9), X, "9 columns, 5 tested")
    assert same_bits(phi[:, 5:, :], np.zeros((12, 4, 3)))


@pytest.mark.parametrize("K,F,n", [(2, 4, 20), (64, 6, 9), (64, 48, 40)])
def test_class_counts(K, F, n):
    """K = 2; K = 64 with the accumulators of 21 rows in 64 KB of LDS; K = 64 x 48 columns, where a row's accumulators take
    24 KB, fewer than four rows fit and the workgroups (32 rows each, so two of them) add into the output itself."""
    arrays = synthetic(31 + K, 3, min(F, 6), K, 5)
    check(dict(arrays, n_features=F), rows(32, n, F), f"K = {K}, F = {F}")


def test_refusals(cases):
    from obia_amd.classify import forest_shap
    with pytest.raises(NotImplementedError, match="32 distinct features"):
        forest_shap(S.forest_of(S.comb_forest(33)), np.zeros((2, 33), np.float32))
    with pytest.raises(NotImplementedError, match="64 classes"):
        forest_shap(S.forest_of(synthetic(1, 2, 3, 65, 2)), rows(1, 4, 3))
    with pytest.raises(ValueError, match="Forest.from_sklearn"):
        forest_shap(fr.forest_of(fr.load_case("b")), cases["b"]["X32"])


def test_abi_refuses_bad_covers_and_bad_nodes():
    """Passed straight to obia_forest_shap_dev (the Forest constructor would not let the nodes through): a zero cover, a NaN
    cover, a child or a feature outside its range are OBIA_E_INVALID, and nothing is followed out of the arrays."""
    import torch
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    d = synthetic(2, 2, 3, 4, 3)
    x = torch.as_tensor(rows(3, 10, 3, nan=0)).cuda()

    def call(arr):
        t = {k: torch.as_tensor(np.ascontiguousarray(arr[k])).cuda() for k in S.ARRAYS + ("cover",)}
        off = np.ascontiguousarray(arr["tree_offset"], np.int64)
        fs = _lib.Forest(*(t[k].data_ptr() for k in S.ARRAYS[:6]), off.ctypes.data, t["value"].data_ptr(), len(arr["threshold"]), len(off), 4)
        phi = torch.zeros((10, 3, 4), dtype=torch.float64, device="cuda")
        base = torch.zeros((4,), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        return lib.obia_forest_shap_dev(ctx.handle, x.data_ptr(), 10, 3, ctypes.byref(fs), t["cover"].data_ptr(), phi.data_ptr(), base.data_ptr())

    def changed(key, index, v):
        a = d[key].copy()
        a[index] = v
        return dict(d, **{key: a})

    assert call(d) == _lib.OBIA_OK
    last = len(d["cover"]) - 1
    assert call(changed("cover", last, 0.0)) == _lib.E_INVALID and "cover" in _lib.last_error()
    assert call(changed("cover", 0, float("nan"))) == _lib.E_INVALID and "cover" in _lib.last_error()
    assert call(changed("cover", 1, float("inf"))) == _lib.E_INVALID
    assert call(changed("right", 0, 10 ** 6)) == _lib.E_INVALID and "out of range" in _lib.last_error()
    assert call(changed("left", 0, 10 ** 6)) == _lib.E_INVALID
    assert call(changed("feature", 0, 3)) == _lib.E_INVALID
    assert call(changed("right", 0, 0)) == _lib.E_INVALID            # the root as its own child: a cycle
    assert call(d) == _lib.OBIA_OK


def test_predict_segments_fills_shap_values(cases):
    import pandas as pd
    from obia_amd.classify import forest_shap, predict_segments, standard_scale
    c = cases["c"]
    table = fr.load_case("c")["table"][:50]
    frame = pd.DataFrame(table, columns=[f"f{i}" for i in range(table.shape[1])])
    frame["segment_id"] = np.arange(len(frame))
    res = predict_segments(c["forest"], frame.copy(), compute_shap=True)
    X32, _, _ = standard_scale(table)
    phi, base = forest_shap(c["forest"], X32)
    assert res.shap_values.shape == (50, table.shape[1], len(c["classes_"]))
    assert same_bits(res.shap_values, phi) and same_bits(res.shap_base_values, base)
    plain = predict_segments(c["forest"], frame.copy())
    assert plain.shap_values is None and plain.shap_base_values is None
    assert np.array_equal(np.asarray(plain.classified["predicted_class"]), np.asarray(res.classified["predicted_class"]))
