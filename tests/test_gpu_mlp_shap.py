"""Exact Shapley values of an MLP on the GPU (csrc/mlp_shap.hip): ``mlp_coalition_values`` against ``mlp_predict`` bit for bit and
against the longdouble evaluation, ``shapley_combine`` against exact rational arithmetic, ``mlp_shap`` end to end on the fixtures
of tests/golden/gen_goldens_mlp_shap.py, and the properties DESIGN.md 3.5l states.  E is the pooled ``e_ref`` of the mlp_predict
fixtures, ``e_comb`` the distance of the float64 subset formula from the exact one on the same inputs."""
from fractions import Fraction

import numpy as np
import pytest

from tests import mlp_restatement as mr
from tests import mlp_shap_restatement as S

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cases():
    """Every fixture once with its MLP and the GPU's answers.  Nothing in here is modified by a test."""
    from obia_amd.classify import mlp_coalition_values, mlp_shap
    out = {}
    for name in S.CASES:
        c = S.load_case(name)
        mlp = mr.mlp_of(c)
        phi, base = mlp_shap(mlp, c["X"], c["background"])
        values = mlp_coalition_values(mlp, c["X"], c["background"], S.all_masks(c["X"].shape[1]))
        out[name] = dict(c, mlp=mlp, phi=phi, base=base, values=values)
    return out


def reference_values(mlp, X, background, masks):
    """The ordered mean, in NumPy, of mlp_predict's proba on the hybrid rows built in NumPy."""
    from obia_amd.classify import mlp_predict
    h = np.stack([S.hybrid_rows(x, background, masks) for x in X])             # (N, M, B, F)
    N, M, B, F = h.shape
    _, _, proba = mlp_predict(mlp, h.reshape(N * M * B, F))
    return S.ordered_mean(proba.reshape(N, M, B, -1))


def net(seed, layer_sizes, hidden="relu", out="softmax"):
    return mr.mlp_of(mr.random_mlp(np.random.RandomState(seed), layer_sizes, hidden, out))


# width -> (rows of the background a workgroup takes at a time, hidden activation, classes)
WIDTHS = {8: (64, "relu", 3), 100: (32, "tanh", 6), 512: (4, "logistic", 3)}
PIECES = [(w, b) for w in WIDTHS for b in ("1", "R-1", "R", "R+1", "2R+3")]


@pytest.mark.parametrize("width,b", PIECES)
def test_coalition_values_equal_the_mean_of_mlp_predict_bit_for_bit(width, b):
    from obia_amd.classify import _mlp_plan, mlp_coalition_values
    R, hidden, K = WIDTHS[width]
    ls = [3, width, K]
    assert _mlp_plan(ls)[0] == R
    B = {"1": 1, "R-1": R - 1, "R": R, "R+1": R + 1, "2R+3": 2 * R + 3}[b]
    N = 3 if b in ("R-1", "R+1") else 1
    mlp = net(width + B, ls, hidden)
    rs = np.random.RandomState(B)
    X, bg = rs.normal(0, 1.5, (N, 3)), rs.normal(0, 1.5, (B, 3))
    masks = S.all_masks(3)
    got = mlp_coalition_values(mlp, X, bg, masks)
    assert got.dtype == np.float64 and got.shape == (N, 8, K)
    assert same_bits(got, reference_values(mlp, X, bg, masks))


@pytest.mark.parametrize("ls,hidden,out,B", [([4, 8, 1], "identity", "logistic", 65), ([4, 100, 50, 30, 6], "relu", "softmax", 33),
                                             ([2, 3], "relu", "softmax", 70), ([2, 1], "relu", "logistic", 5)])
def test_other_outputs_and_depths_bit_for_bit(ls, hidden, out, B):
    """The logistic output, the identity, the author's depth, no hidden layer at all."""
    from obia_amd.classify import mlp_coalition_values
    mlp = net(B, ls, hidden, out)
    rs = np.random.RandomState(B + 1)
    X, bg = rs.normal(0, 1.5, (3, ls[0])), rs.normal(0, 1.5, (B, ls[0]))
    masks = S.all_masks(ls[0])
    got = mlp_coalition_values(mlp, X, bg, masks.astype(np.uint8))
    assert got.shape == (3, len(masks), mlp.n_classes)
    assert same_bits(got, reference_values(mlp, X, bg, masks))


def test_sixty_features_arrive_in_two_pieces_under_explicit_masks():
    from obia_amd.classify import _mlp_plan, mlp_coalition_values
    ls = [60, 100, 6]
    assert _mlp_plan(ls) == (32, 54)
    mlp = net(60, ls, "relu")
    rs = np.random.RandomState(61)
    X, bg = rs.normal(0, 1.5, (3, 60)), rs.normal(0, 1.5, (33, 60))
    masks = np.stack([np.zeros(60, bool), np.ones(60, bool), rs.rand(60) < 0.5, np.arange(60) >= 54, np.arange(60) % 2 == 0])
    got = mlp_coalition_values(mlp, X, bg, masks)
    assert same_bits(got, reference_values(mlp, X, bg, masks))
    from obia_amd.classify import mlp_predict
    _, _, proba = mlp_predict(mlp, X)
    B = 33
    full = np.zeros_like(proba)
    for _ in range(B):
        full = full + proba
    assert same_bits(got[:, 1, :], full / B)                                     # the full mask: B times the row's own proba


@pytest.mark.parametrize("name", S.CASES)
def test_coalition_values_within_8_E_of_longdouble(cases, name):
    c = cases[name]
    E = mr.pooled_e_ref()
    err = float(np.abs(c["values"] - c["values_ld"]).max())
    print(f"{name}: max|values - values_ld| = {err:.3e} = {err / E:.2f} E, bar 8 E = {8 * E:.3e}")
    assert c["values"].shape == c["values_ld"].shape and err <= 8 * E


@pytest.mark.parametrize("F,K", [(1, 1), (1, 3), (2, 1), (2, 3), (5, 1), (5, 3), (10, 1), (10, 3)])
def test_shapley_combine_against_fractions(F, K):
    from obia_amd.classify import shapley_combine
    values = np.random.RandomState(10 * F + K).rand(3, 1 << F, K)
    exact = S.to_float(S.shapley(values, num=Fraction))
    e_comb = max(2.0 ** -52, float(np.abs(S.shapley(values, num=float) - exact).max()))
    phi = shapley_combine(values)
    err = float(np.abs(phi - exact).max())
    print(f"F = {F}, K = {K}: max|phi - exact| = {err:.3e}, e_comb {e_comb:.3e}, bar {8 * e_comb:.3e}")
    assert phi.dtype == np.float64 and phi.shape == (3, F, K) and err <= 8 * e_comb


def test_shapley_combine_at_sixteen_features():
    from obia_amd.classify import shapley_combine
    values = np.random.RandomState(16).rand(1, 1 << 16, 2)
    feats = [0, 7, 15]
    exact = S.to_float(S.shapley(values, num=Fraction, features=feats))
    e_comb = max(2.0 ** -52, float(np.abs(S.shapley(values, num=float, features=feats) - exact).max()))
    phi = shapley_combine(values)
    err = float(np.abs(phi[:, feats, :] - exact).max())
    print(f"F = 16: max|phi - exact| on features 0, 7, 15 = {err:.3e}, e_comb {e_comb:.3e}, bar {8 * e_comb:.3e}")
    assert phi.shape == (1, 16, 2) and err <= 8 * e_comb


@pytest.mark.parametrize("name", S.CASES)
def test_mlp_shap_end_to_end(cases, name):
    """|phi - phi_exact| <= 16 E + 8 e_comb: the size weights of a feature sum to 1 and every difference carries two values, each
    within 8 E; the subset formula adds 8 e_comb.  |base - base_exact| <= 8 E.  |sum_f phi + base - proba| <= (F + 1) (16 E +
    8 e_comb) + B 2^-53: F + 1 terms whose exact sum is the full coalition's value -- the ordered mean of B copies of proba, which
    is within B 2^-53 of proba."""
    from obia_amd.classify import mlp_predict
    c = cases[name]
    E, e_comb = mr.pooled_e_ref(), float(c["e_comb"])
    N, F = c["X"].shape
    B = c["background"].shape[0]
    assert c["phi"].dtype == np.float64 and c["phi"].shape == c["phi_exact"].shape and c["base"].shape == c["base_exact"].shape
    bar = 16 * E + 8 * e_comb
    err_phi, err_base = float(np.abs(c["phi"] - c["phi_exact"]).max()), float(np.abs(c["base"] - c["base_exact"]).max())
    _, _, proba = mlp_predict(c["mlp"], c["X"])
    gap = float(np.abs(c["phi"].sum(axis=1) + c["base"][None, :] - proba).max())
    gap_bar = (F + 1) * bar + B * 2.0 ** -53
    print(f"{name}: phi {err_phi:.3e} = {err_phi / bar:.3f} of its bar {bar:.3e}; base {err_base:.3e} = {err_base / (8 * E):.3f} of 8 E; "
          f"additivity gap {gap:.3e} = {gap / gap_bar:.3f} of its bar {gap_bar:.3e}")
    assert err_phi <= bar and err_base <= 8 * E and gap <= gap_bar
    assert same_bits(c["base"], c["values"][0, 0]) and same_bits(c["values"][:, 0], np.broadcast_to(c["base"], (N, len(c["base"]))))


def test_a_column_equal_to_every_background_row_gets_exactly_zero(cases):
    c = cases["r1"]                                    # row 0 equals the background in column 2
    assert same_bits(c["phi"][0, 2], np.zeros(3)) and (c["phi"][1:, 2] != 0).all()


def test_one_feature_is_the_full_minus_the_empty_coalition():
    from obia_amd.classify import mlp_coalition_values, mlp_shap
    mlp = net(1, [1, 8, 3], "tanh")
    rs = np.random.RandomState(2)
    X, bg = rs.normal(0, 1.5, (4, 1)), rs.normal(0, 1.5, (9, 1))
    phi, base = mlp_shap(mlp, X, bg)
    v = mlp_coalition_values(mlp, X, bg, S.all_masks(1))
    assert same_bits(phi[:, 0, :], v[:, 1, :] - v[:, 0, :]) and same_bits(base, v[0, 0])


def test_repeatable_and_independent_of_the_other_rows_and_of_the_pieces(cases, monkeypatch):
    import importlib
    import torch
    C = importlib.import_module("obia_amd.classify")
    c = cases["r2"]
    phi, base = C.mlp_shap(c["mlp"], c["X"], c["background"])
    assert same_bits(phi, c["phi"]) and same_bits(base, c["base"])
    part, base_part = C.mlp_shap(c["mlp"], c["X"][3:5], c["background"])
    assert same_bits(part, c["phi"][3:5]) and same_bits(base_part, c["base"])
    monkeypatch.setattr(C, "_SHAP_VALUES_BYTES", 8)                              # one row per piece
    one, base_one = C.mlp_shap(c["mlp"], c["X"], c["background"])
    assert same_bits(one, c["phi"]) and same_bits(base_one, c["base"])
    monkeypatch.undo()
    tphi, tbase = C.mlp_shap(c["mlp"], torch.as_tensor(c["X"]).cuda(), torch.as_tensor(c["background"]).cuda())
    assert tphi.is_cuda and tbase.is_cuda and tphi.dtype == torch.float64
    assert same_bits(tphi.cpu().numpy(), c["phi"]) and same_bits(tbase.cpu().numpy(), c["base"])
    tv = C.mlp_coalition_values(c["mlp"], torch.as_tensor(c["X"]).cuda(), c["background"], torch.as_tensor(S.all_masks(3)).cuda())
    assert tv.is_cuda and same_bits(tv.cpu().numpy(), c["values"])
    tc = C.shapley_combine(tv)
    assert tc.is_cuda and same_bits(tc.cpu().numpy(), c["phi"]) and same_bits(C.shapley_combine(c["values"]), c["phi"])


def test_nan_and_infinity_are_refused(cases):
    from obia_amd.classify import mlp_coalition_values, mlp_shap
    c = cases["r2"]
    X, bg = c["X"].copy(), c["background"].copy()
    X[1, 2] = np.nan
    bg[32, 0] = np.inf
    with pytest.raises(ValueError, match="Input X contains NaN or infinity"):
        mlp_shap(c["mlp"], X, c["background"])
    with pytest.raises(ValueError, match="Input background contains NaN or infinity"):
        mlp_shap(c["mlp"], c["X"], bg)
    with pytest.raises(ValueError, match="Input X contains NaN"):
        mlp_coalition_values(c["mlp"], X, c["background"], S.all_masks(3)[:1])       # the empty mask never reads X: refused all the same


def test_predict_segments_fills_shap_values_for_an_mlp(cases):
    import pandas as pd
    from obia_amd.classify import mlp_shap, predict_segments, standard_scale
    c = cases["r3"]
    table = np.random.RandomState(3).normal(5, 2, (6, 7))
    frame = pd.DataFrame(table, columns=[f"f{i}" for i in range(7)])
    frame["segment_id"] = np.arange(len(frame))
    res = predict_segments(c["mlp"], frame.copy(), compute_shap=True, shap_background=c["background"])
    X, _, _ = standard_scale(table, dtype=np.float64)
    phi, base = mlp_shap(c["mlp"], X, c["background"])
    assert res.shap_values.shape == (6, 7, 4)
    assert same_bits(res.shap_values, phi) and same_bits(res.shap_base_values, base)
    plain = predict_segments(c["mlp"], frame.copy())
    assert plain.shap_values is None and np.array_equal(np.asarray(plain.classified["predicted_class"]), np.asarray(res.classified["predicted_class"]))
