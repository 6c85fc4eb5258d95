"""NumPy / Fraction restatement of ``mlp_coalition_values`` / ``shapley_combine`` / ``mlp_shap`` (test
infrastructure, nothing here touches a GPU).

The game of a row x against a background table: ``v(S) = mean over b of proba(x on the features in S, background[b] elsewhere)``.
``coalition_values`` evaluates it in the contract's order -- the background rows added in ascending order from 0.0, one division by
B -- in float64 on ``mlp_restatement.predict_proba``, or in ``np.longdouble`` on a longdouble forward pass (rounded to float64 at
the very end).  ``shapley`` turns the values of all 2^F coalitions (binary order: bit f of m = feature f is in the coalition) into
Shapley values by the subset formula, in float64 in the kernel's order or exactly in ``fractions.Fraction``;
``shapley_by_permutations`` is the definition itself -- the mean marginal contribution over all F! orders -- for small F.
"""
import itertools
import math
import os
from fractions import Fraction

import numpy as np

from tests import mlp_restatement as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_shap")
CASES = ["author", "r1", "r2", "r3"]              # tests/golden/mlp_shap/<case>.npz (gen_goldens_mlp_shap.py)


def load_case(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def all_masks(F):
    """(2^F, F) bool: row m holds feature f iff bit f of m is set."""
    return ((np.arange(1 << F)[:, None] >> np.arange(F)[None, :]) & 1).astype(bool)


def hybrid_rows(x, background, masks):
    """(M, B, F): ``x[f]`` where ``masks[m, f]``, ``background[b, f]`` elsewhere."""
    x, background, masks = np.asarray(x, np.float64), np.asarray(background, np.float64), np.asarray(masks) != 0
    return np.where(masks[:, None, :], x[None, None, :], background[None, :, :])


def ordered_mean(p):
    """p (..., B, K) -> (..., K): ((0.0 + p_0) + p_1) + ... + p_{B-1}, then one division by B, in p's own number type."""
    acc = np.zeros(p.shape[:-2] + p.shape[-1:], p.dtype)
    for b in range(p.shape[-2]):
        acc = acc + p[..., b, :]
    return acc / p.dtype.type(p.shape[-2])


def proba_longdouble(mlp, X):
    """The forward pass in np.longdouble, NOT rounded (gen_goldens_mlp.forward_longdouble on the flat arrays)."""
    L = np.longdouble
    a = np.asarray(X, np.float64).astype(L)
    hidden = str(mr._get(mlp, "hidden_activation"))
    act = {"identity": lambda z: z, "relu": lambda z: np.maximum(z, L(0)), "tanh": np.tanh,
           "logistic": lambda z: L(1) / (L(1) + np.exp(-z))}[hidden]
    ly = mr.layers(mlp)
    for i, (W, b) in enumerate(ly):
        a = a @ W.astype(L) + b.astype(L)
        if i + 1 < len(ly):
            a = act(a)
    if str(mr._get(mlp, "out_activation")) == "logistic":
        p = L(1) / (L(1) + np.exp(-a[:, 0]))
        return np.stack([L(1) - p, p], axis=1)
    e = np.exp(a - a.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def coalition_values(mlp, X, background, masks, num=float):
    """(N, M, K) float64.  ``num=float``: the contract's arithmetic; ``num=np.longdouble``: everything in longdouble, one rounding."""
    X, background = np.asarray(X, np.float64), np.asarray(background, np.float64)
    out = []
    for x in X:
        h = hybrid_rows(x, background, masks)
        M, B, F = h.shape
        p = (proba_longdouble if num is np.longdouble else mr.predict_proba)(mlp, h.reshape(M * B, F))
        out.append(ordered_mean(p.reshape(M, B, -1)).astype(np.float64))
    return np.stack(out)


def size_weights(F, num=float):
    w = [Fraction(math.factorial(s) * math.factorial(F - 1 - s), math.factorial(F)) for s in range(F)]
    return w if num is Fraction else np.array([float(v) for v in w], np.float64)


def shapley(values, num=float, features=None):
    """values (N, 2^F, K) float64 (or Fractions, with ``num=Fraction``) -> phi (N, len(features), K) (all F features by default).
    ``num=float``: the kernel's order -- the coalitions without bit f in ascending m from 0.0,
    ``acc = acc + w[popcount(m)] * (v[m | 1 << f] - v[m])`` with the correctly rounded weights.  ``num=Fraction``: the same sum exactly (an object array of Fractions)."""
    values = np.asarray(values)
    if values.dtype != object:
        values = values.astype(np.float64)
    N, M, K = values.shape
    F = M.bit_length() - 1
    assert M == 1 << F and F >= 1 and (num is Fraction or values.dtype != object)
    features = list(range(F)) if features is None else list(features)
    w = size_weights(F, num)
    without = np.arange(M)
    if num is Fraction:
        v = values if values.dtype == object else np.array([Fraction(float(t)) for t in values.ravel()], object).reshape(N, M, K)
        phi = np.empty((N, len(features), K), object)
        for i, f in enumerate(features):
            ms = without[(without >> f) & 1 == 0]
            wm = np.array([w[bin(m).count("1")] for m in ms], object)
            phi[:, i, :] = ((v[:, ms | (1 << f), :] - v[:, ms, :]) * wm[None, :, None]).sum(axis=1)
        return phi
    phi = np.zeros((N, len(features), K), np.float64)
    for i, f in enumerate(features):
        acc = np.zeros((N, K), np.float64)
        for m in without[(without >> f) & 1 == 0].tolist():
            acc = acc + w[bin(m).count("1")] * (values[:, m | (1 << f), :] - values[:, m, :])
        phi[:, i, :] = acc
    return phi


def shapley_by_permutations(values_row):
    """values_row (2^F, K) of Fractions (or floats, taken exactly) -> (F, K) Fractions: the mean over all F! orders of the change of
    the value when the feature joins those before it.  F <= 5."""
    M, K = values_row.shape
    F = M.bit_length() - 1
    assert M == 1 << F and 1 <= F <= 5
    v = [[Fraction(t) if isinstance(t, Fraction) else Fraction(float(t)) for t in row] for row in values_row]
    phi = [[Fraction(0)] * K for _ in range(F)]
    for order in itertools.permutations(range(F)):
        m = 0
        for f in order:
            for k in range(K):
                phi[f][k] += v[m | (1 << f)][k] - v[m][k]
            m |= 1 << f
    n = math.factorial(F)
    return np.array([[t / n for t in row] for row in phi], object)


def to_float(a):
    """An array of Fractions rounded to float64 (``float(Fraction)`` rounds correctly)."""
    return np.array([float(t) for t in np.asarray(a, object).ravel()], np.float64).reshape(np.shape(a))
