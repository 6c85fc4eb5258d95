"""Restatement of ``forest_shap`` (path-dependent TreeSHAP in its per-path form) with the number type as a parameter (test
infrastructure; NumPy and the standard library).

The contract.  A row follows node j to the left iff ``float64(float32(x[feature_j])) <= threshold_j``, a NaN
iff ``missing_go_to_left[j]`` -- the walk of ``forest_predict``.  ``v_t(S)`` at a leaf is ``value[leaf]``, at a node whose
feature is in S the value of the child the row follows, otherwise ``z_left v(left) + z_right v(right)`` with
``z_child = cover[child] / cover[node]``.  ``phi[row, f, :]`` is the Shapley value of feature f under ``(1 / T) sum_t v_t``,
``base = v(empty set)``.

Per path (root to leaf) the splits of one feature are merged into one ELEMENT: ``zero`` = the product of its splits' z_child,
taken from the leaf upwards; ``one`` = 1 iff the row follows the path at every one of these splits, which for a value that is
not NaN is ``not (x <= lo) and x <= hi`` (lo: the largest threshold of the right turns, NaN when there is none; hi: the
smallest of the left turns, +inf when there is none) and for a NaN one stored bit.  The elements are numbered in the order the
walk from the leaf to the root meets them first.  Then, with ``rat(a, b) = a (1 / b)`` (the reciprocal rounded, then the
product) and w[0] = 1:

    EXTEND, s = 1 .. m:     w'[e] = (zero_s w[e]) rat(s - e, s + 1) + (one_s w[e - 1]) rat(e, s + 1)        e = 0 .. s
    UNWIND of element e:    one_e = 1:  n = w[m];  j = m - 1 .. 0:  t = n rat(m + 1, j + 1);  total += t;
                                        n = w[j] - (t zero_e) rat(m - j, m + 1)
                            one_e = 0:  total = (sum over j = m - 1 .. 0 of w[j] rat(m + 1, m - j)) / zero_e
    phi[row, feature_e, :] += ((total (one_e - zero_e)) / T) value[leaf]
    base += ((zero_1 zero_2 ... zero_m) value[leaf]) / T

Paths are taken tree by tree, within a tree in ascending node index of the leaf.  With ``num=fractions.Fraction`` every step is
exact (float64 covers, thresholds and leaf values are rationals); with ``num=float`` every product, sum and quotient rounds on
its own, in the order written above -- the order csrc/shap.hip keeps.
"""
import itertools
import math
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["a", "b", "c", "d", "e", "comb16", "comb32"]         # tests/golden/shap/<case>.npz (gen_goldens_shap.py)
FOREST_CASES = ["a", "b", "c", "d", "e"]                      # ... of these, the ones built on tests/golden/forest/<case>.npz
ARRAYS = ("threshold", "feature", "left", "right", "missing_go_to_left", "tree_offset", "value")
MAX_PATH_FEATURES = 32


def load_case(name):
    with np.load(os.path.join(GOLDEN, "shap", f"{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def forest_of(case):
    """The obia_amd.classify.Forest (with cover) of a fixture or of a dict of flat arrays."""
    from obia_amd.classify import Forest
    return Forest(classes_=case["classes_"], n_features=int(case["n_features"]), cover=case["cover"], **{k: case[k] for k in ARRAYS})


def _get(forest, name):
    return np.asarray(forest[name] if isinstance(forest, dict) or hasattr(forest, "files") else getattr(forest, name))


def paths(forest):
    """Every root-to-leaf path, trees ascending and leaves in ascending node index: a list of dicts ``tree``, ``leaf`` (global
    node index) and ``elems``, one ``(feature, lo, hi, nan_follows, [(cover[child], cover[node]), ...])`` per distinct feature
    in the order the walk from the leaf upwards meets it first, the cover pairs in that order too."""
    thr, feat = _get(forest, "threshold"), _get(forest, "feature")
    left, right = _get(forest, "left").astype(np.int64), _get(forest, "right").astype(np.int64)
    mgl, off, cover = _get(forest, "missing_go_to_left"), _get(forest, "tree_offset").astype(np.int64), _get(forest, "cover")
    out = []
    for t, base in enumerate(off):
        found = []
        stack = [(int(base), [])]                      # (node, chain of (parent, went_left, node) from the root)
        while stack:
            node, chain = stack.pop()
            if left[node] < 0:
                found.append((node, chain))
                continue
            for child, is_left in ((base + right[node], False), (base + left[node], True)):
                stack.append((int(child), chain + [(node, is_left, int(child))]))
        for leaf, chain in sorted(found, key=lambda p: p[0]):
            elems, index = [], {}
            for parent, is_left, child in reversed(chain):
                f = int(feat[parent])
                if f not in index:
                    index[f] = len(elems)
                    elems.append([f, float("nan"), float("inf"), True, []])
                e = elems[index[f]]
                th = float(thr[parent])
                if is_left:
                    e[2] = th if (th != th or th < e[2]) and e[2] == e[2] else e[2]      # a NaN threshold is never followed
                elif th == th and not (th <= e[1]):
                    e[1] = th
                e[3] = e[3] and (bool(mgl[parent]) == is_left)
                e[4].append((float(cover[child]), float(cover[parent])))
            out.append({"tree": t, "leaf": leaf, "elems": [tuple(e) for e in elems]})
    return out


def follows(elem, x32):
    """(N,) bool: the rows of the float32 table that follow the path at every split of this element's feature."""
    _, lo, hi, nan_follows, _ = elem
    v = x32[:, elem[0]].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), nan_follows, ~(v <= lo) & (v <= hi))


def shap_values(forest, X, num=float, order=None):
    """``(phi (N, F, K), base (K,))`` by the per-path algorithm of the module docstring.  ``num=float``: float64 arrays, every
    operation rounded on its own; ``num=Fraction``: object arrays of exact rationals.  ``order``: None for the natural element
    order, or a seed -- every path's elements are then permuted (the exact result does not change, the rounding does)."""
    x32 = np.asarray(X).astype(np.float32)
    N, F = x32.shape
    value = _get(forest, "value")
    K, T = value.shape[1], len(_get(forest, "tree_offset"))
    exact = num is not float
    dt = object if exact else np.float64
    lift = (lambda a: np.array([num(float(v)) for v in np.ravel(a)], dtype=object).reshape(np.shape(a))) if exact else \
        (lambda a: np.asarray(a, np.float64))
    inv = [num(0)] + [num(1) / num(b) for b in range(1, MAX_PATH_FEATURES + 2)]
    rat = [[num(a) * inv[b] for b in range(MAX_PATH_FEATURES + 2)] for a in range(MAX_PATH_FEATURES + 2)]
    zero_row = lift(np.zeros(N))
    phi = np.empty((N, F, K), dt)
    phi[...] = num(0)
    base = lift(np.zeros(K))
    Tn = num(T)
    rs = None if order is None else np.random.RandomState(order)
    for p in paths(forest):
        elems = list(p["elems"])
        m = len(elems)
        if m > MAX_PATH_FEATURES:
            raise NotImplementedError(f"a path tests {m} distinct features")
        if rs is not None:
            elems = [elems[i] for i in rs.permutation(m)]
        leaf_value = lift(value[p["leaf"]])
        zero, one = [None], [None]
        for e in elems:
            z = None
            for child_cover, node_cover in e[4]:
                q = num(child_cover) / num(node_cover)
                z = q if z is None else z * q
            zero.append(z)
            one.append(lift(follows(e, x32).astype(np.float64)))
        zprod = num(1)
        for s in range(1, m + 1):
            zprod = zero[s] if s == 1 else zprod * zero[s]
        base = base + (zprod * leaf_value) / Tn
        if m == 0:
            continue
        w = [lift(np.ones(N))] + [zero_row] * m
        for s in range(1, m + 1):
            new = list(w)
            for e in range(s + 1):
                a = (zero[s] * w[e]) * rat[s - e][s + 1]
                b = (one[s] * w[e - 1]) * rat[e][s + 1] if e > 0 else zero_row
                new[e] = a + b
            w = new
        for e in range(1, m + 1):
            nop, tot1, tot0 = w[m], zero_row, zero_row
            for j in range(m - 1, -1, -1):
                t = nop * rat[m + 1][j + 1]
                tot1 = tot1 + t
                nop = w[j] - (t * zero[e]) * rat[m - j][m + 1]
                tot0 = tot0 + w[j] * rat[m + 1][m - j]
            total = np.where(one[e] != 0, tot1, tot0 / zero[e])
            scale = (total * (one[e] - zero[e])) / Tn
            f = elems[e - 1][0]
            phi[:, f, :] = phi[:, f, :] + scale[:, None] * leaf_value[None, :]
    return phi, base


def to_float(a):
    """Exact rationals rounded to float64 (``float(Fraction)`` rounds correctly)."""
    return np.array([float(v) for v in np.ravel(a)], np.float64).reshape(np.shape(a))


def brute_force(forest, x):
    """``(phi (F, K), base (K,))`` of ONE row in Fractions from the definition: per tree the Shapley sum over all subsets of the
    features the tree tests, ``v_t(S)`` by the recursion of the contract; then the mean over trees."""
    thr, feat = _get(forest, "threshold"), _get(forest, "feature")
    left, right = _get(forest, "left").astype(np.int64), _get(forest, "right").astype(np.int64)
    mgl, off, cover = _get(forest, "missing_go_to_left"), _get(forest, "tree_offset").astype(np.int64), _get(forest, "cover")
    value = _get(forest, "value")
    x32 = np.asarray(x).astype(np.float32).ravel()
    F, K, T = len(x32), value.shape[1], len(off)
    n = len(thr)
    phi = [[Fraction(0)] * K for _ in range(F)]
    base = [Fraction(0)] * K
    for t, b in enumerate(off):
        end = int(off[t + 1]) if t + 1 < T else n
        used = sorted({int(feat[i]) for i in range(int(b), end) if left[i] >= 0})

        def v(node, S):
            if left[node] < 0:
                return [Fraction(float(u)) for u in value[node]]
            f = int(feat[node])
            l, r = int(b + left[node]), int(b + right[node])
            if f in S:
                xv = float(x32[f])
                go_left = bool(mgl[node]) if xv != xv else xv <= float(thr[node])
                return v(l if go_left else r, S)
            zl = Fraction(float(cover[l])) / Fraction(float(cover[node]))
            zr = Fraction(float(cover[r])) / Fraction(float(cover[node]))
            return [zl * p + zr * q for p, q in zip(v(l, S), v(r, S))]

        vs = {S: v(int(b), frozenset(S)) for k in range(len(used) + 1) for S in itertools.combinations(used, k)}
        nu = len(used)
        for k in range(K):
            base[k] += vs[()][k]
        for f in used:
            rest = [u for u in used if u != f]
            for size in range(nu):
                wgt = Fraction(math.factorial(size) * math.factorial(nu - size - 1), math.factorial(nu))
                for S in itertools.combinations(rest, size):
                    with_f = vs[tuple(sorted(S + (f,)))]
                    for k in range(K):
                        phi[f][k] += wgt * (with_f[k] - vs[S][k])
    phi = np.array([[p / T for p in row] for row in phi], dtype=object).reshape(F, K)
    return phi, np.array([p / T for p in base], dtype=object)


def comb_forest(n_chain, n_classes=3, repeat_splits=40, repeat_features=6, seed=0):
    """Two synthetic trees as a dict of flat arrays with ``cover``.  Tree 0: a right-leaning chain of ``n_chain`` splits on the
    features 0 .. n_chain - 1 (the left child of every split is a leaf), so the deepest path tests ``n_chain`` distinct
    features.  Tree 1: a chain of ``repeat_splits`` splits over ``repeat_features`` features, turning left or right at random.
    Leaf covers are integers and an inner node's cover is the sum of its children's."""
    rs = np.random.RandomState(seed)
    parts = {k: [] for k in ARRAYS if k != "tree_offset"}
    parts["cover"] = []
    off, total = [], 0
    for n_split, feats, right_only in ((n_chain, np.arange(n_chain), True),
                                       (repeat_splits, rs.randint(0, repeat_features, repeat_splits), False)):
        n = 2 * n_split + 1
        # node 2 i is split i, node 2 i + 1 its leaf child; the chain goes on at node 2 i + 2; the last node is a leaf
        thr, ft, lf, rt = np.full(n, -2.0), np.full(n, -2, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        go_right = np.ones(n_split, bool) if right_only else rs.rand(n_split) < 0.5
        for i in range(n_split):
            thr[2 * i] = np.round(rs.normal(0, 1) * 8) / 8 - (1.5 if right_only else 0.0)
            ft[2 * i] = feats[i]
            lf[2 * i], rt[2 * i] = (2 * i + 1, 2 * i + 2) if go_right[i] else (2 * i + 2, 2 * i + 1)
        cov = np.zeros(n)
        leaf = lf < 0
        cov[leaf] = rs.randint(1, 9, int(leaf.sum()))
        for i in range(n_split - 1, -1, -1):
            cov[2 * i] = cov[lf[2 * i]] + cov[rt[2 * i]]
        v = rs.randint(0, 5, (n, n_classes)).astype(np.float64) + 1.0
        for k, a in (("threshold", thr), ("feature", ft), ("left", lf), ("right", rt),
                     ("missing_go_to_left", rs.randint(0, 2, n).astype(np.uint8)), ("value", v / v.sum(1, keepdims=True)), ("cover", cov)):
            parts[k].append(a)
        off.append(total)
        total += n
    out = {k: np.concatenate(v) for k, v in parts.items()}
    out.update(tree_offset=np.asarray(off, np.int64), classes_=np.arange(n_classes), n_features=np.int64(max(n_chain, repeat_features)))
    return out


def with_cover(forest_dict, rs):
    """A dict of flat arrays (``forest_restatement.random_forest``) plus integer covers: leaves random, inner nodes the sum."""
    left, right, off = forest_dict["left"], forest_dict["right"], forest_dict["tree_offset"]
    n = len(left)
    size = np.diff(np.r_[off, n])
    base = np.repeat(off, size)
    cov = np.where(left < 0, rs.randint(1, 9, n), 0).astype(np.float64)
    for i in range(n - 1, -1, -1):                      # children are allocated after their parent
        if left[i] >= 0:
            cov[i] = cov[base[i] + left[i]] + cov[base[i] + right[i]]
    return dict(forest_dict, cover=cov)
