"""Host-side mirror of ``obia.classification.classify`` (classify.py:68-175) with the prediction half on the GPU.

Training stays scikit-learn on the host: it sees a few hundred labelled rows and is the reference's own estimator.  What touches
the whole segment table runs on the device (libobia_hip.so, csrc/classify.hip):

    standard_scale  ``StandardScaler().fit(x).transform(x)`` of classify.py:126-129 plus the forest's cast to float32
                    (``dtype=np.float64``: without the cast, what ``MLPClassifier`` is handed)
    forest_predict  the ``segments.iterrows()`` loop of :135-158 -- ``predict_proba`` / ``predict`` row by row, the class filter
                    and the margin -- as one tree walk per (row, tree) for all rows at once
    mlp_predict     the same loop for a fitted ``MLPClassifier``: the forward pass of all rows, class filter and margin in one
                    kernel (csrc/mlp.hip)
    forest_shap     ``shap.TreeExplainer(classifier).shap_values(x)`` of :113-118 for the whole table: path-dependent TreeSHAP,
                    one (row, root-to-leaf path) pair at a time (csrc/shap.hip)
    mlp_shap        ``shap.KernelExplainer(classifier.predict_proba, background).shap_values(x)`` of :108-115 for a table of at
                    most 16 features, where every coalition is enumerated: the exact interventional Shapley value of the
                    network against the background rows (csrc/mlp_shap.hip: mlp_coalition_values, then shapley_combine)
    predict_segments  the back half of ``classify`` for a classifier fitted earlier (forest or MLP)

The forest's arithmetic is scikit-learn's: ``proba`` is bit-identical to
``RandomForestClassifier.predict_proba`` with ``n_jobs=None``.  The MLP's is an order of our own in float64:
scikit-learn's own bits depend on the BLAS call.  There is no CPU path.
"""
import ctypes
import math
import struct
from fractions import Fraction

import numpy as np

from . import _device, _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

MAX_CLASSES, MAX_FEATURES, MAX_TREES = 64, 4096, 65536
_FOREST_ARRAYS = ("threshold", "feature", "left", "right", "missing_go_to_left", "tree_offset", "value")
_DROPPED = ["feature_class", "geometry", "segment_id"]
MLP_MAX_LAYERS, MLP_MAX_WIDTH = 8, 512
_MLP_ARRAYS = ("weights", "biases", "layer_sizes")
_HIDDEN_ACTIVATIONS = ("identity", "relu", "tanh", "logistic")     # obia_mlp.hidden_activation
_OUT_ACTIVATIONS = ("softmax", "logistic")                         # obia_mlp.out_activation
SHAP_MAX_FEATURES = 16                                             # mlp_shap enumerates all 2^F coalitions
_SHAP_VALUES_BYTES = 256 << 20                                     # mlp_shap: the (rows, 2^F, K) coalition values of one piece at most


class Forest:
    """A fitted tree ensemble as flat arrays: the nodes of all trees one after the other.

    ``threshold`` (n,) float64, ``feature`` (n,) int32, ``left`` / ``right`` (n,) int32 -- indices within the node's own tree, -1 at
    a leaf, as scikit-learn's ``children_left`` / ``children_right`` -- ``missing_go_to_left`` (n,) uint8, ``tree_offset`` (T,) int64
    (the first node of every tree, its root), ``value`` (n, K) float64 (what a leaf adds to ``proba`` before the division by T:
    the tree's own ``predict_proba`` row) and ``classes_`` (K,).  ``cover`` (n,) float64, optional: the weight of the training
    rows that reached every node (scikit-learn's ``weighted_n_node_samples``); only :func:`forest_shap` needs it.
    """

    def __init__(self, threshold, feature, left, right, missing_go_to_left, tree_offset, value, classes_, n_features=None, cover=None):
        self.threshold = np.ascontiguousarray(threshold, np.float64)
        self.feature = np.ascontiguousarray(feature, np.int32)
        self.left = np.ascontiguousarray(left, np.int32)
        self.right = np.ascontiguousarray(right, np.int32)
        self.missing_go_to_left = np.ascontiguousarray(missing_go_to_left, np.uint8)
        self.tree_offset = np.ascontiguousarray(tree_offset, np.int64)
        self.value = np.ascontiguousarray(value, np.float64)
        self.classes_ = np.asarray(classes_)
        if self.classes_.dtype == object:
            raise ValueError("classes_ must be numbers or strings, not Python objects")
        n = self.threshold.shape[0]
        if n == 0 or self.tree_offset.ndim != 1 or self.tree_offset.shape[0] == 0:
            raise ValueError("a forest needs at least one tree with one node")
        for name in ("feature", "left", "right", "missing_go_to_left"):
            if getattr(self, name).shape != (n,):
                raise ValueError(f"{name} must hold one entry per node ({n})")
        if self.value.ndim != 2 or self.value.shape != (n, len(self.classes_)):
            raise ValueError("value must be (number of nodes, number of classes)")
        off = self.tree_offset
        if off[0] != 0 or (np.diff(off) <= 0).any() or off[-1] >= n:
            raise ValueError("tree_offset must start at 0, increase and stay below the number of nodes")
        size = np.diff(np.concatenate([off, [n]]))
        per_node = np.repeat(size, size)
        inner = self.left >= 0
        if ((self.left[inner] >= per_node[inner]).any() or (self.right[inner] < 0).any() or (self.right[inner] >= per_node[inner]).any()
                or (self.feature[inner] < 0).any()):
            raise ValueError("a node's children or feature are out of range")
        self.n_features = int(n_features) if n_features is not None else (int(self.feature[inner].max()) + 1 if inner.any() else 1)
        if inner.any() and int(self.feature[inner].max()) >= self.n_features:
            raise ValueError("a node tests a feature beyond n_features")
        self.cover = None if cover is None else np.ascontiguousarray(cover, np.float64)
        if self.cover is not None and self.cover.shape != (n,):
            raise ValueError(f"cover must hold one entry per node ({n})")
        self._dev = {}

    n_nodes = property(lambda self: int(self.threshold.shape[0]))
    n_trees = property(lambda self: int(self.tree_offset.shape[0]))
    n_classes = property(lambda self: int(self.value.shape[1]))

    @classmethod
    def from_sklearn(cls, rf):
        """Read a fitted ``RandomForestClassifier`` (or any ensemble whose ``estimators_`` are single-output
        ``DecisionTreeClassifier``\\ s that vote by averaging ``predict_proba``)."""
        parts = {k: [] for k in _FOREST_ARRAYS}
        cover = []
        offset = 0
        for est in rf.estimators_:
            t = est.tree_
            if t.value.shape[1] != 1:
                raise NotImplementedError("multi-output trees are not supported")
            n = int(t.node_count)
            v = np.array(t.value[:, 0, :], dtype=np.float64)
            # what DecisionTreeClassifier.predict_proba returns for a leaf: current versions store class fractions and return
            # them untouched; older ones store weighted counts and divide by the row sum (0 -> 1)
            root = float(v[0].sum())
            if abs(root - float(t.weighted_n_node_samples[0])) < abs(root - 1.0):
                norm = v.sum(axis=1)
                norm[norm == 0.0] = 1.0
                v = v / norm[:, None]
            parts["threshold"].append(np.asarray(t.threshold, np.float64))
            parts["feature"].append(np.asarray(t.feature, np.int32))
            parts["left"].append(np.asarray(t.children_left, np.int32))
            parts["right"].append(np.asarray(t.children_right, np.int32))
            mgl = getattr(t, "missing_go_to_left", None)
            parts["missing_go_to_left"].append(np.zeros(n, np.uint8) if mgl is None else np.asarray(mgl, np.uint8))
            parts["tree_offset"].append(offset)
            parts["value"].append(v)
            cover.append(np.asarray(t.weighted_n_node_samples, np.float64))
            offset += n
        if not parts["value"]:
            raise ValueError("the ensemble has no trees")
        cat = {k: np.concatenate(v) for k, v in parts.items() if k != "tree_offset"}
        return cls(tree_offset=np.asarray(parts["tree_offset"], np.int64), classes_=np.asarray(rf.classes_),
                   n_features=int(rf.n_features_in_), cover=np.concatenate(cover), **cat)

    def save(self, path):
        """Plain ``.npz`` of the arrays and ``classes_`` (and ``cover`` when there is one); nothing pickled."""
        extra = {} if self.cover is None else {"cover": self.cover}
        np.savez(path, classes_=self.classes_, n_features=np.int64(self.n_features), **{k: getattr(self, k) for k in _FOREST_ARRAYS}, **extra)
        return path

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(classes_=z["classes_"], n_features=int(z["n_features"]), cover=z["cover"] if "cover" in z.files else None,
                       **{k: z[k] for k in _FOREST_ARRAYS})

    def _on(self, device):
        d = self._dev.get(str(device))
        if d is None:
            d = self._dev[str(device)] = {k: torch.as_tensor(getattr(self, k), device=device) for k in _FOREST_ARRAYS}
        return d

    def _cover_on(self, device):
        """``cover`` on the device, uploaded once (kept apart from :meth:`_on`: prediction does not need it)."""
        d = self._dev.get(("cover", str(device)))
        if d is None:
            d = self._dev[("cover", str(device))] = torch.as_tensor(self.cover, device=device)
        return d


class MLP:
    """A fitted multi-layer perceptron as flat arrays: ``weights`` float64 = ``coefs_[0]``, ``coefs_[1]``, ... each row-major
    (n_in, n_out), one after the other; ``biases`` float64 = ``intercepts_`` likewise; ``layer_sizes`` int32 = n_features, hidden
    widths ..., n_out (the number of classes, or 1 for the binary logistic output); ``hidden_activation`` one of identity / relu /
    tanh / logistic; ``out_activation`` softmax or logistic; ``classes_`` (K,)."""

    def __init__(self, weights, biases, layer_sizes, hidden_activation, out_activation, classes_):
        self.weights = np.ascontiguousarray(weights, np.float64)
        self.biases = np.ascontiguousarray(biases, np.float64)
        self.layer_sizes = np.ascontiguousarray(layer_sizes, np.int32)
        self.hidden_activation, self.out_activation = str(hidden_activation), str(out_activation)
        self.classes_ = np.asarray(classes_)
        if self.classes_.dtype == object:
            raise ValueError("classes_ must be numbers or strings, not Python objects")
        if self.hidden_activation not in _HIDDEN_ACTIVATIONS:
            raise ValueError(f"hidden_activation must be one of {_HIDDEN_ACTIVATIONS}, got {self.hidden_activation!r}")
        if self.out_activation not in _OUT_ACTIVATIONS:
            raise ValueError(f"out_activation must be one of {_OUT_ACTIVATIONS}, got {self.out_activation!r}")
        ls = self.layer_sizes
        if ls.ndim != 1 or ls.shape[0] < 2 or (ls <= 0).any():
            raise ValueError("layer_sizes must hold n_features, the hidden widths and n_out, all positive")
        n_w = int((ls[:-1].astype(np.int64) * ls[1:]).sum())
        if self.weights.shape != (n_w,) or self.biases.shape != (int(ls[1:].sum()),):
            raise ValueError(f"layer_sizes {ls.tolist()} need {n_w} weights and {int(ls[1:].sum())} biases, flat")
        if self.classes_.ndim != 1 or len(self.classes_) != (int(ls[-1]) if self.out_activation == "softmax" else 2) or \
                (self.out_activation == "logistic" and ls[-1] != 1):
            raise ValueError("softmax needs one output per class; the logistic output is one unit for two classes")
        self._dev = {}

    n_features = property(lambda self: int(self.layer_sizes[0]))
    n_layers = property(lambda self: int(self.layer_sizes.shape[0]) - 1)
    n_classes = property(lambda self: int(len(self.classes_)))

    @classmethod
    def from_sklearn(cls, clf):
        """Read a fitted ``MLPClassifier``.  float32 ``coefs_`` become float64, as NumPy promotes them against a float64 table."""
        if clf.out_activation_ == "logistic" and clf.n_outputs_ > 1:
            raise NotImplementedError("multilabel MLPClassifier (several logistic outputs) is not supported")
        ls = [int(clf.coefs_[0].shape[0])] + [int(w.shape[1]) for w in clf.coefs_]
        return cls(np.concatenate([np.asarray(w, np.float64).ravel() for w in clf.coefs_]),
                   np.concatenate([np.asarray(b, np.float64).ravel() for b in clf.intercepts_]), ls, clf.activation, clf.out_activation_,
                   np.asarray(clf.classes_))

    def layers(self):
        """[(W (n_in, n_out), b (n_out,)), ...] as views of the flat arrays."""
        out, wo, bo = [], 0, 0
        for n_in, n_out in zip(self.layer_sizes[:-1].tolist(), self.layer_sizes[1:].tolist()):
            out.append((self.weights[wo:wo + n_in * n_out].reshape(n_in, n_out), self.biases[bo:bo + n_out]))
            wo, bo = wo + n_in * n_out, bo + n_out
        return out

    def save(self, path):
        """Plain ``.npz`` of the arrays, the two activation names and ``classes_``; nothing pickled."""
        np.savez(path, classes_=self.classes_, hidden_activation=np.str_(self.hidden_activation),
                 out_activation=np.str_(self.out_activation), **{k: getattr(self, k) for k in _MLP_ARRAYS})
        return path

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(classes_=z["classes_"], hidden_activation=str(z["hidden_activation"]), out_activation=str(z["out_activation"]),
                       **{k: z[k] for k in _MLP_ARRAYS})

    def _on(self, device):
        d = self._dev.get(str(device))
        if d is None:
            d = self._dev[str(device)] = {k: torch.as_tensor(getattr(self, k), device=device) for k in ("weights", "biases")}
        return d


def standard_scale(table, ctx=None, dtype=np.float32):
    """``StandardScaler().fit(table).transform(table)`` followed by the forest's cast: returns ``(X32, mean, scale)`` with X32
    (N, F) float32 and ``mean`` / ``scale`` (F,) float64 (obia_table_scale_dev).  Per column the NaNs are left out of the count,
    the mean and the two-pass variance; a column scikit-learn treats as constant gets scale 1; an all-NaN column stays NaN.
    ``dtype=np.float64``: the table without the cast, as ``MLPClassifier`` is handed it (obia_table_scale_f64_dev; ``mean`` and
    ``scale`` are the same bits).  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensors out."""
    _device.need_torch("obia_amd.classify")
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("dtype must be numpy.float32 or numpy.float64")
    is_t = _device.is_torch(table)
    dev = _device.device_of(ctx, table)
    shape = tuple(table.shape)
    if len(shape) != 2 or shape[1] == 0:
        raise ValueError("table must be (rows, features)")
    if shape[0] == 0:
        raise ValueError("the table has no rows")
    t = _device.as_dev(table, torch.float64, dev)
    N, F = shape
    mean = torch.empty((F,), dtype=torch.float64, device=t.device)
    scale = torch.empty_like(mean)
    wide = dtype == np.dtype(np.float64)
    out = torch.empty((N, F), dtype=torch.float64 if wide else torch.float32, device=t.device)
    lib, c = _device.begin(dev, ctx)
    entry = lib.obia_table_scale_f64_dev if wide else lib.obia_table_scale_dev
    _lib.check(entry(c.handle, t.data_ptr(), N, F, mean.data_ptr(), scale.data_ptr(), out.data_ptr()))
    return _device.out((out, mean, scale), is_t)


def _check_candidates(acceptable, n_rows, n_classes):
    """The reference raises where a row has fewer than two candidate classes (``np.partition(..., -2)`` on one value, ``idxmax``
    on none, classify.py:150-151,157): so does this, before anything is launched."""
    if acceptable is None:
        if n_classes < 2:
            raise ValueError("prediction needs at least two classes (the margin is the difference of the two largest probabilities)")
        return
    if tuple(acceptable.shape) != (n_rows, n_classes):
        raise ValueError(f"acceptable must be (rows, classes) = ({n_rows}, {n_classes}), got {tuple(acceptable.shape)}")
    few = (acceptable != 0).sum(1) < 2
    if bool(few.any()):
        first = int(few.nonzero()[0][0]) if not _device.is_torch(few) else int(few.nonzero()[0, 0])
        raise ValueError(f"row {first} has fewer than two acceptable classes among classes_")


def _check_forest_table(forest, X32, who):
    """The argument checks :func:`forest_predict` and :func:`forest_shap` share; returns ``(is_torch, rows, columns)``."""
    if not isinstance(forest, Forest):
        raise TypeError("forest must be an obia_amd.classify.Forest (Forest.from_sklearn(rf))")
    _device.device_of(None, X32)                       # (a CPU tensor is refused here)
    shape = tuple(X32.shape)
    if len(shape) != 2:
        raise ValueError("X32 must be (rows, features)")
    N, F = shape
    if N == 0:
        raise ValueError("the table has no rows")
    if F < forest.n_features:
        raise ValueError(f"the forest tests feature {forest.n_features - 1}, the table has {F} columns")
    K = forest.n_classes
    if K > MAX_CLASSES or F > MAX_FEATURES or forest.n_trees > MAX_TREES or forest.n_nodes >= 2 ** 31:
        raise NotImplementedError(f"{who} supports at most {MAX_CLASSES} classes, {MAX_FEATURES} features, {MAX_TREES} trees "
                                  f"and 2^31 - 1 nodes (got {K}, {F}, {forest.n_trees}, {forest.n_nodes})")
    return _device.is_torch(X32), N, F


def _forest_struct(forest, device):
    d = forest._on(device)
    return _lib.Forest(*(d[k].data_ptr() for k in ("threshold", "feature", "left", "right", "missing_go_to_left", "tree_offset")),
                       forest.tree_offset.ctypes.data, d["value"].data_ptr(), forest.n_nodes, forest.n_trees, forest.n_classes)


def forest_predict(forest, X32, acceptable=None, ctx=None):
    """Prediction of ``forest`` for every row of ``X32`` (N, F) float32: returns ``(pred, margin, proba)``.

    ``proba`` (N, K) float64 is ``RandomForestClassifier.predict_proba`` bit for bit (leaf rows added in float64 in tree order,
    divided by the number of trees), never filtered.  ``acceptable``: optional (N, K) boolean mask in ``classes_`` order;
    ``pred`` (N,) int32 is the index into ``classes_`` of the first maximum of ``proba`` over the row's acceptable classes
    (all classes without a mask), ``margin`` (N,) float64 the largest minus the second largest of those values.  A row with
    fewer than two candidates raises ValueError.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensors out."""
    _device.need_torch("obia_amd.classify")
    is_t, N, F = _check_forest_table(forest, X32, "forest_predict")
    K = forest.n_classes
    _check_candidates(acceptable, N, K)
    dev = _device.device_of(ctx, X32, acceptable)
    x = _device.as_dev(X32, torch.float32, dev)
    mask = None if acceptable is None else _lib.mask_bytes(acceptable, device=x.device)
    fs = _forest_struct(forest, x.device)
    proba = torch.empty((N, K), dtype=torch.float64, device=x.device)
    pred = torch.empty((N,), dtype=torch.int32, device=x.device)
    margin = torch.empty((N,), dtype=torch.float64, device=x.device)
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_forest_predict_dev(c.handle, x.data_ptr(), N, F, ctypes.byref(fs), None if mask is None else mask.data_ptr(),
                                           proba.data_ptr(), pred.data_ptr(), margin.data_ptr()))
    return _device.out((pred, margin, proba), is_t)


def forest_shap(forest, X32, ctx=None):
    """SHAP values of ``forest`` for every row of ``X32`` (N, F) float32: returns ``(phi, base)``.

    ``phi`` (N, F, K) float64 -- the layout ``shap.TreeExplainer(rf).shap_values(x)`` returns for a multi-class forest -- is the
    Shapley value of every feature for every class under the forest's path-dependent value function (no background data: a
    feature outside the coalition is averaged out with ``cover[child] / cover[node]``); ``base`` (K,) float64 is the
    cover-weighted mean of the leaves, the explainer's ``expected_value``.  ``phi.sum(1) + base`` is ``proba`` of
    :func:`forest_predict` up to rounding, and a feature no tree tests gets exactly 0.  The rows are walked as
    :func:`forest_predict` walks them (cast to float32, NaN by ``missing_go_to_left``), which is where this departs from the
    ``shap`` package.  Float64 throughout, no floating-point atomics: two calls agree bit for bit, and a row's
    result does not depend on the other rows.  A path may test at most 32 distinct features.

    The output takes N * F * K * 8 bytes: 1.9 GB for 489 480 x 96 x 5.  ``forest`` needs ``cover`` (``Forest.from_sklearn``
    fills it).  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensors out."""
    _device.need_torch("obia_amd.classify")
    if isinstance(forest, Forest) and forest.cover is None:
        raise ValueError("forest_shap needs the nodes' cover: build the forest with Forest.from_sklearn(rf) or pass cover=")
    is_t, N, F = _check_forest_table(forest, X32, "forest_shap")
    K = forest.n_classes
    dev = _device.device_of(ctx, X32)
    x = _device.as_dev(X32, torch.float32, dev)
    fs = _forest_struct(forest, x.device)
    phi = torch.empty((N, F, K), dtype=torch.float64, device=x.device)
    base = torch.empty((K,), dtype=torch.float64, device=x.device)
    cover = forest._cover_on(x.device)
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_forest_shap_dev(c.handle, x.data_ptr(), N, F, ctypes.byref(fs), cover.data_ptr(), phi.data_ptr(), base.data_ptr()))
    return _device.out((phi, base), is_t)


def _mlp_plan(layer_sizes):
    """(rows a workgroup takes, features of the input layer staged at a time) of obia_mlp_predict_dev for these layer sizes: the
    same few lines as in csrc/mlp.hip, for the tests that walk the kernel's thresholds.  64 KB of LDS hold two activation buffers
    of (widest layer output) x rows doubles and the staging buffer of features x (rows + 1)."""
    ls = [int(v) for v in layer_sizes]
    wmax, rows = max(ls[1:]), 64
    while 2 * wmax * rows + 8 * (rows + 1) > 8192:
        rows //= 2
    return rows, min(ls[0], (8192 - 2 * wmax * rows) // (rows + 1))


def mlp_predict(mlp, X, acceptable=None, ctx=None, _logits=False):
    """Prediction of ``mlp`` for every row of ``X`` (N, F) float64: returns ``(pred, margin, proba)``.

    ``proba`` (N, K) float64 is ``MLPClassifier.predict_proba`` in the summation order of DESIGN.md 3.5j (inputs in ascending
    order, every product and sum rounded on its own), never filtered; it agrees with scikit-learn's to a few units of the last
    place of 1.  ``acceptable`` / ``pred`` / ``margin``: as in :func:`forest_predict`.  A NaN or an infinity in ``X`` raises
    ValueError, as scikit-learn does.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensors out.  ``_logits=True`` appends the
    last layer before its activation, (N, n_out) (test hook)."""
    _device.need_torch("obia_amd.classify")
    if not isinstance(mlp, MLP):
        raise TypeError("mlp must be an obia_amd.classify.MLP (MLP.from_sklearn(clf))")
    is_t = _device.is_torch(X)
    _device.device_of(None, X)                         # (a CPU tensor is refused here)
    shape = tuple(X.shape)
    if len(shape) != 2:
        raise ValueError("X must be (rows, features)")
    N, F = shape
    if N == 0:
        raise ValueError("the table has no rows")
    if F != mlp.n_features:
        raise ValueError(f"the network takes {mlp.n_features} features, the table has {F} columns")
    K, ls = mlp.n_classes, mlp.layer_sizes
    if mlp.n_layers > MLP_MAX_LAYERS or F > MAX_FEATURES or K > MAX_CLASSES or (mlp.n_layers > 1 and int(ls[1:-1].max()) > MLP_MAX_WIDTH):
        raise NotImplementedError(f"mlp_predict supports at most {MLP_MAX_LAYERS} weight matrices, {MAX_FEATURES} features, {MAX_CLASSES} "
                                  f"classes and {MLP_MAX_WIDTH} units in a hidden layer (layer sizes {ls.tolist()}, {K} classes)")
    _check_candidates(acceptable, N, K)
    dev = _device.device_of(ctx, X, acceptable)
    x = _device.as_dev(X, torch.float64, dev)
    mask = None if acceptable is None else _lib.mask_bytes(acceptable, device=x.device)
    ms = _mlp_struct(mlp, x.device)
    proba = torch.empty((N, K), dtype=torch.float64, device=x.device)
    pred = torch.empty((N,), dtype=torch.int32, device=x.device)
    margin = torch.empty((N,), dtype=torch.float64, device=x.device)
    logits = torch.empty((N, int(ls[-1])), dtype=torch.float64, device=x.device) if _logits else None
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_mlp_predict_dev(c.handle, x.data_ptr(), N, F, ctypes.byref(ms), None if mask is None else mask.data_ptr(),
                                        proba.data_ptr(), pred.data_ptr(), margin.data_ptr(), None if logits is None else logits.data_ptr()))
    return _device.out((pred, margin, proba) + ((logits,) if _logits else ()), is_t)


def _check_mlp_table(mlp, X, name, who):
    """The argument checks of :func:`mlp_predict` for one table; returns ``(is_torch, rows)``."""
    if not isinstance(mlp, MLP):
        raise TypeError("mlp must be an obia_amd.classify.MLP (MLP.from_sklearn(clf))")
    _device.device_of(None, X)                         # (a CPU tensor is refused here)
    shape = tuple(X.shape)
    if len(shape) != 2:
        raise ValueError(f"{name} must be (rows, features)")
    if shape[1] != mlp.n_features:
        raise ValueError(f"the network takes {mlp.n_features} features, {name} has {shape[1]} columns")
    K, ls = mlp.n_classes, mlp.layer_sizes
    if mlp.n_layers > MLP_MAX_LAYERS or shape[1] > MAX_FEATURES or K > MAX_CLASSES or (mlp.n_layers > 1 and int(ls[1:-1].max()) > MLP_MAX_WIDTH):
        raise NotImplementedError(f"{who} supports at most {MLP_MAX_LAYERS} weight matrices, {MAX_FEATURES} features, {MAX_CLASSES} "
                                  f"classes and {MLP_MAX_WIDTH} units in a hidden layer (layer sizes {ls.tolist()}, {K} classes)")
    return _device.is_torch(X), shape[0]


def _mlp_struct(mlp, device):
    d = mlp._on(device)
    return _lib.Mlp(d["weights"].data_ptr(), d["biases"].data_ptr(), mlp.layer_sizes.ctypes.data, mlp.n_layers,
                    _HIDDEN_ACTIVATIONS.index(mlp.hidden_activation), _OUT_ACTIVATIONS.index(mlp.out_activation), mlp.n_classes)


def _coalition_inputs(mlp, X, background, who, ctx, masks=None):
    """Checks both tables (before the library is loaded) and puts them on one device: ``(x, bg, device index, is_torch)``."""
    _device.need_torch("obia_amd.classify")
    is_t, N = _check_mlp_table(mlp, X, "X", who)
    _, B = _check_mlp_table(mlp, background, "background", who)
    if N == 0:
        raise ValueError("the table has no rows")
    if B == 0:
        raise ValueError("the background has no rows")
    dev = _device.device_of(ctx, X, background, masks)
    return _device.as_dev(X, torch.float64, dev), _device.as_dev(background, torch.float64, dev), dev, is_t


def mlp_coalition_values(mlp, X, background, masks, ctx=None):
    """Coalition values of ``mlp`` for every row of ``X`` (N, F) float64 against ``background`` (B, F) float64 under ``masks``
    (M, F) boolean: returns ``values`` (N, M, K) float64,

        ``values[n, m] = (...((0.0 + p(h_0)) + p(h_1)) + ... + p(h_{B-1})) / B``,

    where ``h_b[f] = X[n, f]`` if ``masks[m, f]`` else ``background[b, f]`` and ``p`` is ``proba`` of :func:`mlp_predict` for that
    row, the same bits: the background rows are added in ascending order from 0.0 and the sum is divided once
    by B; the empty and the full mask follow the same rule.  This is the game whose Shapley values :func:`mlp_shap` returns, and
    what a sampled KernelSHAP for wider tables would evaluate.  A NaN or an infinity in ``X`` or ``background`` raises
    ValueError.  The limits of :func:`mlp_predict`; B >= 1, M >= 1.  NumPy in -> NumPy out, CUDA tensor ``X`` in -> CUDA tensor out."""
    _device.need_torch("obia_amd.classify")
    if not _device.is_torch(masks):
        masks = np.asarray(masks)
    if isinstance(mlp, MLP) and (len(tuple(masks.shape)) != 2 or masks.shape[1] != mlp.n_features or masks.shape[0] == 0):
        raise ValueError(f"masks must be (coalitions, features) = (M >= 1, {mlp.n_features}), got {tuple(masks.shape)}")
    x, bg, dev, is_t = _coalition_inputs(mlp, X, background, "mlp_coalition_values", ctx, masks)
    mk = _lib.mask_bytes(masks, device=x.device)
    N, M, K = x.shape[0], mk.shape[0], mlp.n_classes
    values = torch.empty((N, M, K), dtype=torch.float64, device=x.device)
    ms = _mlp_struct(mlp, x.device)
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_mlp_coalition_dev(c.handle, x.data_ptr(), N, x.shape[1], ctypes.byref(ms), bg.data_ptr(), bg.shape[0], mk.data_ptr(), M,
                                          values.data_ptr()))
    return _device.out(values, is_t)


def _check_shap_width(mlp):
    if isinstance(mlp, MLP) and mlp.n_features > SHAP_MAX_FEATURES:
        raise NotImplementedError(f"mlp_shap enumerates all 2^F coalitions and supports at most {SHAP_MAX_FEATURES} features (the network "
                                  f"takes {mlp.n_features}); for a wider table evaluate chosen coalitions with mlp_coalition_values")


def _size_weights(F):
    """w[s] = s! (F - 1 - s)! / F! for s = 0 .. F - 1, each the correctly rounded float64 of the rational."""
    return np.array([float(Fraction(math.factorial(s) * math.factorial(F - 1 - s), math.factorial(F))) for s in range(F)], np.float64)


def _combine(lib, c, values, F, K, phi):
    w = _size_weights(F)
    _lib.check(lib.obia_shapley_combine_dev(c.handle, values.data_ptr(), phi.shape[0], F, K, w.ctypes.data, phi.data_ptr()))


def shapley_combine(values, ctx=None):
    """Shapley values from the values of all coalitions: ``values`` (N, 2^F, K) float64, row m the coalition whose bit f says that
    feature f is in it; returns ``phi`` (N, F, K) float64,

        ``phi[n, f, k] = sum over the m without bit f of w[popcount(m)] * (values[n, m | 1 << f, k] - values[n, m, k])``,

    ``w[s] = s! (F - 1 - s)! / F!`` rounded correctly from the rational.  The coalitions are taken in ascending m from 0.0; every
    difference, product and sum is rounded on its own, so two calls agree bit for bit.  F <= 16.  NumPy in -> NumPy out, CUDA
    tensor in -> CUDA tensor out."""
    _device.need_torch("obia_amd.classify")
    is_t = _device.is_torch(values)
    dev = _device.device_of(ctx, values)
    shape = tuple(values.shape)
    if len(shape) != 3 or shape[1] < 2 or shape[1] & (shape[1] - 1) or shape[2] == 0:
        raise ValueError("values must be (rows, 2^F coalitions, classes) with F >= 1")
    N, M, K = shape
    F = M.bit_length() - 1
    if N == 0:
        raise ValueError("the table has no rows")
    if F > SHAP_MAX_FEATURES or K > MAX_CLASSES:
        raise NotImplementedError(f"shapley_combine supports at most {SHAP_MAX_FEATURES} features and {MAX_CLASSES} classes (got {F}, {K})")
    v = _device.as_dev(values, torch.float64, dev)
    phi = torch.empty((N, F, K), dtype=torch.float64, device=v.device)
    lib, c = _device.begin(dev, ctx)
    _combine(lib, c, v, F, K, phi)
    return _device.out(phi, is_t)


def mlp_shap(mlp, X, background, ctx=None):
    """Exact Shapley values of ``mlp`` for every row of ``X`` (N, F) float64 against ``background`` (B, F) float64: returns
    ``(phi, base)``.

    The game is ``v(S) = mean over the background rows b of predict_proba(x on the features in S, background[b] elsewhere)`` --
    what ``shap.KernelExplainer(clf.predict_proba, background).shap_values(X)`` fits when its budget covers every coalition (up
    to 11 features with the default budget); here all 2^F coalitions are evaluated for up to 16 features, with no sampling
    (DESIGN.md 3.5l, 5).  ``phi`` (N, F, K) float64 is the layout ``shap_values[:, :, class_ind]`` indexes; ``base`` (K,) float64
    is the value of the empty coalition, the explainer's ``expected_value``.  ``phi.sum(1) + base`` is ``proba`` of
    :func:`mlp_predict` up to rounding, and a feature on which a row equals every background row gets exactly +0.0.
    :func:`mlp_coalition_values` on all coalitions in binary order, then :func:`shapley_combine`, a piece of rows at a time so
    that the coalition values stay under ``_SHAP_VALUES_BYTES``; a row's result does not depend on the piece it fell in.
    The work is N * 2^F * B forward passes.  NumPy in -> NumPy out, CUDA tensor ``X`` in -> CUDA tensors out."""
    _check_shap_width(mlp)
    x, bg, dev, is_t = _coalition_inputs(mlp, X, background, "mlp_shap", ctx)
    N, F = x.shape
    K, M = mlp.n_classes, 1 << F
    rows = max(1, min(N, _SHAP_VALUES_BYTES // (M * K * 8)))
    values = torch.empty((rows, M, K), dtype=torch.float64, device=x.device)
    phi = torch.empty((N, F, K), dtype=torch.float64, device=x.device)
    base = None
    ms = _mlp_struct(mlp, x.device)
    lib, c = _device.begin(dev, ctx)
    for r0 in range(0, N, rows):
        n = min(rows, N - r0)
        _lib.check(lib.obia_mlp_coalition_dev(c.handle, x[r0:r0 + n].data_ptr(), n, F, ctypes.byref(ms), bg.data_ptr(), bg.shape[0], None, M,
                                              values.data_ptr()))
        _combine(lib, c, values, F, K, phi[r0:r0 + n])
        if base is None:
            base = values[0, 0].clone()                # the empty coalition does not depend on the row
            torch.cuda.current_stream(dev).synchronize()   # copied before the next piece overwrites it
    return _device.out((phi, base), is_t)


class ClassifiedImage:
    """The reference's result object (classify.py:12-65): ``classified`` (the segment table with ``predicted_class`` and
    ``prediction_margin``), ``confusion_matrix``, ``report``, ``shap_values``, ``transform``, ``crs``, ``params``.  ``shap_base_values`` (not in the
    reference) is the explainer's ``expected_value`` that goes with ``shap_values``; both are None unless they were asked for."""

    def __init__(self, classified, confusion_matrix, report, shap_values, transform, crs, params):
        self.classified = classified
        self.report = report
        self.confusion_matrix = confusion_matrix
        self.shap_values = shap_values
        self.params = params
        self.transform = transform
        self.crs = crs
        self.shap_base_values = None

    def to_raster(self, labels, start_label=1, fill=0):
        """Class per pixel: a gather of ``predicted_class`` through the label raster.  The table's rows are the labels that
        exist, in ascending order (as create_objects numbers them); pixels below ``start_label`` get ``fill``.  Classes must be
        integers.  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out (int32)."""
        _device.need_torch("obia_amd.classify")
        cls = np.asarray(self.classified["predicted_class"])
        try:
            cls_i = cls.astype(np.int64)
            exact = bool(np.all(cls_i == cls))
        except (TypeError, ValueError):
            exact = False
        if not exact or (cls_i.size and (cls_i.min() < -2 ** 31 or cls_i.max() >= 2 ** 31)):
            raise ValueError("to_raster needs integer classes that fit int32")
        is_t = _device.is_torch(labels)
        lab = _device.as_dev(labels, torch.int64, _device.device_of(None, labels))
        valid = lab >= start_label
        present = torch.unique(lab[valid])
        if present.numel() != len(cls_i):
            raise ValueError(f"the label raster holds {present.numel()} segments, the table {len(cls_i)} rows")
        n = int(present[-1].item()) - start_label + 1 if present.numel() else 0
        lut = torch.full((n + 1,), int(fill), dtype=torch.int32, device=lab.device)       # (last entry: pixels below start_label)
        lut[present - start_label] = torch.as_tensor(cls_i, device=lab.device).to(torch.int32)
        out = lut[torch.where(valid, lab - start_label, torch.full_like(lab, n))]
        return _device.out(out, is_t)


def _zone_wkb(geom):
    """One zone geometry as little-endian WKB: bytes as they are, an object with ``.wkb`` (shapely), or one (V, 2) ring."""
    if isinstance(geom, (bytes, bytearray, memoryview)):
        return bytes(geom)
    if hasattr(geom, "wkb"):
        return bytes(geom.wkb)
    ring = np.asarray(geom, dtype="<f8")
    if ring.ndim != 2 or ring.shape[1] != 2 or ring.shape[0] < 3:
        raise ValueError("a zone geometry must be WKB bytes or a (V, 2) ring")
    return struct.pack("<BII", 1, 3, 1) + struct.pack("<I", ring.shape[0]) + ring.tobytes()


def acceptable_mask(acceptable_classes_gdf, classes_, labels, affine_transformation=None, start_label=1, ctx=None):
    """The (segments, classes) boolean mask of ``classify(acceptable_classes_gdf=...)`` on the label raster.

    ``acceptable_classes_gdf``: a table with ``geometry`` (WKB bytes, shapely geometries or (V, 2) rings) and
    ``acceptable_classes`` (a list of class values per row).  The zones are burnt with :func:`obia_amd.polygons.rasterize` in
    reverse table order, so the first row wins a pixel; a segment's zone is the lowest row index under its pixel centres (the
    ``min`` of :func:`obia_amd.statistics.zonal_stats` on that raster) -- the reference's ``intersections.iloc[0]``
    (classify.py:140-143).  A segment under no zone accepts every class.  One row per existing label, ascending.
    Deviation: the reference's ``intersects`` also counts a zone that only touches a segment's border or covers
    none of its pixel centres; the raster rule does not."""
    from .polygons import rasterize
    from .statistics import zonal_stats
    geoms = list(acceptable_classes_gdf["geometry"])
    wanted = list(acceptable_classes_gdf["acceptable_classes"])
    nz = len(geoms)
    if nz >= 2 ** 24:
        raise NotImplementedError("2^24 or more zones are not supported")
    lab = labels if _device.is_torch(labels) else np.asarray(labels)
    H, W = (int(v) for v in lab.shape)
    classes_ = np.asarray(classes_)
    zone_rows = np.stack([np.isin(classes_, np.asarray(list(w))) for w in wanted]) if nz else np.zeros((0, len(classes_)), bool)
    order = np.arange(nz - 1, -1, -1)
    zr = rasterize([_zone_wkb(geoms[i]) for i in order], (H, W), affine_transformation=affine_transformation,
                   values=order.astype(np.int32), fill=-1, ctx=ctx, as_tensor=True)
    plane = zr.to(torch.float32)
    plane[zr < 0] = float("nan")                       # zonal_stats drops NaN pixels: no zone here
    lab_t = lab if _device.is_torch(lab) else torch.as_tensor(np.ascontiguousarray(lab, dtype=np.int32), device=zr.device)
    st = zonal_stats(plane[:, :, None].contiguous(), lab_t, start_label=start_label, ctx=ctx)
    present = (st["count"] > 0).cpu().numpy()
    zone = st["min"][:, 0].cpu().numpy()[present]
    mask = np.ones((int(present.sum()), len(classes_)), bool)
    has = ~np.isnan(zone)
    mask[has] = zone_rows[zone[has].astype(np.int64)]
    return mask


def classify(segments, training_classes, acceptable_classes_gdf=None, method='rf', test_size=0.2, compute_reports=False,
             compute_shap=False, sample_shap=False, *, acceptable=None, labels=None, affine_transformation=None, start_label=1,
             ctx=None, **kwargs):
    """Mirror of obia ``classify`` (classify.py:68-175): same positional order and defaults.

    On the host, as the reference does it: ``feature_class`` / ``geometry`` / ``segment_id`` are dropped,
    ``train_test_split(random_state=42)``, a ``StandardScaler`` per split, ``RandomForestClassifier(**kwargs).fit``, the
    reports when asked.  On the device: :func:`standard_scale` on the segments' feature columns and :func:`forest_predict` for
    all rows at once instead of one ``predict_proba`` call per row.  ``segments`` gains ``predicted_class`` (the class value)
    and ``prediction_margin`` and is returned inside a :class:`ClassifiedImage`.

    ``acceptable``: (N, K) boolean mask in ``classes_`` order, or ``acceptable_classes_gdf`` (see :func:`acceptable_mask`; needs
    ``segments.attrs["labels"]`` or ``labels=``, and ``affine_transformation=`` when the zones are in map coordinates).
    ``method='mlp'`` and ``compute_shap=True`` are refused here: fit the classifier yourself and call :func:`predict_segments`
    (``compute_shap=True`` there, or :func:`forest_shap`)."""
    if method == 'mlp':
        raise NotImplementedError("method='mlp' is not switched on in classify(): fit the MLPClassifier and call predict_segments")
    if method != 'rf':
        raise ValueError('An unsupported classification algorithm was requested')
    if compute_shap:
        raise NotImplementedError("compute_shap=True is not switched on in classify(): fit the forest and call "
                                  "predict_segments(..., compute_shap=True) or forest_shap")
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import train_test_split
    from sklearn.preprocessing import StandardScaler

    x = training_classes.drop(_DROPPED, axis=1)
    y = training_classes['feature_class']
    x_train, x_test, y_train, y_test = train_test_split(x, y, test_size=test_size, random_state=42)
    x_train = StandardScaler().fit_transform(x_train)
    classifier = RandomForestClassifier(**kwargs)
    classifier.fit(x_train, y_train)
    report = cm = None
    if compute_reports:
        from sklearn.metrics import classification_report, confusion_matrix
        y_pred = classifier.predict(StandardScaler().fit_transform(x_test))
        cm = confusion_matrix(y_test, y_pred)
        report = classification_report(y_test, y_pred)

    res = predict_segments(classifier, segments, acceptable_classes_gdf, acceptable=acceptable, labels=labels,
                           affine_transformation=affine_transformation, start_label=start_label, ctx=ctx)
    res.confusion_matrix, res.report = cm, report
    return res


def predict_segments(classifier, segments, acceptable_classes_gdf=None, *, acceptable=None, labels=None, affine_transformation=None,
                     start_label=1, ctx=None, **options):
    """The back half of :func:`classify` (classify.py:125-175) for a classifier fitted earlier, so that a second raster or tile
    does not pay for training again.

    ``classifier``: a fitted ``RandomForestClassifier`` or ``MLPClassifier``, a :class:`Forest` or an :class:`MLP`.  The three
    non-feature columns are dropped, the rest scaled with :func:`standard_scale` -- float32 for a forest, float64 for an MLP --
    and predicted with :func:`forest_predict` / :func:`mlp_predict`.  ``segments`` gains ``predicted_class`` and
    ``prediction_margin`` and is returned inside a :class:`ClassifiedImage` whose ``params`` are the estimator's ``get_params()``
    ({} for a Forest or an MLP).  The acceptable-class arguments are those of :func:`classify`.

    One more keyword, ``compute_shap=False`` (taken through ``**options`` so that the listed keywords, which a test pins, stay
    as they are; any other name raises TypeError).  ``compute_shap=True``, forests only: ``shap_values`` is ``phi`` (rows,
    features, classes) of :func:`forest_shap` on the scaled table and ``shap_base_values`` its ``base``; mind the size, rows x
    features x classes x 8 bytes.  ``compute_shap=True, shap_background=B`` (a second key taken the same way), MLPs only: ``B``
    (rows, features) is a background table in the scaled feature space, and ``shap_values`` / ``shap_base_values`` are ``phi`` /
    ``base`` of :func:`mlp_shap` on the float64 scaled table against it (at most 16 features).  Without a background an MLP is
    refused; a background given with a forest, whose explainer takes none, or without ``compute_shap=True`` raises
    ValueError."""
    import pandas as pd
    compute_shap = bool(options.pop("compute_shap", False))
    shap_background = options.pop("shap_background", None)
    if options:
        raise TypeError(f"predict_segments() got an unexpected keyword argument {sorted(options)[0]!r}")
    params = {}
    if isinstance(classifier, (Forest, MLP)):
        model = classifier
    else:
        params = classifier.get_params()
        if hasattr(classifier, "coefs_"):
            model = MLP.from_sklearn(classifier)
        elif hasattr(classifier, "estimators_"):
            model = Forest.from_sklearn(classifier)
        else:
            raise TypeError("classifier must be a fitted RandomForestClassifier or MLPClassifier, a Forest or an MLP")
    x_pred = segments.drop(_DROPPED, axis=1, errors='ignore')
    if acceptable is None and acceptable_classes_gdf is not None:
        if labels is None:
            labels = getattr(segments, "attrs", {}).get("labels")
        if labels is None:
            raise ValueError("acceptable_classes_gdf needs the label raster: segments.attrs['labels'] or labels=")
        acceptable = acceptable_mask(acceptable_classes_gdf, model.classes_, labels, affine_transformation=affine_transformation,
                                     start_label=start_label, ctx=ctx)
        if acceptable.shape[0] != len(segments):
            raise ValueError(f"the label raster holds {acceptable.shape[0]} segments, the table {len(segments)} rows")
    is_mlp = isinstance(model, MLP)
    if compute_shap and is_mlp and shap_background is None:
        raise NotImplementedError("compute_shap=True explains forests only (TreeSHAP); there is no explainer for an MLP")
    if shap_background is not None and not (compute_shap and is_mlp):
        raise ValueError("shap_background goes with compute_shap=True and an MLP: forest_shap takes no background data")
    if shap_background is not None:
        _check_shap_width(model)
    X, _, _ = standard_scale(np.ascontiguousarray(x_pred.to_numpy(dtype=np.float64)), ctx=ctx, dtype=np.float64 if is_mlp else np.float32)
    pred, margin, _ = (mlp_predict if is_mlp else forest_predict)(model, X, acceptable=None if acceptable is None else np.asarray(acceptable),
                                                                  ctx=ctx)

    segments['predicted_class'] = model.classes_[pred]
    segments['prediction_margin'] = margin
    for col in segments.columns:                      # classify.py:165-173
        if col == 'geometry' or not isinstance(segments[col].dtype, np.dtype):
            continue
        if np.issubdtype(segments[col].dtype, np.integer):
            segments[col] = segments[col].astype(pd.Int64Dtype())
        elif np.issubdtype(segments[col].dtype, np.floating):
            segments[col] = segments[col].astype(float)
    res = ClassifiedImage(segments, None, None, None, None, None, params)
    if compute_shap:
        res.shap_values, res.shap_base_values = mlp_shap(model, X, shap_background, ctx=ctx) if is_mlp else forest_shap(model, X, ctx=ctx)
    return res
