"""From over-segmented superpixels to objects without a detector: multiresolution merging on the segment graph alone
(include/obia_merging.h).  The reference has no counterpart.  The definitions are this project's, modelled on the
fusion criterion of Baatz and Schaepe (2000), "multiresolution segmentation" -- the size-weighted growth of the spectral heterogeneity
plus the two shape terms, compactness and smoothness, against a scale parameter -- and are compared with eCognition or any other
implementation nowhere.

A :class:`RegionState` holds what a merge round needs: per segment the area, the per-band mean and ``m2`` (variance times area), the
perimeter and the box, the :class:`~obia_amd.adjacency.SegmentGraph`, and ``root``, the row every ORIGINAL segment now belongs to.
``RegionState.from_raster`` is the one pass over the raster (graph, shapes, zonal statistics).  ``fusion_cost`` is the cost of every
edge, ``merge_pairs`` merges the node tables of disjoint pairs, contracts the graph (:meth:`SegmentGraph.contract`) and composes
``root``; ``merge_regions`` runs rounds of mutual best neighbours on a state to the fixed point, and ``multiresolution_merge`` is the
whole way: the state of the raster, the rounds, and one relabel at the end.

NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out.  There is no CPU path."""
import numpy as np

from . import _device, _lib
from .adjacency import SegmentGraph, _check_labels, _ptr, compact_roots, relabel, segment_graph
from .cost import _shape

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def _need_torch():
    _device.need_torch("obia_amd.merging")


def _check_terms(shape, compactness):
    s, c = float(shape), float(compactness)
    if not 0.0 <= s <= 1.0:
        raise ValueError(f"shape must lie in [0, 1], got {shape!r}")
    if not 0.0 <= c <= 1.0:
        raise ValueError(f"compactness must lie in [0, 1], got {compactness!r}")
    return s, c


def _check_weights(band_weights, F):
    """(F) float64 on the host; ``F`` None: any length of at least 1"""
    if band_weights is None:
        return None if F is None else np.ones(F, np.float64)
    if _device.is_torch(band_weights):
        band_weights = band_weights.detach().cpu().numpy()
    w = np.asarray(band_weights, np.float64)
    if w.ndim != 1 or w.size < 1 or (F is not None and w.size != F):
        raise ValueError(f"band_weights must be one weight per band ({'F' if F is None else F}), got shape {w.shape}")
    if not (w >= 0.0).all():                                          # a NaN fails the comparison too
        raise ValueError("band_weights must be numbers >= 0")
    return w


def _check_rounds(max_rounds):
    if max_rounds is None:
        return None
    if isinstance(max_rounds, bool) or int(max_rounds) != max_rounds or int(max_rounds) < 0:
        raise ValueError(f"max_rounds must be a non-negative integer or None, got {max_rounds!r}")
    return int(max_rounds)


class RegionState:
    """The tables of include/obia_merging.h over the rows 0 .. ``n_labels`` - 1 (segment i carries the label ``start_label`` + i; N
    never changes during a run): ``area`` (N) int64, ``mean`` and ``m2`` (N, F) float64, ``perimeter`` (N) int64, ``box`` (N, 4)
    int32, ``graph``, the current :class:`SegmentGraph`, and ``root`` (N) int32.  A merged region lives at the row of its smallest
    member; the other rows are empty: zeros in the integer tables, the quiet NaN in ``mean`` and ``m2``, no entries in the graph."""

    def __init__(self, area, mean, m2, perimeter, box, graph, root=None, as_tensor=None):
        _need_torch()
        self.graph = graph
        self.n_labels, self.start_label = graph.n_labels, graph.start_label
        self._dev, self._ctx = graph._dev, graph._ctx
        self._is_t = graph._is_t if as_tensor is None else bool(as_tensor)
        N = self.n_labels
        self._area = _device.as_dev(area, torch.int64, self._dev)
        self._mean = _device.as_dev(mean, torch.float64, self._dev)
        self._m2 = _device.as_dev(m2, torch.float64, self._dev)
        self._perimeter = _device.as_dev(perimeter, torch.int64, self._dev)
        self._box = _device.as_dev(box, torch.int32, self._dev)
        self._root = (torch.arange(N, dtype=torch.int32, device=self._area.device) if root is None
                      else _device.as_dev(root, torch.int32, self._dev))
        if self._mean.dim() == 1:
            self._mean, self._m2 = self._mean.reshape(-1, 1), self._m2.reshape(-1, 1)
        if (self._mean.dim() != 2 or self._mean.shape[0] != N or self._mean.shape[1] < 1 or self._m2.shape != self._mean.shape
                or tuple(self._area.shape) != (N,) or tuple(self._perimeter.shape) != (N,) or tuple(self._box.shape) != (N, 4)
                or tuple(self._root.shape) != (N,)):
            raise ValueError(f"the tables must be area (N), mean and m2 (N, F) with F >= 1, perimeter (N), box (N, 4) and root (N) with N = {N}")
        if N * self._mean.shape[1] >= 2 ** 31:
            raise NotImplementedError("mean must have fewer than 2^31 elements")

    def _out(self, t):
        return _device.out(t, self._is_t)

    n_bands = property(lambda self: int(self._mean.shape[1]))
    area = property(lambda self: self._out(self._area))
    mean = property(lambda self: self._out(self._mean))
    m2 = property(lambda self: self._out(self._m2))
    perimeter = property(lambda self: self._out(self._perimeter))
    box = property(lambda self: self._out(self._box))
    root = property(lambda self: self._out(self._root))
    present = property(lambda self: self._out(self._area > 0), doc="(N) bool: the rows that hold a region")
    variance = property(lambda self: self._out(self._m2 / self._area.to(torch.float64)[:, None]), doc="(N, F) float64: m2 / area")

    @property
    def n_regions(self):
        return int((self._area > 0).sum())

    def shape_table(self):
        """The :class:`~obia_amd.shapes.ShapeTable` view of the regions: area, perimeter and box as they are; the moment columns
        (sums 1 .. 5) are not carried through a merge and are zero."""
        from .shapes import ShapeTable
        sums = torch.zeros((self.n_labels, _lib.SHAPE_SUMS), dtype=torch.int64, device=self._area.device)
        sums[:, 0], sums[:, 6] = self._area, self._perimeter
        return ShapeTable(sums, self._box, self.n_labels, self.start_label, as_tensor=self._is_t)

    @classmethod
    def from_raster(cls, raw, labels, bands=None, start_label=1, ctx=None):
        """The state of a label raster (H, W) over ``raw`` (H, W, C): ``segment_graph``, ``segment_shapes`` and ``zonal_stats``,
        the one pass over the pixels.  A segment with a NaN in a used band (``count != area``) is refused with ``ValueError``."""
        _need_torch()
        _check_labels(labels, start_label, None)
        from .shapes import segment_shapes
        from .statistics import zonal_stats
        is_t = _device.is_torch(labels)
        dev = _device.device_of(ctx, labels, raw)
        lab = _device.as_dev(labels, torch.int32, dev)
        r = _device.as_dev(raw, torch.float32, dev)
        g = segment_graph(lab, start_label, ctx=ctx)
        N = g.n_labels
        g = SegmentGraph(g._indptr, g._neighbor, g._border, N, start_label, ctx=ctx, as_tensor=is_t)   # it answers as the labels came in
        sh = segment_shapes(lab, start_label, n_labels=N, ctx=ctx)
        st = zonal_stats(r, lab, bands=bands, start_label=start_label, n_labels=N, ctx=ctx)
        area = sh._sums[:, 0].clone()
        F = int(st["mean"].shape[1])
        count = _device.as_dev(st["count"], torch.int64, dev)
        bad = (count != area) & (area > 0)
        # zonal_stats drops NaN pixels per band and still counts them, so the count alone does not show them: one elementwise look
        holes = torch.isnan(r if bands is None else r[:, :, [int(b) for b in bands]]).any(-1)
        if bool(holes.any()):
            seg = lab[holes].to(torch.int64) - int(start_label)
            bad[seg[(seg >= 0) & (seg < N)]] = True
        if bool(bad.any()):
            first = int(torch.nonzero(bad)[0])
            raise ValueError(f"segment {first + int(start_label)} has a NaN in a used band: its pixel count differs from its area")
        has = (area > 0)[:, None]
        nan = torch.full((1, 1), float("nan"), dtype=torch.float64, device=area.device)
        mean = _device.as_dev(st["mean"], torch.float64, dev).reshape(N, F)
        var = _device.as_dev(st["variance"], torch.float64, dev).reshape(N, F)
        m2 = torch.clamp(var * area.to(torch.float64)[:, None], min=0.0)
        return cls(area, torch.where(has, mean, nan), torch.where(has, m2, nan), sh._sums[:, 6].clone(), sh._box.clone(), g, as_tensor=is_t)


def _cost(state, w, w_color, w_compact):
    g = state.graph
    F = state.n_bands
    wd = torch.as_tensor(w, device=state._area.device)
    out = torch.empty(g.nnz, dtype=torch.float64, device=state._area.device)
    lib, c, head = g._begin()
    _lib.check(lib.obia_merge_cost_dev(*head, _ptr(g._border), g.n_labels, g.nnz, _ptr(state._area), _ptr(state._mean), _ptr(state._m2), F,
                                       wd.data_ptr(), _ptr(state._perimeter), _ptr(state._box), w_color, w_compact, _ptr(out)))
    return out


def fusion_cost(state, band_weights=None, shape=0.1, compactness=0.5):
    """(nnz) float64: the fusion cost of every edge of ``state.graph`` (include/obia_merging.h, FUSION COST): ``w_color`` = 1 -
    ``shape`` times the weighted growth of the spectral heterogeneity, ``shape`` times the growth of the compactness
    (``compactness``) and smoothness (1 - ``compactness``) terms.  NaN for a pseudo entry; ``cost[i->j]`` and ``cost[j->i]`` are the
    same bits."""
    _need_torch()
    s, c = _check_terms(shape, compactness)
    w = _check_weights(band_weights, state.n_bands)
    return state._out(_cost(state, w, 1.0 - s, c))


def _merge_pairs(state, partner):
    g, N, F = state.graph, state.n_labels, state.n_bands
    dev = state._area.device
    area, perimeter = torch.empty_like(state._area), torch.empty_like(state._perimeter)
    mean, m2, box = torch.empty_like(state._mean), torch.empty_like(state._m2), torch.empty_like(state._box)
    lib, c, head = g._begin()
    _lib.check(lib.obia_merge_pairs_dev(*head, _ptr(g._border), N, g.nnz, _ptr(partner), _ptr(state._area), _ptr(state._mean), _ptr(state._m2), F,
                                        _ptr(state._perimeter), _ptr(state._box), _ptr(area), _ptr(mean), _ptr(m2), _ptr(perimeter), _ptr(box)))
    me = torch.arange(N, dtype=torch.int64, device=dev)
    p = partner.to(torch.int64)
    inside = (p >= 0) & (p < N) & (p != me)
    valid = inside & (p[p.clamp(0, max(N - 1, 0))] == me) if N else inside
    step = torch.where(valid, torch.minimum(me, p), me).to(torch.int32)
    graph = g._contract(step)
    root = step[state._root.to(torch.int64)]
    return RegionState(area, mean, m2, perimeter, box, graph, root, as_tensor=state._is_t)


def merge_pairs(state, partner):
    """A new :class:`RegionState` in which every pair (i, ``partner[i]``) is one region at row min(i, partner[i]).  ``partner`` is (N)
    integers, -1 for none; an index outside 0 .. N - 1 and a partner that does not point back count as none."""
    _need_torch()
    p = _device.as_dev(partner, torch.int32, state._dev)
    if tuple(p.shape) != (state.n_labels,):
        raise ValueError(f"partner must be an (n_labels,) column with n_labels = {state.n_labels}, got shape {tuple(p.shape)}")
    return _merge_pairs(state, p)


def _round(state, w, w_color, w_compact, limit):
    """one round: ``(partner, pairs)``, the mutual best neighbours whose cost is at most ``limit``"""
    N = state.n_labels
    best, best_cost = state.graph._best(_cost(state, w, w_color, w_compact))
    me = torch.arange(N, dtype=torch.int64, device=best.device)
    b = best.to(torch.int64)
    mutual = (b >= 0) & (b[b.clamp(min=0)] == me) & (best_cost <= limit)
    return torch.where(mutual, best, torch.full_like(best, -1)), int(mutual.sum()) // 2


def _drive(state, w, w_color, w_compact, limit, rounds):
    """rounds to the fixed point (``rounds`` None) or ``rounds`` of them: ``(state, counts)``"""
    n = state.n_regions
    counts = []
    while rounds is None or len(counts) < rounds:
        partner, pairs = _round(state, w, w_color, w_compact, limit)
        if pairs:
            state = _merge_pairs(state, partner)
        n -= pairs
        counts.append(n)
        if not pairs:
            break
    return state, counts


def merge_regions(state, scale, band_weights=None, shape=0.1, compactness=0.5, max_rounds=None):
    """The rounds of :func:`multiresolution_merge` on a :class:`RegionState`, without the raster: ``(state, counts)``, the state at
    the fixed point (or after ``max_rounds`` rounds) and the number of regions after every round that ran.  A pure function of the
    state: the same bits for the same tables."""
    _need_torch()
    t = float(scale)
    if not t >= 0.0:
        raise ValueError(f"scale must be >= 0, got {scale!r}")
    s, c = _check_terms(shape, compactness)
    rounds = _check_rounds(max_rounds)
    w = _check_weights(band_weights, state.n_bands)
    return _drive(state, w, 1.0 - s, c, t * t, rounds)


def multiresolution_merge(raw, labels, scale, bands=None, band_weights=None, shape=0.1, compactness=0.5, max_rounds=None, start_label=1,
                          return_state=False, ctx=None):
    """Rounds of mutual best neighbours under the fusion cost.  A round takes the cost of every edge and every region's cheapest
    neighbour (ties to the lowest index); i and j merge when each is the other's best and the cost is at most ``scale ** 2``.  The
    raster is read once at the start (:meth:`RegionState.from_raster`) and written once at the end (one ``relabel``); a round works
    on the graph and the node tables alone (:func:`merge_regions`).  It stops after ``max_rounds`` rounds, by default (None) at the
    fixed point, where a round merges nothing and no real edge costs ``scale ** 2`` or less.  Returns ``(labels, counts)``: the
    raster (H, W) int32 with the objects numbered from ``start_label`` in ascending order of their smallest member, and the number
    of objects after every round that ran; with ``return_state`` also the final :class:`RegionState`, whose ``root``, ``mean``,
    ``variance``, ``shape_table()`` and ``graph`` are the objects' table without another pass."""
    _need_torch()
    _check_labels(labels, start_label, None)
    t = float(scale)
    if not t >= 0.0:
        raise ValueError(f"scale must be >= 0, got {scale!r}")
    s, c = _check_terms(shape, compactness)
    rounds = _check_rounds(max_rounds)
    if len(_shape(raw)) != 3 or tuple(_shape(raw)[:2]) != tuple(_shape(labels)):
        raise ValueError(f"raw must be an (H, W, C) raster over the labels, got shapes {_shape(raw)} and {_shape(labels)}")
    w = _check_weights(band_weights, _shape(raw)[2] if bands is None else len(list(bands)))
    is_t = _device.is_torch(labels)
    dev = _device.device_of(ctx, labels, raw)
    lab = _device.as_dev(labels, torch.int32, dev)
    state = RegionState.from_raster(raw, labels, bands=bands, start_label=start_label, ctx=ctx)
    present = state._area > 0
    state, counts = _drive(state, w, 1.0 - s, c, t * t, rounds)
    out = relabel(lab, compact_roots(state._root, start_label, present=present), start_label, ctx=ctx)
    res = (_device.out(out, is_t), counts)
    return res + (state,) if return_state else res
