"""Which segments touch each other: the segment adjacency graph of a label raster and what an object-based workflow hangs on it
(include/obia_adjacency.h).  The reference has no counterpart: its objects table holds per-segment columns only, and
its one way from superpixels to objects leads through detection boxes (``assign_fid``; here :func:`obia_amd.boxes.dissolve_by_box`).

``segment_graph`` counts, for every pair of 4-adjacent segments, the pixel edges they share -- one pass over the raster, run as a
count pass and a write pass, with the sort and the sums between them left to torch -- and returns a :class:`SegmentGraph`: a symmetric
CSR over the segments with the background and the raster's frame as two pseudo-neighbours.  On it: the squared distance of the two
ends of every edge (``d2``), border-weighted statistics of a segment's neighbours (``neighbor_stats``), its border to every class
(``border_to_class``), its nearest neighbour (``best_neighbor``) and the connected components of any link rule (``components``).
``merge_by_threshold``, ``dissolve_by_class`` and ``merge_similar`` are the three drivers: one cut at a distance, one object per run
of equal classes, rounds of mutual best neighbours.  ``context_columns`` is the second half of an OBIA feature table.

NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out; a graph answers as the raster it was made from.  There is no CPU path."""
import numpy as np

from . import _device, _lib
from .cost import _shape

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

STAT_COLUMNS = ("mean", "min", "max", "used", "diff")


def _need_torch():
    _device.need_torch("obia_amd.adjacency")


def _check_labels(labels, start_label, n_labels):
    s = _shape(labels)
    if len(s) != 2 or 0 in s:
        raise ValueError(f"labels must be a non-empty (H, W) raster, got shape {s}")
    if s[0] * s[1] >= 2 ** 31:
        raise NotImplementedError(f"labels must have fewer than 2^31 pixels, got {s[0]} x {s[1]}")
    if int(start_label) != start_label or not -2 ** 31 <= int(start_label) < 2 ** 31:
        raise ValueError(f"start_label must be an int32, got {start_label!r}")
    if n_labels is not None and (int(n_labels) != n_labels or not 0 <= int(n_labels) <= 2 ** 31 - 3):
        raise ValueError(f"n_labels must be an integer in 0 .. 2^31 - 3, got {n_labels!r}")


def _count_labels(lab, start_label, n_labels):
    n = max(int(lab.max()) - int(start_label) + 1, 0) if n_labels is None else int(n_labels)
    if n > 2 ** 31 - 3:
        raise ValueError("labels must stay below start_label + 2^31 - 3")
    return n


def _ptr(t):
    return t.data_ptr() if t.numel() else None


class SegmentGraph:
    """The symmetric CSR of include/obia_adjacency.h over the segments 0 .. ``n_labels`` - 1 (segment i carries the label
    ``start_label`` + i): ``indptr`` (N + 1) int64, ``neighbor`` (nnz) int32 ascending inside a row -- the real neighbours, then N
    (background) if present, then N + 1 (outside the raster) if present -- and ``border`` (nnz) int64, the shared pixel edges."""

    def __init__(self, indptr, neighbor, border, n_labels, start_label=1, ctx=None, as_tensor=None):
        _need_torch()
        self._is_t = _device.is_torch(indptr) if as_tensor is None else bool(as_tensor)
        self._dev = _device.device_of(ctx, indptr, neighbor, border)
        self._ctx = ctx
        self.n_labels, self.start_label = int(n_labels), int(start_label)
        self._indptr = _device.as_dev(indptr, torch.int64, self._dev)
        self._neighbor = _device.as_dev(neighbor, torch.int32, self._dev)
        self._border = _device.as_dev(border, torch.int64, self._dev)
        if self._indptr.dim() != 1 or self._indptr.numel() != self.n_labels + 1:
            raise ValueError(f"indptr must have n_labels + 1 = {self.n_labels + 1} elements, got shape {tuple(self._indptr.shape)}")
        if self._neighbor.dim() != 1 or self._neighbor.shape != self._border.shape:
            raise ValueError("neighbor and border must be one-dimensional and of one length")
        if self.nnz >= 2 ** 31:
            raise NotImplementedError("a graph must have fewer than 2^31 entries")

    # ---- the table, as the raster came in
    def _out(self, t):
        return _device.out(t, self._is_t)

    @property
    def nnz(self):
        return int(self._neighbor.numel())

    indptr = property(lambda self: self._out(self._indptr))
    neighbor = property(lambda self: self._out(self._neighbor))
    border = property(lambda self: self._out(self._border))

    def _real(self):
        return self._neighbor < self.n_labels

    def _rows(self):
        """the row of every entry, (nnz) int64"""
        n = self._indptr[1:] - self._indptr[:-1]
        return torch.repeat_interleave(torch.arange(self.n_labels, dtype=torch.int64, device=n.device), n)

    def _row_sum(self, x):
        """(N) int64: the sum of the int64 column ``x`` (nnz) over every row, by differences of one running sum"""
        run = torch.cat([torch.zeros(1, dtype=torch.int64, device=x.device), torch.cumsum(x.to(torch.int64), 0)])
        return run[self._indptr[1:]] - run[self._indptr[:-1]]

    real = property(lambda self: self._out(self._real()), doc="(nnz) bool: the entries whose neighbour is a segment")
    rows = property(lambda self: self._out(self._rows()), doc="(nnz) int64: the row of every entry")
    n_neighbors = property(lambda self: self._out(self._row_sum(self._real())), doc="(N) int64: real neighbours of every segment")
    perimeter = property(lambda self: self._out(self._row_sum(self._border)), doc="(N) int64: pixel edges around every segment")
    border_background = property(lambda self: self._out(self._row_sum(self._border * (self._neighbor == self.n_labels))))
    border_frame = property(lambda self: self._out(self._row_sum(self._border * (self._neighbor == self.n_labels + 1))))
    border_segments = property(lambda self: self._out(self._row_sum(self._border * self._real())))

    # ---- the table kernels
    def _values(self, values):
        v = _device.as_dev(values, torch.float64, self._dev)
        if v.dim() == 1:
            v = v.reshape(-1, 1)
        if v.dim() != 2 or v.shape[0] != self.n_labels or v.shape[1] < 1:
            raise ValueError(f"values must be an (n_labels, F) table with n_labels = {self.n_labels} and F >= 1, got shape {tuple(v.shape)}")
        if self.n_labels * v.shape[1] >= 2 ** 31:
            raise NotImplementedError("values must have fewer than 2^31 elements")
        return v.contiguous()

    def _begin(self):
        lib, c = _device.begin(self._dev, self._ctx)
        return lib, c, (c.handle, _ptr(self._indptr), _ptr(self._neighbor))

    def _d2(self, values):
        v = self._values(values)
        out = torch.empty(self.nnz, dtype=torch.float64, device=v.device)
        lib, c, head = self._begin()
        _lib.check(lib.obia_adj_edge_d2_dev(*head, self.n_labels, self.nnz, _ptr(v), v.shape[1], _ptr(out)))
        return out

    def d2(self, values):
        """(nnz) float64: the squared distance of the rows of ``values`` (N, F) at the two ends of every edge, summed in ascending
        f; NaN for a pseudo entry.  ``d2[i->j]`` and ``d2[j->i]`` are the same bits."""
        return self._out(self._d2(values))

    def weights(self, values):
        """``sqrt(d2)``, for people: the Euclidean distance of the two ends of every edge"""
        return self._out(torch.sqrt(self._d2(values)))

    def neighbor_stats(self, values):
        """Statistics of every segment's real neighbours, per column of ``values`` (N, F): a dict of ``mean`` (weighted by the shared
        border), ``min``, ``max`` (float64), ``used`` (int32, the neighbours whose value is not NaN) and ``diff`` = values - mean,
        (N, F) each.  A segment without such a neighbour gets NaN."""
        v = self._values(values)
        N, F = v.shape
        mean, mn, mx = (torch.empty((N, F), dtype=torch.float64, device=v.device) for _ in range(3))
        used = torch.empty((N, F), dtype=torch.int32, device=v.device)
        lib, c, head = self._begin()
        _lib.check(lib.obia_adj_neighbor_stats_dev(*head, _ptr(self._border), N, self.nnz, _ptr(v), F, _ptr(mean), _ptr(mn), _ptr(mx), _ptr(used)))
        diff = v - mean
        diff = torch.where(diff != diff, torch.full_like(diff, float("nan")), diff)      # every NaN the quiet NaN, as the kernels write it
        return self._out(dict(zip(STAT_COLUMNS, (mean, mn, mx, used, diff))))

    def border_to_class(self, classes, n_classes):
        """(N, n_classes) int64: the pixel edges every segment shares with the segments of class k; ``classes`` (N) integers, those
        outside 0 .. n_classes - 1 add nothing."""
        K = int(n_classes)
        if K < 1:
            raise ValueError(f"n_classes must be at least 1, got {n_classes!r}")
        if self.n_labels * K >= 2 ** 31:
            raise NotImplementedError("n_labels * n_classes must be below 2^31")
        cls = _device.as_dev(classes, torch.int32, self._dev)
        if tuple(cls.shape) != (self.n_labels,):
            raise ValueError(f"classes must be an (n_labels,) column, got shape {tuple(cls.shape)}")
        out = torch.empty((self.n_labels, K), dtype=torch.int64, device=cls.device)
        lib, c, head = self._begin()
        _lib.check(lib.obia_adj_class_border_dev(*head, _ptr(self._border), self.n_labels, self.nnz, _ptr(cls), K, _ptr(out)))
        return self._out(out)

    def _entry_column(self, x, dtype, what):
        t = _device.as_dev(x, dtype, self._dev)
        if tuple(t.shape) != (self.nnz,):
            raise ValueError(f"{what} must be an (nnz,) column with nnz = {self.nnz}, got shape {tuple(t.shape)}")
        return t

    def _best(self, d2):
        d = self._entry_column(d2, torch.float64, "d2")
        best = torch.empty(self.n_labels, dtype=torch.int32, device=d.device)
        best_d2 = torch.empty(self.n_labels, dtype=torch.float64, device=d.device)
        lib, c, head = self._begin()
        _lib.check(lib.obia_adj_best_neighbor_dev(*head, self.n_labels, self.nnz, _ptr(d), _ptr(best), _ptr(best_d2)))
        return best, best_d2

    def best_neighbor(self, d2):
        """``(best, best_d2)``: per segment the real neighbour of the smallest ``d2`` that is not NaN, ties to the lowest index, -1
        and NaN when there is none.  (N) int32 and float64."""
        return self._out(self._best(d2))

    def _components(self, link):
        if _device.is_torch(link):
            ln = (link.to(f"cuda:{self._dev}") != 0).to(torch.uint8).contiguous()
        else:
            ln = torch.as_tensor(np.ascontiguousarray(np.asarray(link) != 0).view(np.uint8), device=f"cuda:{self._dev}")
        if tuple(ln.shape) != (self.nnz,):
            raise ValueError(f"link must be an (nnz,) column with nnz = {self.nnz}, got shape {tuple(ln.shape)}")
        root = torch.empty(self.n_labels, dtype=torch.int32, device=ln.device)
        lib, c, head = self._begin()
        _lib.check(lib.obia_adj_components_dev(*head, self.n_labels, self.nnz, _ptr(ln), _ptr(root)))
        return root

    def components(self, link):
        """``root`` (N) int32: the smallest index of every segment's component when i and j are linked wherever ``link`` (nnz),
        taken as a truth value, is set on i->j or on j->i.  Pseudo entries link nothing."""
        return self._out(self._components(link))

    def _contract(self, root):
        """the three calls of include/obia_merging.h, CONTRACTION, with torch's prefix sums between them; ``root`` (N) int32 on the
        device, already checked"""
        N, nnz, dev = self.n_labels, self.nnz, self._indptr.device
        raw = torch.empty(N, dtype=torch.int64, device=dev)
        lib, c, head = self._begin()
        _lib.check(lib.obia_merge_contract_rows_dev(c.handle, _ptr(self._indptr), N, nnz, _ptr(root), _ptr(raw)))
        raw_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        raw_ptr[1:] = torch.cumsum(raw, 0)
        key_work = torch.empty(nnz, dtype=torch.int32, device=dev)
        border_work = torch.empty(nnz, dtype=torch.int64, device=dev)
        cursor = torch.empty(N, dtype=torch.int32, device=dev)
        count = torch.empty(N, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()                 # raw_ptr is complete before the context's stream reads it
        _lib.check(lib.obia_merge_contract_count_dev(*head, _ptr(self._border), N, nnz, _ptr(root), _ptr(raw_ptr), _ptr(key_work), _ptr(border_work),
                                                     _ptr(cursor), _ptr(count)))
        indptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        indptr[1:] = torch.cumsum(count.to(torch.int64), 0)
        total = int(indptr[-1])                                      # (waits for torch's stream: indptr is complete)
        neighbor = torch.empty(total, dtype=torch.int32, device=dev)
        border = torch.empty(total, dtype=torch.int64, device=dev)
        _lib.check(lib.obia_merge_contract_write_dev(c.handle, N, nnz, _ptr(raw_ptr), _ptr(count), _ptr(key_work), _ptr(border_work), _ptr(indptr),
                                                     total, _ptr(neighbor), _ptr(border)))
        return SegmentGraph(indptr, neighbor, border, N, self.start_label, ctx=self._ctx, as_tensor=self._is_t)

    def contract(self, root):
        """The graph of the objects ``root`` (N) forms -- ``root[i]`` is the row the segment i goes to, with ``root[root[i]] ==
        root[i]``, as :meth:`components` gives it -- without another pass over the raster (include/obia_merging.h, CONTRACTION): row
        r holds the entries of all its members with every neighbour mapped through ``root``, the entries inside an object dropped
        and equal neighbours combined, their borders added.  Every other row is empty; ``n_labels`` and ``start_label`` stay.  It
        equals ``segment_graph(relabel(labels, root + start_label), start_label, n_labels=N)`` array for array, and is the graph
        counterpart of :meth:`obia_amd.shapes.ShapeTable.merge`."""
        N = self.n_labels
        r = _device.as_dev(root, torch.int32, self._dev)
        if tuple(r.shape) != (N,):
            raise ValueError(f"root must be an (n_labels,) column with n_labels = {N}, got shape {tuple(r.shape)}")
        if N:
            r64 = r.to(torch.int64)
            if int(r64.min()) < 0 or int(r64.max()) >= N:
                raise ValueError("root must hold rows 0 .. n_labels - 1")
            if not bool((r64[r64] == r64).all()):
                raise ValueError("root must satisfy root[root[i]] == root[i]")
        return self._contract(r)


def segment_graph(labels, start_label=1, n_labels=None, ctx=None):
    """The :class:`SegmentGraph` of a label raster (H, W): label l is segment l - ``start_label`` when that lies in 0 .. ``n_labels``
    - 1 (default: up to the largest label), every other value is background.  4-connectivity."""
    _need_torch()
    _check_labels(labels, start_label, n_labels)
    dev = _device.device_of(ctx, labels)
    lab = _device.as_dev(labels, torch.int32, dev)
    N = _count_labels(lab, start_label, n_labels)
    H, W = lab.shape
    n_tiles = -(-H // _lib.ADJ_TILE_H) * -(-W // _lib.ADJ_TILE_W)
    lib, c = _device.begin(dev, ctx)
    count = torch.empty(n_tiles, dtype=torch.int32, device=lab.device)
    _lib.check(lib.obia_adj_tile_count_dev(c.handle, lab.data_ptr(), H, W, int(start_label), N, count.data_ptr()))
    count = count.to(torch.int64)
    offset = torch.cumsum(count, 0) - count
    total = int(count.sum())                                         # (waits for torch's stream: offset is complete)
    if total >= 2 ** 31:
        raise NotImplementedError(f"the tiles of the raster hold {total} records; fewer than 2^31 are supported")
    key = torch.empty(total, dtype=torch.int64, device=lab.device)
    edges = torch.empty(total, dtype=torch.int32, device=lab.device)
    work = torch.empty(_lib.ADJ_WORK, dtype=torch.int32, device=lab.device)
    _lib.check(lib.obia_adj_tile_write_dev(c.handle, lab.data_ptr(), H, W, int(start_label), N, offset.data_ptr(), total, _ptr(key), _ptr(edges),
                                           work.data_ptr()))
    indptr, neighbor, border = _csr_of_records(key, edges, N)
    return SegmentGraph(indptr, neighbor, border, N, start_label, ctx=ctx, as_tensor=_device.is_torch(labels))


def _csr_of_records(key, edges, N):
    """directed records (key = src (N + 2) + dst, edges) of all tiles -> the CSR: a sort of the keys, an integer sum over every run
    of equal keys, the row starts from the sorted sources.  Integers only: the same bits whatever order the records came in."""
    dev = key.device
    if key.numel() == 0:
        return (torch.zeros(N + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.int64, device=dev))
    skey, order = torch.sort(key)
    uniq, runs = torch.unique_consecutive(skey, return_counts=True)
    last = torch.cumsum(runs, 0) - 1
    run = torch.cumsum(edges[order].to(torch.int64), 0)[last]
    border = run - torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), run[:-1]])
    src = torch.div(uniq, N + 2, rounding_mode="floor")
    neighbor = (uniq - src * (N + 2)).to(torch.int32)
    indptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(src, minlength=N), 0)
    return indptr, neighbor, border


def compact_roots(root, start_label=1, present=None):
    """``map`` (N) int32 from ``root`` (N): the components numbered ``start_label``, ``start_label`` + 1, ... in ascending order of
    their roots.  ``present`` (N) bool: only the components with a present member are numbered, the members of the others get
    ``start_label`` - 1 -- the drivers pass the segments that have pixels, so a label nobody carries takes no number."""
    _need_torch()
    is_t = _device.is_torch(root)
    dev = _device.device_of(None, root, present)
    r = _device.as_dev(root, torch.int64, dev)
    if r.dim() != 1:
        raise ValueError(f"root must be one-dimensional, got shape {tuple(r.shape)}")
    has = torch.ones(r.numel(), dtype=torch.bool, device=r.device)
    if present is not None:
        p = _device.as_dev(present, torch.int32, dev) != 0
        if p.shape != r.shape:
            raise ValueError(f"present must have the shape of root, got {tuple(p.shape)}")
        has = torch.zeros(r.numel(), dtype=torch.bool, device=r.device)
        has[r[p]] = True
    counted = (r == torch.arange(r.numel(), dtype=torch.int64, device=r.device)) & has
    rank = torch.cumsum(counted.to(torch.int64), 0) - 1 + int(start_label)
    return _device.out(torch.where(has[r], rank[r], torch.full_like(r, int(start_label) - 1)).to(torch.int32), is_t)


def relabel(labels, map, start_label=1, ctx=None):
    """``map[l - start_label]`` for every segment pixel of ``labels``, ``map`` (N) int32; a background value below ``start_label``
    is kept, one past the table becomes ``start_label`` - 1.  (H, W) int32."""
    _need_torch()
    _check_labels(labels, start_label, None)
    if len(_shape(map)) != 1 or _shape(map)[0] > 2 ** 31 - 3:
        raise ValueError(f"map must be an (n_labels,) table, got shape {_shape(map)}")
    dev = _device.device_of(ctx, labels, map)
    lab = _device.as_dev(labels, torch.int32, dev)
    m = _device.as_dev(map, torch.int32, dev)
    out = torch.empty_like(lab)
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_adj_relabel_dev(c.handle, lab.data_ptr(), lab.numel(), int(start_label), m.numel(), _ptr(m), out.data_ptr()))
    return _device.out(out, _device.is_torch(labels))


def _merge(lab, g, root, start_label, ctx):
    """the raster relabelled by the components ``root`` of the graph ``g`` and the number of components that have pixels"""
    m = compact_roots(root, start_label, present=g._row_sum(g._border) > 0)      # a segment with a pixel has an edge around it
    n = max(int(m.max()) - int(start_label) + 1, 0) if m.numel() else 0
    return relabel(lab, m, start_label, ctx=ctx), n


def _means(raw_or_values, lab, bands, start_label, N, ctx):
    """(N, F) float64 on the device: a table as it is, a raster (H, W, C) through the means of zonal_stats"""
    if len(_shape(raw_or_values)) == 3:
        from .statistics import zonal_stats
        raw = _device.as_dev(raw_or_values, torch.float32, lab.device.index or 0)
        return zonal_stats(raw, lab, bands=bands, start_label=start_label, n_labels=N, ctx=ctx)["mean"]
    if bands is not None:
        raise ValueError("bands select from a raster (H, W, C); a table of values is taken whole")
    return raw_or_values


def merge_by_threshold(raw_or_values, labels, threshold, bands=None, start_label=1, ctx=None):
    """One cut: adjacent segments whose means lie within ``threshold`` of each other (Euclidean, over the bands) are linked, the
    components of those links become the new segments.  ``raw_or_values``: the raster (H, W, C), whose per-segment means are taken
    with ``zonal_stats``, or an (N, F) table of values.  Returns ``(labels, n)``: the relabelled raster (H, W) int32 with the
    components numbered from ``start_label`` in ascending order of their smallest member, and their number.  The comparison is
    ``d2 <= threshold ** 2``; an edge with a NaN at either end links nothing."""
    _need_torch()
    _check_labels(labels, start_label, None)
    t = float(threshold)
    if not t >= 0.0:
        raise ValueError(f"threshold must be >= 0, got {threshold!r}")
    is_t = _device.is_torch(labels)
    dev = _device.device_of(ctx, labels, raw_or_values)
    lab = _device.as_dev(labels, torch.int32, dev)
    g = segment_graph(lab, start_label, ctx=ctx)
    d2 = g._d2(_means(raw_or_values, lab, bands, start_label, g.n_labels, ctx))
    out, n = _merge(lab, g, g._components(d2 <= t * t), start_label, ctx)
    return _device.out(out, is_t), n


def dissolve_by_class(labels, classes, start_label=1, ctx=None):
    """Adjacent segments of one class become one object: i and j are linked when ``classes[i] == classes[j] >= 0``.  ``classes``:
    (N) integers, N the number of labels from ``start_label`` to the largest.  Returns ``(labels, n)`` as
    :func:`merge_by_threshold` does."""
    _need_torch()
    _check_labels(labels, start_label, None)
    is_t = _device.is_torch(labels)
    dev = _device.device_of(ctx, labels, classes)
    lab = _device.as_dev(labels, torch.int32, dev)
    g = segment_graph(lab, start_label, ctx=ctx)
    cls = _device.as_dev(classes, torch.int64, dev)
    if tuple(cls.shape) != (g.n_labels,):
        raise ValueError(f"classes must be an (n_labels,) column with n_labels = {g.n_labels}, got shape {tuple(cls.shape)}")
    link = torch.zeros(g.nnz, dtype=torch.bool, device=lab.device)
    if g.nnz and g.n_labels:
        real = g._real()
        mine, theirs = cls[g._rows()], cls[g._neighbor.to(torch.int64).clamp(max=g.n_labels - 1)]
        link = real & (mine == theirs) & (mine >= 0)
    out, n = _merge(lab, g, g._components(link), start_label, ctx)
    return _device.out(out, is_t), n


def merge_similar(raw, labels, threshold, bands=None, max_rounds=8, start_label=1, stats=None, ctx=None):
    """Rounds of mutual best neighbours.  A round takes the per-segment means (``zonal_stats`` of ``raw`` over ``bands``, or
    ``stats(raw, labels)``, an (N, F) table), the graph, ``d2`` and every segment's best neighbour; i and j merge when each is the
    other's best and ``d2 <= threshold ** 2``.  Such pairs are disjoint, so the pair becomes min(i, j) and the segments are
    renumbered from ``start_label``.  It stops after ``max_rounds`` rounds or when a round merges nothing.  Returns ``(labels,
    counts)``: the raster (H, W) int32 and the number of segments after every round that ran."""
    _need_torch()
    _check_labels(labels, start_label, None)
    t = float(threshold)
    if not t >= 0.0:
        raise ValueError(f"threshold must be >= 0, got {threshold!r}")
    if int(max_rounds) != max_rounds or int(max_rounds) < 0:
        raise ValueError(f"max_rounds must be a non-negative integer, got {max_rounds!r}")
    is_t = _device.is_torch(labels)
    dev = _device.device_of(ctx, labels, raw)
    lab = _device.as_dev(labels, torch.int32, dev)
    r = _device.as_dev(raw, torch.float32, dev)
    counts = []
    for _ in range(int(max_rounds)):
        g = segment_graph(lab, start_label, ctx=ctx)
        N = g.n_labels
        values = stats(r, lab) if stats is not None else _means(r, lab, bands, start_label, N, ctx)
        best, best_d2 = g._best(g._d2(values))
        me = torch.arange(N, dtype=torch.int64, device=lab.device)
        b = best.to(torch.int64)
        mutual = (b >= 0) & (b[b.clamp(min=0)] == me) & (best_d2 <= t * t)
        root = torch.where(mutual, torch.minimum(me, b), me)
        merged = int(mutual.sum()) // 2
        lab, n = _merge(lab, g, root, start_label, ctx)
        counts.append(n)
        if not merged:
            break
    return _device.out(lab, is_t), counts


def context_columns(objects, graph, columns=None):
    """The context half of an objects table: a DataFrame aligned with the rows of ``create_objects`` -- the segments that have
    pixels, in ascending label order -- with ``n_neighbors``, ``perimeter`` (pixel edges), ``rel_border_background`` and
    ``rel_border_frame`` (shares of the perimeter) and, for every column c of ``columns`` (default: every numeric column but
    ``segment_id``), ``c_nb_mean``, ``c_nb_diff``, ``c_nb_min`` and ``c_nb_max`` of :meth:`SegmentGraph.neighbor_stats`."""
    import pandas as pd
    N = graph.n_labels
    perimeter = np.asarray(_device.out(graph._row_sum(graph._border), False))
    present = perimeter > 0                                           # a segment with a pixel has an edge around it
    if int(present.sum()) != len(objects):
        raise ValueError(f"the table has {len(objects)} rows, the graph {int(present.sum())} segments with pixels")
    if columns is None:
        columns = [c for c in objects.columns if c not in ("segment_id", "geometry") and pd.api.types.is_numeric_dtype(objects[c])]
    columns = list(columns)
    data = {"n_neighbors": np.asarray(_device.out(graph._row_sum(graph._real()), False))[present], "perimeter": perimeter[present]}
    per = perimeter[present].astype(np.float64)
    data["rel_border_background"] = np.asarray(_device.out(graph._row_sum(graph._border * (graph._neighbor == N)), False))[present] / per
    data["rel_border_frame"] = np.asarray(_device.out(graph._row_sum(graph._border * (graph._neighbor == N + 1)), False))[present] / per
    if columns:
        values = np.full((N, len(columns)), np.nan, np.float64)
        values[present] = objects[columns].to_numpy(dtype=np.float64)
        st = _device.out(SegmentGraph.neighbor_stats(graph, values), False) if graph._is_t else graph.neighbor_stats(values)
        for k, c in enumerate(columns):
            for name in ("mean", "diff", "min", "max"):
                data[f"{c}_nb_{name}"] = np.asarray(st[name])[present, k]
    return pd.DataFrame(data, index=objects.index)
