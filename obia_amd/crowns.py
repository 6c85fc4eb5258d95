"""Crowns from seeds: ``cost_allocation`` and ``grow_crowns`` (include/obia_crowns.h).

The reference writes a seed layer (obia/utils/seeds.py) and a cost raster (obia/utils/cost.py) and has no module that uses the two
together.  This one does: every canopy pixel goes to the seed it is cheapest to reach along a path over the pixel grid, a step
between two neighbouring pixels costing ``length * (1.0 + weight * mean cost of the two)`` -- the reference's seed metric
(seeds.py:163) taken along the path instead of along a straight line.  That is marker-controlled growth over the cost surface, also
known as cost allocation; with the canonical clusters as markers a segment is a crown.  The label raster goes straight into
``polygonize``, ``segments_table``, ``create_objects``, ``write_segments_gpkg`` and ``classify``.

The results are exact: the distance is, bit for bit, what Dijkstra's algorithm computes in float64, and ties between seeds go to the
lowest id.  Both run in libobia_hip.so (crowns.hip).  NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out; there is no CPU path.

A crown whose seeds lie apart may come out as two pieces (the seeds of a canonical cluster are linked by a straight-line distance, the
crown grows along paths); ``polygonize`` then gives it a multi-part geometry."""
import ctypes
import math

import numpy as np

from . import _device, _lib
from .cost import _is_path, _plane, _shape

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def _pixel_size(pixel_size):
    """(sy, sx) from a number or a pair (sy, sx)"""
    try:
        sy, sx = (float(pixel_size),) * 2 if np.ndim(pixel_size) == 0 else [float(v) for v in pixel_size]
    except (TypeError, ValueError):
        raise ValueError(f"pixel_size must be a positive number or a pair (sy, sx), got {pixel_size!r}") from None
    if not (math.isfinite(sy) and math.isfinite(sx) and sy > 0 and sx > 0):
        raise ValueError(f"pixel_size must be a positive number or a pair (sy, sx), got {pixel_size!r}")
    return sy, sx


def _check_args(weight, connectivity, max_dist):
    if not (isinstance(weight, (int, float, np.integer, np.floating)) and math.isfinite(weight) and weight >= 0):
        raise ValueError(f"weight must be a finite number >= 0, got {weight!r}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    if max_dist is not None and not float(max_dist) >= 0:
        raise ValueError(f"max_dist must be None or a number >= 0, got {max_dist!r}")


def cost_allocation(cost, seed_rows, seed_cols, seed_ids, mask=None, weight=0.5, pixel_size=1.0, connectivity=8, max_dist=None,
                    ctx=None):
    """Shortest-path distance to the nearest seed over the cost surface, and the id of that seed.

    cost : (H, W) array or CUDA tensor, taken as float32.  A NaN or an infinite cost is a barrier; a negative one raises ValueError.
    seed_rows, seed_cols, seed_ids : n pixel positions and their ids (int32, >= 1).  A seed on a barrier or outside the raster is
        ignored; if none is left the call raises ValueError.  Seeds of one id grow one segment.
    mask : (H, W), non-zero = passable; None = every pixel.
    weight, pixel_size (a number or (sy, sx)), connectivity (4 or 8): a step from pixel u to a neighbour v costs, in float64,
        ``len * (1.0 + weight * (0.5 * (cost[u] + cost[v])))`` with len = sx, sy or sqrt(sx^2 + sy^2).
    max_dist : pixels farther than this from every seed are left out.
    Returns (dist, labels): float64 (H, W), +inf where no seed reaches (barriers included); int32 (H, W), 0 there.  Where two seeds
    are equally far the lower id wins, so the result depends on nothing but the inputs."""
    _device.need_torch("obia_amd.crowns")
    shape = _shape(cost)
    if len(shape) != 2 or 0 in shape:
        raise ValueError(f"cost must be a non-empty (H, W) raster, got shape {shape}")
    if mask is not None and _shape(mask) != shape:
        raise ValueError(f"the mask is {_shape(mask)}, the cost raster {shape}")
    n = _shape(seed_rows)
    if len(n) != 1 or _shape(seed_cols) != n or _shape(seed_ids) != n:
        raise ValueError(f"seed_rows, seed_cols and seed_ids must be 1-D and of one length, got {n}, {_shape(seed_cols)} and "
                         f"{_shape(seed_ids)}")
    if n[0] == 0:
        raise ValueError("no seeds")
    _check_args(weight, connectivity, max_dist)
    sy, sx = _pixel_size(pixel_size)
    if shape[0] * shape[1] > 2 ** 31 - 1:
        raise NotImplementedError("cost has 2^31 pixels or more")
    is_t = _device.is_torch(cost)
    dev = _device.device_of(ctx, cost, mask, seed_rows, seed_cols, seed_ids)
    cst = _device.as_dev(cost, torch.float32, dev)
    msk = None if mask is None else _lib.mask_bytes(mask, device=cst.device)
    rc = torch.stack([_device.as_dev(seed_rows, torch.int32, dev), _device.as_dev(seed_cols, torch.int32, dev)], 1).contiguous()
    ids = _device.as_dev(seed_ids, torch.int32, dev)
    H, W = shape
    dist = torch.empty((H, W), dtype=torch.float64, device=cst.device)
    labels = torch.empty((H, W), dtype=torch.int32, device=cst.device)
    lib, c = _device.begin(dev, ctx)
    _lib.check(lib.obia_crowns_allocate_dev(c.handle, cst.data_ptr(), None if msk is None else msk.data_ptr(), H, W, rc.data_ptr(),
                                            ids.data_ptr(), int(n[0]), float(weight), sx, sy, math.sqrt(sx * sx + sy * sy),
                                            int(connectivity), -1.0 if max_dist is None else float(max_dist), dist.data_ptr(),
                                            labels.data_ptr(), (ctypes.c_int32 * 2)()))
    return _device.out((dist, labels), is_t)


def grow_crowns(cost_surface, seeds, mask=None, cost_affine=None, by="cluster", weight=0.5, connectivity=8, max_dist=None,
                return_distance=False, ctx=None):
    """One segment per canonical cluster: the crowns that grow from the seeds of ``make_canonical_seeds`` over the cost surface of
    ``make_cost_surface``.

    cost_surface : (H, W) array / CUDA tensor or a raster path (GDAL).
    seeds : the dict ``make_canonical_seeds`` returns (x, y, id, cluster) or the ``.gpkg`` layer it wrote.
    mask : the canopy mask, (H, W), non-zero = canopy; None = every pixel.
    cost_affine : [a, b, d, e, xoff, yoff] of the cost raster; None = pixel coordinates.  A seed's pixel is the one that contains
        (x, y) -- the floor of the inverse transformation; the pixel size is (|e|, |a|), in whose units ``max_dist`` is.  A rotated
        raster (b or d not 0) raises ValueError.
    by : "cluster" = one crown per canonical cluster, "id" = one per seed.
    Returns the int32 label raster: crown ids 1..N in ascending order of the cluster (seed) id -- the numbering ``create_objects`` and
    ``zonal_stats`` expect --, 0 outside the canopy mask and beyond ``max_dist``; with ``return_distance`` the pair (labels, dist).
    N counts every cluster of the table; one whose seeds all lie on barriers or off the raster has no pixel.  A crown whose seeds
    lie apart may be two pieces: ``polygonize`` gives it a multi-part geometry."""
    _device.need_torch("obia_amd.crowns")
    if by not in ("cluster", "id"):
        raise ValueError(f'by must be "cluster" or "id", got {by!r}')
    _check_args(weight, connectivity, max_dist)
    a, b, d, e, _, _ = affine = [float(v) for v in (cost_affine if cost_affine is not None else (1, 0, 0, 1, 0, 0))]
    if b != 0.0 or d != 0.0:
        raise ValueError(f"grow_crowns needs an unrotated cost raster, got the affine transformation {affine}")
    from .consumers import invert_affine
    ia, _, _, ie, c0, r0 = invert_affine(affine)
    if _is_path(seeds):
        from .seeds import read_seed_points
        seeds = read_seed_points(seeds)
    if not isinstance(seeds, dict) or "x" not in seeds or "y" not in seeds or by not in seeds:
        raise ValueError(f"seeds must be a dict with x, y and {by} (what make_canonical_seeds returns) or a .gpkg path of such a layer")
    cost_surface = _plane(cost_surface, None, "cost_surface")
    if 0 in _shape(cost_surface):
        raise ValueError("cost_surface is empty")
    H, W = _shape(cost_surface)
    dev = _device.device_of(ctx, cost_surface, mask, seeds["x"], seeds["y"], seeds[by])
    x, y = _device.as_dev(seeds["x"], torch.float64, dev), _device.as_dev(seeds["y"], torch.float64, dev)
    key = _device.as_dev(seeds[by], torch.int64, dev)
    if x.ndim != 1 or x.shape != y.shape or x.shape != key.shape:
        raise ValueError(f"the seed columns x, y and {by} must be 1-D and of one length")
    if x.numel() == 0:
        raise ValueError("no seeds")
    cols = torch.floor(ia * x + c0).clamp(-1, W).to(torch.int32)             # -1 and W: off the raster, ignored
    rows = torch.floor(ie * y + r0).clamp(-1, H).to(torch.int32)
    ids = torch.unique(key, sorted=True, return_inverse=True)[1].to(torch.int32) + 1
    cst = cost_surface if _device.is_torch(cost_surface) else _device.as_dev(cost_surface, torch.float32, dev)
    dist, labels = cost_allocation(cst, rows, cols, ids, mask=mask, weight=weight, pixel_size=(abs(e), abs(a)), connectivity=connectivity,
                                   max_dist=max_dist, ctx=ctx)
    return _device.out((labels, dist) if return_distance else labels, _device.is_torch(cost_surface))
