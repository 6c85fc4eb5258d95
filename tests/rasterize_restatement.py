"""The rasterisation rule of obia_amd.polygons.rasterize restated in NumPy float64 -- test infrastructure.

Everything is in pixel coordinates: x = column axis, y = row axis, (0, 0) = top-left corner, pixel (r, c) has its centre at
(xc, yc) = (c + 0.5, r + 0.5).  A shape is a set of rings; every ring is closed by an edge from its last vertex to its first.
An edge (x0, y0) -> (x1, y1) counts for a centre when

    (y0 <= yc) != (y1 <= yc)    and    x0 + (yc - y0) * (x1 - x0) / (y1 - y0) <= xc

and the shape covers the pixel iff an odd number of its edges count.  Shapes are burned in input order, later over earlier.
``burn`` is a plain loop over shapes with a brute-force parity over the shape's clipped bounding box; ``covers_full`` is the
same parity over the whole raster (tests/test_rasterize_restatement_cpu.py holds the two against each other).
"""
import numpy as np


def shape_edges(xy, ring_offset, rings):
    """(x0, y0, x1, y1) of every edge of the given rings, the closing edge of each ring included."""
    x0, y0, x1, y1 = [], [], [], []
    for r in rings:
        v = np.asarray(xy[ring_offset[r]:ring_offset[r + 1]], np.float64)
        if len(v) == 0:
            continue
        w = np.roll(v, -1, axis=0)
        x0.append(v[:, 0]); y0.append(v[:, 1]); x1.append(w[:, 0]); y1.append(w[:, 1])
    if not x0:
        z = np.zeros(0)
        return z, z, z, z
    return tuple(np.concatenate(a) for a in (x0, y0, x1, y1))


def _row_parity(x0, y0, x1, y1, yc, xc):
    """Coverage of the centres (xc[i], yc) of one row: odd number of counting edges."""
    sel = (y0 <= yc) != (y1 <= yc)
    if not sel.any():
        return np.zeros(len(xc), bool)
    a, b, c, d = x0[sel], y0[sel], x1[sel], y1[sel]
    xi = a + (yc - b) * (c - a) / (d - b)
    return ((xi[None, :] <= xc[:, None]).sum(1) & 1).astype(bool)


def _first_centre_ge(v):
    """First integer k with k + 0.5 >= v."""
    f = np.floor(v)
    return int(f) + (1 if f + 0.5 < v else 0)


def covers_full(edges, H, W):
    """(H, W) bool coverage of one shape, every pixel of the raster tested."""
    x0, y0, x1, y1 = edges
    out = np.zeros((H, W), bool)
    xc = np.arange(W) + 0.5
    for r in range(H):
        out[r] = _row_parity(x0, y0, x1, y1, r + 0.5, xc)
    return out


def covers_bbox(edges, H, W):
    """The same coverage, looked for only where it can be: rows whose centre lies in [ymin, ymax), columns from one before the
    first centre >= xmin to the first centre >= xmax (a crossing is a rounded value and may leave [xmin, xmax] by an ulp)."""
    x0, y0, x1, y1 = edges
    out = np.zeros((H, W), bool)
    if len(x0) == 0:
        return out
    lim = 2.0 ** 40
    xs, ys = np.clip(np.concatenate([x0, x1]), -lim, lim), np.clip(np.concatenate([y0, y1]), -lim, lim)
    r0, r1 = max(_first_centre_ge(ys.min()), 0), min(_first_centre_ge(ys.max()) - 1, H - 1)
    c0, c1 = max(_first_centre_ge(xs.min()) - 1, 0), min(_first_centre_ge(xs.max()), W - 1)
    if r0 > r1 or c0 > c1:
        return out
    xc = np.arange(c0, c1 + 1) + 0.5
    for r in range(r0, r1 + 1):
        out[r, c0:c1 + 1] = _row_parity(x0, y0, x1, y1, r + 0.5, xc)
    return out


def burn(xy, ring_offset, ring_shape, values, out_shape, fill=0, full=False):
    """(H, W) int32 raster: shapes in input order, the last covering shape wins, ``fill`` where none covers."""
    H, W = out_shape
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ring_offset = np.asarray(ring_offset, np.int64)
    ring_shape = np.asarray(ring_shape, np.int64)
    out = np.full((H, W), fill, np.int32)
    cover = covers_full if full else covers_bbox
    with np.errstate(all="ignore"):
        for s in range(len(values)):
            rings = np.nonzero(ring_shape == s)[0]
            if len(rings) == 0:
                continue
            out[cover(shape_edges(xy, ring_offset, rings), H, W)] = values[s]
    return out


def pack(shapes):
    """[[ring (n, 2), ...] per shape] -> (xy, ring_offset, ring_shape)."""
    chunks, lens, owner = [], [], []
    for s, rings in enumerate(shapes):
        for ring in rings:
            ring = np.asarray(ring, np.float64).reshape(-1, 2)
            chunks.append(ring); lens.append(len(ring)); owner.append(s)
    xy = np.concatenate(chunks) if chunks else np.zeros((0, 2))
    return xy, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.asarray(owner, np.int32)


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def star(rs, cx, cy, n, r_lo, r_hi, shuffle=False, on_centres=False):
    """Ring of n vertices around (cx, cy): angles in order (a star) or shuffled (self-intersecting); ``on_centres`` snaps the
    vertices to pixel centres, so that vertices and axis-parallel edges lie exactly on them."""
    ang = np.sort(rs.uniform(0, 2 * np.pi, n))
    if shuffle:
        rs.shuffle(ang)
    rad = rs.uniform(r_lo, r_hi, n)
    v = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
    if on_centres:
        v = np.floor(v) + 0.5
    return v
