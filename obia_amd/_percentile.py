"""np.percentile / np.nanpercentile (method "linear") from the order statistics the device selects: the interpolation NumPy does on
the host, restated operation for operation, and the call of the select.  Shared by obia_amd.cost (q = 2, 98) and obia_amd.image
(any pair)."""
import ctypes

import numpy as np

from . import _lib


def quantiles(p_lo, p_hi):
    """The two percentiles as the fractions NumPy works with (np.true_divide(q, 100))."""
    return np.true_divide((p_lo, p_hi), 100.0)


def lerp(n, a, b, dtype, q):
    """np.nanpercentile(x, 100 * q) from the order statistics: a[k], b[k] = the values of rank floor(v_k) and floor(v_k) + 1
    (both the last value when v_k >= n - 1) at the virtual index v_k = (n - 1) * q_k.  NumPy's _lerp: the difference in the
    input dtype, the weight in float64, the upper half computed from b."""
    if n == 0:
        return np.full(2, np.nan, dtype)
    v = (n - 1) * q
    prev = np.floor(v)
    prev[v >= n - 1] = -1
    gamma = v - prev.astype(np.intp)
    a = np.asarray(a, dtype)
    b = np.asarray(b, dtype)
    diff = np.subtract(b, a)
    out = np.add(a, diff * gamma)
    np.subtract(b, diff * (1 - gamma), out=out, where=gamma >= 0.5, casting="unsafe", dtype=out.dtype)
    return out


def select(lib, c, plane, q):
    """(lo, hi) = np.nanpercentile(plane, 100 * q) of a float32 / float64 device plane (16-byte aligned), and the number of valid
    (non-NaN) values."""
    import torch
    f64 = plane.dtype == torch.float64
    n = ctypes.c_int64(0)
    bits = (ctypes.c_uint64 * 4)()
    _lib.check(lib.obia_cost_select_dev(c.handle, plane.data_ptr(), int(f64), plane.numel(), float(q[0]), float(q[1]),
                                        ctypes.byref(n), bits))
    raw = np.array(list(bits), np.uint64)
    vals = raw.view(np.float64) if f64 else raw.astype(np.uint32).view(np.float32)
    lohi = lerp(int(n.value), vals[[0, 2]], vals[[1, 3]], np.float64 if f64 else np.float32, q)
    return float(lohi[0]), float(lohi[1]), int(n.value)
