"""Contiguous views that start off a 16-byte boundary (test helper, not a conftest).

A fresh torch / NumPy allocation starts on a boundary of 64 bytes or more, so a test that only ever passes fresh allocations never takes
the library's branches for a misaligned base pointer ("Buffer alignment").  `offset_view(t, k)` copies `t` into a larger
flat buffer `k` elements past its start and hands back that slice in `t`'s shape: the same values, contiguous, and a `data_ptr()` that
is `k * itemsize` bytes past the buffer's -- what a caller gets from `flat[k:]` or from a row slab `img[r0:r1]` of a raster."""
import numpy as np

PAD = 16      # elements kept behind the view, so that a read a little past the end stays inside the buffer


def offset_view(t, k):
    """`t` (torch tensor, any device) copied to elements [k, k + numel) of a fresh flat buffer of numel + k + PAD elements; returns
    the slice viewed in t's shape.  The elements around it are zero."""
    import torch
    k = int(k)
    assert k >= 0
    n = t.numel()
    buf = torch.zeros(n + k + PAD, dtype=t.dtype, device=t.device)
    buf[k:k + n].copy_(t.reshape(-1))
    view = buf[k:k + n].view(t.shape)
    assert view.is_contiguous()
    assert view.data_ptr() % 16 == (buf.data_ptr() + k * t.element_size()) % 16
    assert view.data_ptr() == buf.data_ptr() + k * t.element_size()
    return view


def offset_array(a, k):
    """The NumPy twin, for the host-pointer entry points."""
    a = np.asarray(a)
    k = int(k)
    assert k >= 0
    n = a.size
    buf = np.zeros(n + k + PAD, dtype=a.dtype)
    buf[k:k + n] = a.reshape(-1)
    view = buf[k:k + n].reshape(a.shape)
    assert view.flags["C_CONTIGUOUS"] and view.base is not None
    assert view.ctypes.data % 16 == (buf.ctypes.data + k * a.itemsize) % 16
    assert view.ctypes.data == buf.ctypes.data + k * a.itemsize
    return view


def residue(x, mod=16):
    """Address of the first element modulo `mod` (torch tensor or NumPy array)."""
    return (x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data) % mod
