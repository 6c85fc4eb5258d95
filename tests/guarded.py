"""Output buffers with poisoned guards on both sides (test helper, not a conftest).

A test that judges only what lies inside an output buffer cannot see a write next to it, and cannot tell an element the call wrote from
one that still holds what an earlier call left there ("Output buffers").  `guarded(shape, dtype, poison, device, k)` makes one
flat byte buffer

    | guard | k elements of slack | payload (shape, dtype) | guard |

in which EVERY byte is `poison`, and hands out the payload as a contiguous tensor (device "cuda" / "cpu") or NumPy array (device
"numpy": the host entry points).  The payload starts `k * itemsize` bytes past a 16-byte boundary, like the views of
tests/offset_views.py.  After the call under test:

  * `stray()`      offsets of the guard and slack bytes that no longer hold `poison`, counted from the payload's edges: -1 is the byte
                   just before the first payload byte (the slack, then the front guard), 0 the first byte past the end;
  * `unwritten()`  flat indices of the payload elements whose bytes ALL still equal `poison`;
  * `findings()`   both as a list of sentences: a test asserts that it is empty.

The guard is a condition, not a measurement: on each side the larger of 4096 bytes -- one 256-lane workgroup of 16-byte stores -- and
two rows of the payload (a row: everything but the first dimension), so that a row index off by one lands inside it.

`snapshot(t)` / `unchanged(t, snap)` compare an input byte for byte before and after a call."""
import numpy as np

GUARD_MIN = 4096
POISONS = (0xA5, 0x5A)        # int32 -1515870811 / 1515870810; finite float32 / float64 of no meaning; as uint8 neither 0 nor 1


def _np_dtype(dtype):
    if isinstance(dtype, np.dtype) or isinstance(dtype, type) or isinstance(dtype, str):
        return np.dtype(dtype)
    return np.dtype(str(dtype).replace("torch.", ""))            # torch.float32 -> float32


def guard_bytes(shape, itemsize):
    """bytes of guard on each side: max(4096, two rows), rounded up to a multiple of 16"""
    row = int(np.prod(shape[1:], dtype=np.int64)) * itemsize if len(shape) else itemsize
    g = max(GUARD_MIN, 2 * row)
    return -(-g // 16) * 16


class Guarded:
    """One guarded output buffer.  `t`: the payload (torch tensor or NumPy array); `ptr`: its address."""

    def __init__(self, shape, dtype, poison, device, k=0):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        dt = _np_dtype(dtype)
        k, poison = int(k), int(poison)
        assert k >= 0 and 0 <= poison <= 255 and dt.itemsize in (1, 4, 8) and all(s >= 0 for s in shape)
        self.shape, self.dtype, self.k, self.poison, self.itemsize = shape, dt, k, poison, dt.itemsize
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        self.guard = guard_bytes(shape, dt.itemsize)
        total = 16 + self.guard + k * dt.itemsize + self.nbytes + self.guard
        self.is_numpy = device is None or device == "numpy"
        if self.is_numpy:
            self.buf = np.full(total, poison, np.uint8)
            base = self.buf.ctypes.data
        else:
            import torch
            self.buf = torch.full((total,), poison, dtype=torch.uint8, device=device)
            if self.buf.is_cuda:
                torch.cuda.synchronize(self.buf.device)          # the fill is complete before a library stream may write the payload
            base = self.buf.data_ptr()
        self.head = (-base) % 16                                   # bytes skipped so that the front guard starts on a boundary
        self.lo = self.head + self.guard + k * dt.itemsize          # first payload byte within buf
        self.front = self.guard + k * dt.itemsize                   # checked bytes in front of the payload
        if self.is_numpy:
            self.t = self.buf[self.lo:self.lo + self.nbytes].view(dt).reshape(shape)
            self.ptr = self.t.ctypes.data if self.nbytes else base + self.lo
            assert self.t.flags["C_CONTIGUOUS"]
        else:
            import torch
            self.t = self.buf[self.lo:self.lo + self.nbytes].view(getattr(torch, dt.name)).view(shape)
            self.ptr = self.t.data_ptr() if self.nbytes else base + self.lo
            assert self.t.is_contiguous()
        assert self.ptr == base + self.lo
        assert self.ptr % 16 == (k * dt.itemsize) % 16, f"payload at residue {self.ptr % 16}, wanted {(k * dt.itemsize) % 16}"

    # ---- the bytes as they are now, on the host
    def _bytes(self):
        b = self.buf if self.is_numpy else self.buf.cpu().numpy()
        return b[self.head:]

    def stray(self):
        """sorted offsets (int64) of changed guard / slack bytes from the payload's edges: negative in front, >= 0 behind"""
        b = self._bytes()
        front = b[:self.front]
        back = b[self.front + self.nbytes:self.front + self.nbytes + self.guard]
        assert len(back) == self.guard
        lo = np.flatnonzero(front != self.poison).astype(np.int64) - self.front
        hi = np.flatnonzero(back != self.poison).astype(np.int64)
        return np.concatenate([lo, hi])

    def unwritten(self, exempt=None):
        """flat indices of payload elements that are still poison in every byte; `exempt`: boolean array of the payload's shape (or
        flat), True where the header promises nothing"""
        b = self._bytes()[self.front:self.front + self.nbytes]
        if self.nbytes == 0:
            return np.zeros(0, np.int64)
        still = (b.reshape(-1, self.itemsize) == self.poison).all(1)
        if exempt is not None:
            still &= ~np.asarray(exempt, bool).reshape(-1)
        return np.flatnonzero(still).astype(np.int64)

    def untouched(self):
        """True when the whole payload is still poison (an output the call must not write)"""
        b = self._bytes()[self.front:self.front + self.nbytes]
        return bool((b == self.poison).all())

    def host(self):
        """the payload as a NumPy array (a copy)"""
        return np.array(self.t, copy=True) if self.is_numpy else self.t.cpu().numpy()

    def findings(self, exempt=None, name="output"):
        out = []
        s = self.stray()
        if len(s):
            out.append(f"{name}: stray: {len(s)} guard bytes changed, offsets from the payload's edges {s[:8].tolist()}"
                       f"{' ...' if len(s) > 8 else ''} (payload {self.shape} {self.dtype.name}, {self.nbytes} bytes, k = {self.k})")
        u = self.unwritten(exempt)
        if len(u):
            idx = [tuple(int(v) for v in np.unravel_index(i, self.shape)) for i in u[:8]]
            out.append(f"{name}: unwritten: {len(u)} of {self.nbytes // self.itemsize} elements still hold the poison 0x{self.poison:02X}, "
                       f"at {idx}{' ...' if len(u) > 8 else ''}")
        return out


def guarded(shape, dtype, poison, device, k=0):
    """a Guarded buffer on `device`: "cuda" / "cpu" (torch tensor) or "numpy" / None (NumPy array, the twin for host entry points)"""
    return Guarded(shape, dtype, poison, device, k)


def guarded_array(shape, dtype, poison, k=0):
    """the NumPy twin"""
    return Guarded(shape, dtype, poison, "numpy", k)


def poison_value(dtype, poison):
    """the value an element of `dtype` has when all its bytes are `poison`"""
    dt = _np_dtype(dtype)
    return np.frombuffer(bytes([int(poison)]) * dt.itemsize, dt)[0]


def holds_poison(a):
    """True when an element of the array `a` equals the all-poison value of its dtype for either poison: an expected output for which
    `unwritten` would fire on a legitimate value"""
    a = np.asarray(a)
    if a.dtype == np.bool_:
        return False
    if a.size == 0:
        return False
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1, a.dtype.itemsize)
    return any(bool((b == p).all(1).any()) for p in POISONS)


def snapshot(t):
    """the bytes of a torch tensor / NumPy array (any device), for `unchanged`"""
    a = t.detach().cpu().numpy() if hasattr(t, "data_ptr") else np.asarray(t)
    return (a.shape, a.dtype.str, np.ascontiguousarray(a).tobytes())


def unchanged(t, snap):
    """True when `t` holds the bytes `snapshot(t)` saw"""
    return snapshot(t) == snap
