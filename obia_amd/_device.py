"""The one place where the wrappers turn arrays and tensors into device pointers and hand results back.

A wrapper calls, in this order: ``need_torch``; ``device_of`` (which refuses a CPU tensor) and its own argument checks, none of
which touches the library; ``as_dev`` for every array a kernel reads; ``begin`` -- the library, the context and the wait for
torch's stream -- directly before the first ABI call; ``out`` on what it returns.  ``end`` waits for the context's stream: only
cost.py and seeds.py call it, and only they ask ``as_dev`` for 16-byte alignment."""
import numpy as np

from . import _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def need_torch(who, what="for device memory"):
    if torch is None:
        raise ImportError(f"{who} needs torch {what}")


def is_torch(x):
    return torch is not None and isinstance(x, torch.Tensor)


def device_of(ctx, *xs, hint=""):
    """Index of the device the call runs on: that of the first tensor among ``xs``, else the context's, else 0.  A CPU tensor in
    any position is refused: its pointer must never reach a kernel.  Loads nothing and creates no context."""
    dev = None
    for x in xs:
        if is_torch(x):
            if not x.is_cuda:
                raise ValueError("torch inputs must live on the GPU" + hint)
            if dev is None:
                dev = x.device.index or 0
    if dev is None:
        dev = ctx.device if ctx is not None else 0
    return dev


def as_dev(x, dtype, dev, align16=False):
    """Contiguous tensor of ``dtype`` on ``cuda:dev`` from a tensor or from anything NumPy accepts (cast on the host, as
    ``astype`` casts).  ``align16``: a tensor that does not start on a 16-byte boundary is copied to one that does."""
    if is_torch(x):
        t = x.to(device=f"cuda:{dev}", dtype=dtype).contiguous()
    else:
        npdt = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64}[dtype]
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(x).astype(npdt, copy=False)), device=f"cuda:{dev}")
    if align16 and t.data_ptr() % 16:
        t = t.clone()
    return t


def begin(dev, ctx, host=False):
    """``(lib, context)`` directly before the first ABI call.  ``host=True``: the call hands host arrays to a host entry point, so
    torch has written nothing to wait for (and need not be installed)."""
    lib = _lib.load()
    c = ctx or _lib.default_context(dev)
    if not host:
        torch.cuda.current_stream(dev).synchronize() # inputs written by torch are complete before the context's stream reads them
    return lib, c


def end(lib, c):
    _lib.check(lib.obia_synchronize(c.handle))       # outputs are complete before torch (or the host) sees them


def out(t, is_t):
    """A tensor, or a tuple or dict of tensors, as it is for tensor input and as NumPy otherwise; other values pass through."""
    if is_t:
        return t
    if isinstance(t, tuple):
        return tuple(out(v, False) for v in t)
    if isinstance(t, dict):
        return {k: out(v, False) for k, v in t.items()}
    return t.cpu().numpy() if is_torch(t) else t
