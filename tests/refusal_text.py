"""The whole text of a refusal: what an entry point says when it turns a call down is part of its behaviour, word for word."""
from obia_amd import _lib


def refused_saying(text, fn, *argsets):
    """every call fn(*args) -- fn(**args) for a dict -- is refused with OBIA_E_INVALID and leaves exactly `text` as the last error"""
    for args in argsets:
        rc = fn(**args) if isinstance(args, dict) else fn(*args)
        assert rc == _lib.E_INVALID and _lib.last_error() == text, (fn.__name__, rc, _lib.last_error(), text)
