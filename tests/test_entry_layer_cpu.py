"""The prologue of the C ABI (obia_amd/csrc/common.hpp: enter()) without a GPU: every entry point that takes a handle refuses a null
one before it touches an argument or the device.

The list is derived from the registry of obia_amd/_lib.py (BINDINGS, every header) and the prototypes of the headers, so a new entry
point is covered without an edit here: every name whose first parameter is a handle -- an obia_ctx, or for the obia_tiler_* functions but
obia_tiler_create an obia_tiler -- is called with a null handle and zero / null for everything else.  It returns OBIA_E_INVALID with
"null context" ("null tiler" for a session; MESSAGE for the one that words it otherwise), but for the few that do not return a status,
which give the value their header names."""
import ctypes

import pytest

from obia_amd import _lib
from tests.test_binding_tables_cpu import prototypes

# entry points that do not return a status: what they give for a null handle (include/obia_hip.h)
NO_STATUS = {"obia_tiler_create": None, "obia_workspace_bytes": 0, "obia_last_timing": -1.0, "obia_tiler_next_id": -1,
             "obia_destroy": None, "obia_tiler_destroy": None}
# the one entry point that checks its two pointers in one statement (context.cpp; its header: "OBIA_E_INVALID for a null context or output")
MESSAGE = {"obia_test_visited_nonzero": "null context or null output"}


def handle_takers():
    return {name: table[name] for header, table in _lib.BINDINGS.items() for name, (_, params) in prototypes(header).items()
            if params and params[0].startswith(("obia_ctx *", "obia_tiler *"))}


def null_of(argtype):
    if argtype is _lib.PickFn:
        return ctypes.cast(None, _lib.PickFn)
    if argtype in (ctypes.c_int, ctypes.c_int32, ctypes.c_int64):
        return 0
    if argtype in (ctypes.c_double, ctypes.c_float):
        return 0.0
    return None                                                   # c_void_p and POINTER(...)


def takes_tiler(name):
    return name.startswith("obia_tiler_") and name != "obia_tiler_create"


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_the_tables_list_the_handle_takers():
    names = handle_takers()
    assert len(names) == 119 and set(NO_STATUS) <= set(names)             # of the 129 bound; the other ten take no handle
    assert all(argtypes[0] is ctypes.c_void_p for _, argtypes in names.values())
    assert {"obia_create", "obia_create_on_stream", "obia_rasterize_info", "obia_slic_default_params", "obia_abi_version",
            "obia_last_error", "obia_test_sweep_plan", "obia_test_launch_grid", "obia_test_launch_grid_names",
            "obia_test_seam_sort_limit"}.isdisjoint(names) and len(_lib.bound_entry_points()) == 129
    assert sum(takes_tiler(n) for n in names) == 9


@pytest.mark.parametrize("name", sorted(handle_takers()))
def test_a_null_handle_is_refused_before_anything_else(lib, name):
    res, argtypes = handle_takers()[name]
    args = [null_of(t) for t in argtypes]
    want = "null tiler" if takes_tiler(name) else MESSAGE.get(name, "null context")
    other = lib.obia_synchronize if takes_tiler(name) else lib.obia_tiler_run      # leaves the OTHER message: this call must replace it
    assert other(*([None] + [0] * (len(other.argtypes) - 1))) == _lib.E_INVALID and _lib.last_error() != want
    got = getattr(lib, name)(*args)
    if name in NO_STATUS:
        assert got == NO_STATUS[name]
        if name == "obia_tiler_create":
            assert _lib.last_error() == want
        return
    assert got == _lib.E_INVALID
    assert _lib.last_error() == want
