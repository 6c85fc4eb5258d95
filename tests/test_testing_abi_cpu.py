"""include/obia_testing.h without a GPU: the fourth binding table of obia_amd/_lib.py names exactly what the header declares, the
library exports it, none of it leaks into the operator ABI (include/obia_hip.h), and a null context is refused before anything else;
`timing()` knows the three command counters (obia_last_timing 16-18)."""
import os
import re

from obia_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(obia_[a-z0-9_]+)\s*\(", txt))


def test_the_table_is_the_header():
    syms = declared("obia_testing.h")
    assert syms == set(_lib._TEST_SIGNATURES) == {"obia_test_clear_ranges_dev", "obia_test_sweep_plan", "obia_test_launch_grid",
                                                       "obia_test_launch_grid_names", "obia_test_seam_sort_limit",
                                                       "obia_test_enforce_connectivity_batch_dev", "obia_test_cc_report",
                                                       "obia_test_poison_workspace_dev", "obia_test_visited_nonzero"}
    assert not syms & set(_lib._SIGNATURES) and not syms & declared("obia_hip.h")
    lib = _lib.load()
    for name, (res, args) in _lib._TEST_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args


def test_a_null_context_is_refused_first():
    lib = _lib.load()
    assert lib.obia_synchronize(None) == _lib.E_INVALID
    assert lib.obia_test_clear_ranges_dev(None, None, None, None, 0) == _lib.E_INVALID
    assert _lib.last_error() == "null context"


def test_timing_names_the_command_counters():
    """a null handle gives -1.0 for every class: 16, 17 and 18 are classes like the others"""
    lib = _lib.load()
    assert [lib.obia_last_timing(None, i) for i in (16, 17, 18)] == [-1.0] * 3
    header = open(os.path.join(ROOT, "include", "obia_hip.h")).read()
    assert "16 / 17 / 18 = small commands" in header
