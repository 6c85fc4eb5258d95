"""`timing()` knows the three command counters (obia_last_timing 16-18).  (include/obia_testing.h against its binding table, and a
null context: tests/test_binding_tables_cpu.py and tests/test_entry_layer_cpu.py.)"""
import os

from obia_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_timing_names_the_command_counters():
    """a null handle gives -1.0 for every class: 16, 17 and 18 are classes like the others"""
    lib = _lib.load()
    assert [lib.obia_last_timing(None, i) for i in (16, 17, 18)] == [-1.0] * 3
    header = open(os.path.join(ROOT, "include", "obia_hip.h")).read()
    assert "16 / 17 / 18 = small commands" in header
