"""tests/workspace_history.py without a GPU: every entry point obia_amd/_lib.py binds has a row, every row is a decision, every case a
row names exists, and every source file that takes memory from the arena is run by a case."""
import os
import re

import pytest

from tests import workspace_history as WH

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "obia_amd", "csrc")


def test_every_bound_entry_point_has_a_row():
    """A new entry point fails here until somebody reads what initialises its workspace and decides: a case, or the reason for none."""
    bound = WH.bound_entry_points()
    assert len(bound) == len(set(bound)) == 129
    assert set(bound) == set(WH.ROWS), sorted(set(bound) ^ set(WH.ROWS))


def test_every_row_is_a_decision():
    for name, row in WH.ROWS.items():
        if row.exempt is not None:
            assert not row.cases and row.init is None and len(row.exempt) > 20, name
        else:
            assert row.cases and row.init and len(row.init) > 20, name


def test_every_case_a_row_names_exists():
    pytest.importorskip("torch")
    from tests import test_gpu_output_guards as G
    from tests import test_gpu_pointer_alignment as PA
    from tests import test_gpu_workspace_history as T
    assert set(WH.cases()) == set(T.OPS), sorted(set(WH.cases()) ^ set(T.OPS))
    for c in WH.cases():
        if c.startswith("pa:"):
            assert c[3:] in PA.OPS, c
        elif c.startswith("guards:"):
            assert c[7:] in G.REGISTRY, c
    # a "guards:" case stands in a row of an entry point its registry case really calls
    for name, row in WH.ROWS.items():
        for c in row.cases:
            if c.startswith("guards:"):
                assert name in G.REGISTRY[c[7:]].entries, (name, c)
    assert set(PA.OPS) <= {c[3:] for c in WH.cases() if c.startswith("pa:")}, "an operator of the alignment file has no row"


def test_every_source_file_that_takes_workspace_is_run_by_a_case():
    takes = re.compile(r"arena\.(get|alloc)\b|\bA\.get<")
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".hpp"))
                   and takes.search(open(os.path.join(CSRC, f), encoding="utf-8").read()))
    assert files == sorted(WH.ARENA_FILES), sorted(set(files) ^ set(WH.ARENA_FILES))
    assert set(WH.ARENA_FILES.values()) <= set(WH.cases())


def test_the_test_entries_are_declared():
    header = open(os.path.join(os.path.dirname(CSRC), "..", "include", "obia_testing.h"), encoding="utf-8").read()
    for name in ("obia_test_poison_workspace_dev", "obia_test_visited_nonzero"):
        assert name in header and name in WH.ROWS
