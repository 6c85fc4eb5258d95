"""The schedule of a batch's sweeps without a GPU: plan_sweeps (obia_amd/csrc/slic_sweep_plan.hpp) decides every launch of a batch
as data, and obia_test_sweep_plan (include/obia_testing.h) writes that plan out, one command per line in queue order.  The expected
lines below are written by hand from the rules of the sweep driver; nothing here is produced by the code under test.

A line starts with its stream (s0: the context's, s1: the side stream).  `step`: the centroid step in front of a sweep, with the
problems it steps and the bins it resets; `sweep`: the sweep kernel with its tiles and flags."""
import ctypes

import numpy as np
import pytest

from obia_amd import _lib

FULL = (128, 128, 16, 32, 32, 128 * 128, 16)     # 4 sweep tiles, 16 bins, mask hides nothing, grid seeds
WIDE = (128, 192, 24, 32, 32, 24000, 24)         # 6 sweep tiles, 24 bins, a mask that hides pixels


def plan(problems, C=8, masked=True, max_iter=3, prepass_iter=0, prepass_only=False, exit_on_fixed_point=False, slic_zero=False,
         direct=False, col_lb=False, fuse_features=False, mask_packed=True, repeat=False, debug_sync=False, prep_grouped=False,
         prepass_visits=False, prepass_share=1, prepass_groups=1, sweep_groups=1, residencies=(1 << 30, 1 << 30), expect=_lib.OBIA_OK):
    rows = np.ascontiguousarray(np.asarray(problems, dtype=np.int64).reshape(-1, 7))
    settings = (ctypes.c_int32 * 11)(C, masked, max_iter, prepass_iter, prepass_only, exit_on_fixed_point, slic_zero, direct, col_lb,
                                     fuse_features, mask_packed)
    switches = (ctypes.c_int32 * 6)(debug_sync, prep_grouped, prepass_visits, prepass_share, prepass_groups, sweep_groups)
    res = (ctypes.c_int64 * 2)(*residencies)
    text = ctypes.create_string_buffer(1 << 16)
    rc = _lib.load().obia_test_sweep_plan(rows.ctypes.data, len(rows), settings, int(repeat), switches, res, text, len(text))
    assert rc == expect, _lib.last_error()
    return text.value.decode().splitlines() if rc == _lib.OBIA_OK else _lib.last_error()


def sweeps(lines):
    return [ln for ln in lines if " sweep " in ln]


def steps(lines):
    return [ln for ln in lines if " step " in ln]


def field(line, name):
    words = line.split()
    return words[words.index(name) + 1]


def kernel(line):
    return line.split(" nch ")[0].split(" ", 4)[4]


def splits(lines):
    return int(field(lines[0], "grp_split")), int(field(lines[0], "col_split")), int(field(lines[0], "n_shared"))


SPATIAL_FLAGS = "accumulate 1 accum_color 0 store 0 cache 1 slot 256 timing prepass"
MAIN8 = "slic_assign_kernel<8, true, false, false, false>"
LAST_PRE8 = "slic_assign_kernel<8, true, true, false, false>"


def test_case_g_both_groupings_forced():
    got = plan([FULL, WIDE], prepass_groups=2, sweep_groups=2)
    assert got == [
        "batch grp_split 1 col_split 1 n_shared 0",
        "s0 upload",
        "s0 clear",
        "fork s0 -> s1",
        "s0 step 1 spatial slic_prep_lane_kernel<8> parity 0 first 1 zmode 0 grid (1, 1) problems [0, 1) cells [0, 16)",
        "s0 sweep 1 spatial slic_spatial_kernel<8> nch 8 tiles [0, 4) " + SPATIAL_FLAGS,
        "s1 step 1 spatial slic_prep_lane_kernel<8> parity 0 first 1 zmode 0 grid (1, 1) problems [1, 2) cells [16, 40)",
        "s1 sweep 1 spatial slic_spatial_kernel<8> nch 8 tiles [4, 10) " + SPATIAL_FLAGS,
        "s0 step 2 spatial slic_prep_lane_kernel<8> parity 1 first 0 zmode 0 grid (1, 1) problems [0, 1) cells [0, 16)",
        "s0 sweep 2 spatial slic_spatial_kernel<8> nch 8 tiles [0, 4) " + SPATIAL_FLAGS,
        "s1 step 2 spatial slic_prep_lane_kernel<8> parity 1 first 0 zmode 0 grid (1, 1) problems [1, 2) cells [16, 40)",
        "s1 sweep 2 spatial slic_spatial_kernel<8> nch 8 tiles [4, 10) " + SPATIAL_FLAGS,
        "join s1 -> s0",
        "s0 step 3 spatial slic_prep_lane_kernel<8> parity 0 first 0 zmode 0 grid (1, 2) problems [0, 2) cells [0, 40)",
        "s0 sweep 3 spatial " + LAST_PRE8 + " nch 8 tiles [0, 10) accumulate 1 accum_color 1 store 0 cache 0 slot 256 timing prepass",
        "fork s0 -> s1",
        "s0 step 4 colour slic_prep_lane_kernel<8> parity 1 first 0 zmode 0 grid (1, 1) problems [0, 1) cells [0, 16)",
        "s0 sweep 4 colour " + MAIN8 + " nch 8 tiles [0, 4) accumulate 1 accum_color 1 store 0 cache 1 slot 0 timing assign_grp",
        "s1 step 4 colour slic_prep_lane_kernel<8> parity 1 first 0 zmode 0 grid (1, 1) problems [1, 2) cells [16, 40)",
        "s1 sweep 4 colour " + MAIN8 + " nch 8 tiles [4, 10) accumulate 1 accum_color 1 store 0 cache 1 slot 0 timing assign_grp",
        "s0 step 5 colour slic_prep_lane_kernel<8> parity 0 first 0 zmode 0 grid (1, 1) problems [0, 1) cells [0, 16)",
        "s0 sweep 5 colour " + MAIN8 + " nch 8 tiles [0, 4) accumulate 1 accum_color 1 store 0 cache 1 slot 0 timing assign_grp",
        "s1 step 5 colour slic_prep_lane_kernel<8> parity 0 first 0 zmode 0 grid (1, 1) problems [1, 2) cells [16, 40)",
        "s1 sweep 5 colour " + MAIN8 + " nch 8 tiles [4, 10) accumulate 1 accum_color 1 store 0 cache 1 slot 0 timing assign_grp",
        "s0 step 6 colour slic_prep_lane_kernel<8> parity 1 first 0 zmode 0 grid (1, 1) problems [0, 1) cells [0, 16)",
        "s0 sweep 6 colour " + MAIN8 + " nch 8 tiles [0, 4) accumulate 0 accum_color 1 store 1 cache 1 slot 0 timing assign_grp",
        "s1 step 6 colour slic_prep_lane_kernel<8> parity 1 first 0 zmode 0 grid (1, 1) problems [1, 2) cells [16, 40)",
        "s1 sweep 6 colour " + MAIN8 + " nch 8 tiles [4, 10) accumulate 0 accum_color 1 store 1 cache 1 slot 0 timing assign_grp",
        "join s1 -> s0",
    ]
    # group launches: 4 in the pre-pass, 6 in the colour pass
    grouped = [ln for ln in sweeps(got) if ln.startswith("s1")]
    assert 2 * sum(" spatial " in ln for ln in grouped) == 4 and 2 * sum(" colour " in ln for ln in grouped) == 6


@pytest.mark.parametrize("residencies,expected", [((4, 4), (1, 1)), ((5, 4), (0, 1)), ((5, 5), (0, 0))])
def test_case_g_threshold(residencies, expected):
    """mode 1: a pass is grouped when the smaller group's 4 tiles are at least one residency of its kernel"""
    got = plan([FULL, WIDE], prepass_groups=1, sweep_groups=1, residencies=residencies)
    assert splits(got)[:2] == expected
    assert got.count("fork s0 -> s1") == got.count("join s1 -> s0") == sum(expected)


def test_a_tie_takes_the_later_split():
    assert splits(plan([FULL, FULL, FULL], prepass_share=0, prepass_groups=2, sweep_groups=2))[:2] == (2, 2)


SHARED_FOUR = [FULL, FULL, WIDE, FULL]


def test_case_s_shared_prepass_through_tables():
    got = plan(SHARED_FOUR, prepass_groups=2, sweep_groups=0)
    assert got == [
        "batch grp_split 0 col_split 0 n_shared 2",
        "classes table ap {0 2} at {0 1 2 3 8 9 10 11 12 13} mr {1 0 3 0} kmax_act 24 kmax_mem 16 shared_px 65536",
        "s0 upload",
        "s0 clear",
        "s0 step 1 spatial slic_prep_lane_kernel<8> parity 0 first 1 zmode 0 grid (1, 2) problems table cells [0, 72)",
        "s0 sweep 1 spatial slic_spatial_kernel<8> nch 8 tiles table 10 " + SPATIAL_FLAGS,
        "s0 step 2 spatial slic_prep_lane_kernel<8> parity 1 first 0 zmode 0 grid (1, 2) problems table cells [0, 72)",
        "s0 sweep 2 spatial slic_spatial_kernel<8> nch 8 tiles table 10 " + SPATIAL_FLAGS,
        "s0 broadcast grid (1, 2)",
        "s0 step 3 spatial slic_prep_lane_kernel<8> parity 0 first 0 zmode 0 grid (1, 4) problems [0, 4) cells [0, 72)",
        "s0 sweep 3 spatial " + LAST_PRE8 + " nch 8 tiles [0, 18) accumulate 1 accum_color 1 store 0 cache 0 slot 256 timing prepass",
        "s0 step 4 colour slic_prep_lane_kernel<8> parity 1 first 0 zmode 0 grid (1, 4) problems [0, 4) cells [0, 72)",
        "s0 sweep 4 colour " + MAIN8 + " nch 8 tiles [0, 18) accumulate 1 accum_color 1 store 0 cache 1 slot 0 timing assign",
        "s0 step 5 colour slic_prep_lane_kernel<8> parity 0 first 0 zmode 0 grid (1, 4) problems [0, 4) cells [0, 72)",
        "s0 sweep 5 colour " + MAIN8 + " nch 8 tiles [0, 18) accumulate 1 accum_color 1 store 0 cache 1 slot 0 timing assign",
        "s0 step 6 colour slic_prep_lane_kernel<8> parity 1 first 0 zmode 0 grid (1, 4) problems [0, 4) cells [0, 72)",
        "s0 sweep 6 colour " + MAIN8 + " nch 8 tiles [0, 18) accumulate 0 accum_color 1 store 1 cache 1 slot 0 timing assign",
    ]


def test_case_s_colour_pass_grouped_at_split_2():
    got = plan(SHARED_FOUR, prepass_groups=2, sweep_groups=2)
    assert splits(got) == (0, 2, 2)     # 8 against 10 tiles; the shared pre-pass runs no groups
    assert got.index("s0 broadcast grid (1, 2)") < got.index("fork s0 -> s1") and got.count("fork s0 -> s1") == 1
    assert " tiles [0, 8) " in sweeps(got)[3] and " tiles [8, 18) " in sweeps(got)[4]
    assert steps(got)[3].endswith("grid (1, 2) problems [0, 2) cells [0, 32)") and steps(got)[4].endswith("grid (1, 2) problems [2, 4) cells [32, 72)")
    assert got[-1] == "join s1 -> s0"


def test_case_s_prime_span_form():
    got = plan([FULL, FULL], prepass_groups=2, sweep_groups=0)
    assert got[:8] == [
        "batch grp_split 0 col_split 0 n_shared 1",
        "classes span ap {0} at {0 1 2 3} mr {1 0} kmax_act 16 kmax_mem 16 shared_px 32768",
        "s0 upload",
        "s0 clear",
        "s0 step 1 spatial slic_prep_lane_kernel<8> parity 0 first 1 zmode 0 grid (1, 1) problems [0, 1) cells [0, 32)",
        "s0 sweep 1 spatial slic_spatial_kernel<8> nch 8 tiles [0, 4) " + SPATIAL_FLAGS,
        "s0 step 2 spatial slic_prep_lane_kernel<8> parity 1 first 0 zmode 0 grid (1, 1) problems [0, 1) cells [0, 32)",
        "s0 sweep 2 spatial slic_spatial_kernel<8> nch 8 tiles [0, 4) " + SPATIAL_FLAGS,
    ]
    assert got[8] == "s0 broadcast grid (1, 1)" and "tiles [0, 8)" in got[10] and len(got) == 17


# ---- the rule cases ----------------------------------------------------------------------------------------------------------------

def flags(line):
    return tuple(int(field(line, n)) for n in ("accumulate", "accum_color", "store", "cache"))


def test_unmasked():
    got = plan([FULL], masked=False)
    assert "s0 fill labels" not in got and len(sweeps(got)) == 3
    assert [kernel(ln) for ln in sweeps(got)] == ["slic_assign_kernel<8, false, false, false, false>"] * 3
    assert [flags(ln)[:3] for ln in sweeps(got)] == [(1, 1, 0), (1, 1, 0), (0, 1, 1)]
    assert [field(ln, "parity") for ln in steps(got)] == ["0", "1", "0"]
    assert [field(ln, "slot") + field(ln, "timing") for ln in sweeps(got)] == ["0assign"] * 3


@pytest.mark.parametrize("masked", [False, True])
def test_one_sweep(masked):
    """one sweep in all: the fill value is what the reference keeps; nothing to group, whatever the switches say"""
    got = plan([FULL, WIDE], masked=masked, max_iter=1, prepass_only=masked, prepass_groups=2, sweep_groups=2)
    assert got[1:4] == ["s0 fill labels", "s0 upload", "s0 clear"] and len(sweeps(got)) == 1
    assert flags(sweeps(got)[0])[0::2] == (0, 1) and splits(got) == (0, 0, 0) and "fork s0 -> s1" not in got


def test_repeat():
    got = plan(SHARED_FOUR, repeat=True, prepass_groups=2, sweep_groups=2)
    assert got[1] == "s0 fill labels" and got.count("s0 fill labels") == 2
    assert got[got.index("s0 fill labels", 2) + 1].startswith("s0 step 4 colour")
    assert all(field(ln, "store") == "2" for ln in sweeps(got)) and splits(got) == (0, 0, 0)
    assert [kernel(ln) for ln in sweeps(got)] == ["slic_prepass_kernel<8, true, false>"] * 2 + [LAST_PRE8] + [MAIN8] * 3


def test_fixed_point():
    got = plan([FULL, WIDE], exit_on_fixed_point=True, prepass_groups=2, sweep_groups=2)
    assert got[1:3] == ["s0 fill bin_stamp tile_lp", "s0 fill labels"] and got.count("s0 fill labels tile_lp") == 1
    assert got[got.index("s0 fill labels tile_lp") + 1].startswith("s0 step 4 colour")
    assert [kernel(ln) for ln in sweeps(got)] == ["slic_prepass_kernel<8, true, true>"] * 2 + ["slic_assign_kernel<8, true, true, true, false>"] + \
        ["slic_assign_kernel<8, true, false, true, false>"] * 3
    assert splits(got) == (0, 0, 0)


def test_slic_zero():
    got = plan([FULL, WIDE], masked=False, slic_zero=True, sweep_groups=2)
    assert all(field(ln, "store") == "2" for ln in sweeps(got)) and [field(ln, "zmode") for ln in steps(got)] == ["2", "1", "1"]
    assert [kernel(ln) for ln in sweeps(got)] == ["slic_assign_kernel<8, false, false, false, true>"] * 3
    body = got[got.index("s0 clear") + 1:]
    assert [ln.split()[1] for ln in body] == ["step", "sweep", "step", "maxdist", "sweep", "step", "maxdist", "sweep"]
    assert body[3] == "s0 maxdist grid (128, 2)"


def test_colour_bound_and_padding():
    assert kernel(sweeps(plan([FULL], C=5, col_lb=True))[-1]) == "slic_assign_collb_kernel<8, true, 5>"
    assert kernel(sweeps(plan([FULL], C=5, col_lb=True, masked=False))[0]) == "slic_assign_collb_kernel<8, false, 5>"
    for C, name in [(5, "slic_assign_kernel<8, true, false, false, false, 5>"), (6, "slic_assign_kernel<8, true, false, false, false, 6>"),
                    (7, "slic_assign_kernel<8, true, false, false, false, 7>"), (9, "slic_assign_kernel<12, true, false, false, false, 9>")]:
        got = sweeps(plan([FULL], C=C))
        assert [kernel(ln) for ln in got[3:]] == [name] * 3 and {field(ln, "nch") for ln in got[3:]} == {str(C)}
        assert {field(ln, "nch") for ln in got[:3]} == {str(4 * ((C + 3) // 4))}     # the pre-pass has no padding variants


def test_prepass_only():
    got = plan([FULL, WIDE], prepass_only=True, prepass_share=0, prepass_groups=2, sweep_groups=2)
    assert [field(ln, "sweep") for ln in sweeps(got)] == ["1", "1", "2", "2", "3"] and all(" spatial " in ln for ln in sweeps(got))
    assert flags(sweeps(got)[-1]) == (0, 1, 1, 0) and kernel(sweeps(got)[-1]) == LAST_PRE8
    assert splits(got) == (1, 0, 0)


def test_sweep_counts():
    got = plan([FULL, FULL], prepass_iter=2, prepass_groups=2, sweep_groups=0)
    assert splits(got) == (1, 0, 0) and len(sweeps(got)) == 2 + 1 + 3     # a pre-pass count from the stage entry: no sharing, so sweep 1 as two groups; sweep 2; three colour sweeps
    assert splits(plan([FULL, WIDE], prepass_iter=1, prepass_groups=2, sweep_groups=0)) == (0, 0, 0)
    got = plan([FULL, WIDE], max_iter=2, prepass_groups=0, sweep_groups=2)
    assert splits(got) == (0, 1, 0)
    assert [flags(ln)[0::2] for ln in sweeps(got) if " colour " in ln] == [(1, 0), (1, 0), (0, 1), (0, 1)]


def test_fused_features():
    got = plan([FULL, WIDE], fuse_features=True)
    assert [kernel(ln) for ln in sweeps(got)][:4] == ["slic_spatial_kernel<8>"] * 2 + ["slic_assign_rawin_kernel<8>", MAIN8]
    assert "slic_assign_rawin_kernel<8>" not in "\n".join(plan([FULL, WIDE], fuse_features=True, repeat=True))
    for bad in (dict(masked=False), dict(C=7), dict(C=16)):
        assert plan([FULL, WIDE], fuse_features=True, expect=_lib.E_INVALID, **bad) == "fused feature pass on a batch that cannot take it"


def test_switches_one_at_a_time():
    two = dict(prepass_groups=2, sweep_groups=2)
    got = plan(SHARED_FOUR, prep_grouped=True, **two)
    assert splits(got) == (0, 0, 0) and all(" slic_prep_kernel<16> " in ln for ln in steps(got))
    assert all(" slic_prep_kernel<32> " in ln for ln in steps(plan(SHARED_FOUR, C=16, prep_grouped=True)))
    got = plan(SHARED_FOUR, prepass_visits=True, **two)
    assert splits(got) == (0, 0, 2) and [kernel(ln) for ln in sweeps(got)][:2] == ["slic_prepass_kernel<8, true, false>"] * 2
    assert splits(plan(SHARED_FOUR, prepass_share=0, **two)) == (2, 2, 0)
    assert splits(plan(SHARED_FOUR, debug_sync=True, **two)) == (0, 0, 2)


def test_edges():
    assert plan([], max_iter=3) == ["s0 fill labels", "no sweep"]
    assert plan([FULL], max_iter=0) == ["s0 fill labels", "no sweep"]
    got = plan([(128, 128, 0, 1, 1, 128 * 128, 0), WIDE], prepass_groups=2, sweep_groups=0)
    assert splits(got) == (1, 0, 0) and " grid (1, 1) problems [0, 1) " in steps(got)[0]
    wide = (1, 4194304, 1, 1, 4194304, 4194304, 1)
    assert plan([wide], expect=_lib.E_UNSUPPORTED) == "rasters / tile windows wider than 4194303 pixels are not supported (got 4194304)"
