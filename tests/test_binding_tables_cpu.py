"""The registry of obia_amd/_lib.py (BINDINGS: one table of entry points per header of include/) against the headers, without a GPU:
the headers are the registry's keys; every header declares exactly its table's names; the tables share no name; the library exports
every name and load() binds it as the table says; every prototype agrees with its table entry, return type and parameter by parameter;
and every constant _lib.py mirrors from a header has the header's value.  No entry point is exempt: one that does not parse extends
SCALARS or RETURNS.  (A null handle at every entry point: tests/test_entry_layer_cpu.py.)"""
import ctypes
import os
import re

import pytest

from obia_amd import _lib

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADERS = list(_lib.BINDINGS)

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float}
RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "const char *": ctypes.c_char_p, "void": None}

# header -> {macro: the attribute of obia_amd._lib that mirrors it}
MIRRORS = {
    "obia_hip.h": {"OBIA_OK": "OBIA_OK", "OBIA_E_INVALID": "E_INVALID", "OBIA_E_HIP": "E_HIP", "OBIA_E_NOMEM": "E_NOMEM",
                   "OBIA_E_UNSUPPORTED": "E_UNSUPPORTED", "OBIA_E_EMPTY": "E_EMPTY", "OBIA_E_NONFINITE": "E_NONFINITE",
                   "OBIA_MASK_SEEDS_CHUNK": "MASK_SEEDS_CHUNK", "OBIA_SEEDING_GRID": "SEEDING_GRID", "OBIA_SEEDING_SKIMAGE": "SEEDING_SKIMAGE"},
    "obia_sharpness.h": {"OBIA_SHARP_MAX_WIN": "SHARP_MAX_WIN"},
    "obia_training.h": {"OBIA_TRAIN_MAX_KSIZE": "TRAIN_MAX_KSIZE", "OBIA_TRAIN_MAX_SIDE": "TRAIN_MAX_SIDE", "OBIA_TRAIN_MINMAX_WORK": "TRAIN_MINMAX_WORK"},
    "obia_crowns.h": {"OBIA_CROWNS_TILE": "CROWNS_TILE", "OBIA_E_INTERNAL": "E_INTERNAL"},
    "obia_boxes.h": {"OBIA_BOXES_TABLE": "BOXES_TABLE"},
    "obia_points.h": {"OBIA_POINTS_MAX_NZ": "POINTS_MAX_NZ", "OBIA_POINTS_CHUNK": "POINTS_CHUNK"},
    "obia_ground.h": {"OBIA_GROUND_MAX_COUNT": "GROUND_MAX_COUNT"},
    "obia_groundfilter.h": {"OBIA_MORPH_MAX_RADIUS": "MORPH_MAX_RADIUS", "OBIA_GF_MAX_STEPS": "GF_MAX_STEPS", "OBIA_MORPH_ROW_TILE": "MORPH_ROW_TILE",
                            "OBIA_MORPH_COL_TILE": "MORPH_COL_TILE", "OBIA_MORPH_COL_LANES": "MORPH_COL_LANES"},
    "obia_adjacency.h": {"OBIA_ADJ_TILE_H": "ADJ_TILE_H", "OBIA_ADJ_TILE_W": "ADJ_TILE_W", "OBIA_ADJ_TABLE": "ADJ_TABLE", "OBIA_ADJ_WORK": "ADJ_WORK"},
    "obia_shapes.h": {"OBIA_SHAPE_SUMS": "SHAPE_SUMS", "OBIA_SHAPE_TABLE": "SHAPE_TABLE"},
    "obia_merging.h": {"OBIA_MERGE_ROW_CAP": "MERGE_ROW_CAP"},
}


def code_of(header):
    """the header without its block and line comments"""
    text = open(os.path.join(INCLUDE, header), encoding="utf-8").read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def declared(header):
    return set(re.findall(r"\b(obia_[a-z0-9_]+)\s*\(", code_of(header)))


def prototypes(header):
    """name -> (return type, [parameters]) of every `type obia_name(parameters);` of the header"""
    found = re.findall(r"^[ \t]*([A-Za-z_][\w \t\*]*?)\s*\b(obia_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code_of(header), flags=re.M)
    return {name: (" ".join(ret.split()), [] if " ".join(params.split()) == "void" else [" ".join(p.split()) for p in params.split(",")])
            for ret, name, params in found}


def is_pointer_type(argtype):
    return argtype in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(argtype, type) and issubclass(argtype, ctypes._Pointer))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_the_registry_is_the_headers_and_no_name_is_bound_twice(lib):
    assert sorted(HEADERS) == sorted(os.listdir(INCLUDE)) and len(HEADERS) == 14
    names = _lib.bound_entry_points()
    assert len(names) == len(set(names)) == 129                             # the tables are pairwise disjoint
    assert names == [name for header in HEADERS for name in _lib.BINDINGS[header]]
    assert _lib.EXPORTED_SYMBOLS == tuple(_lib.BINDINGS["obia_hip.h"])       # (what __graft_entry__.build() asks the library for)
    assert lib.obia_abi_version() == 2


@pytest.mark.parametrize("header", HEADERS)
def test_a_table_is_its_header(lib, header):
    table, protos = _lib.BINDINGS[header], prototypes(header)
    assert declared(header) == set(table) == set(protos), sorted(declared(header) ^ set(table)) + sorted(set(protos) ^ set(table))
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    assert not [name for name in table if not hasattr(cdll, name)]            # the library exports every one of them
    for name, (res, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(argtypes), name   # load() bound it as written
        ret, params = protos[name]
        assert res is (ctypes.c_void_p if ret.endswith("*") and ret != "const char *" else RETURNS[ret]), (name, ret, res)
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for p, a in zip(params, argtypes):
            kind = [w for w in p.split() if w != "const"][0]
            if kind == "obia_pick_fn":
                assert a is _lib.PickFn, (name, p, a)
            elif "*" in p or "[" in p:
                assert is_pointer_type(a), (name, p, a)
            else:
                assert a is SCALARS[kind], (name, p, a)


@pytest.mark.parametrize("header", sorted(MIRRORS))
def test_the_mirrored_constants_are_the_headers(header):
    text = open(os.path.join(INCLUDE, header), encoding="utf-8").read()
    for macro, attr in MIRRORS[header].items():
        value = re.search(r"#define\s+" + macro + r"\s+\(?(-?\d+)\)?", text)
        assert value and int(value.group(1)) == getattr(_lib, attr), (macro, attr)


def test_every_mirror_is_listed_and_what_the_code_relies_on_holds():
    """a module constant of _lib.py whose comment names an OBIA_* macro is in MIRRORS; the facts the kernels' callers rely on"""
    src = open(_lib.__file__, encoding="utf-8").read()
    named = {macro for comment in re.findall(r"^[A-Z][A-Z0-9_, ]* = [^#\n]*#([^\n]*)", src, flags=re.M)
             for macro in re.findall(r"\bOBIA_[A-Z0-9_]*[A-Z0-9]\b", comment)}
    listed = {macro for macros in MIRRORS.values() for macro in macros}
    assert named and named <= listed, sorted(named - listed)
    codes = [_lib.OBIA_OK, _lib.E_INVALID, _lib.E_HIP, _lib.E_NOMEM, _lib.E_UNSUPPORTED, _lib.E_EMPTY, _lib.E_NONFINITE, _lib.E_INTERNAL]
    assert len(set(codes)) == len(codes)
    # the LDS tables are powers of two with room to spare: no overflow path (include/obia_adjacency.h, include/obia_shapes.h)
    for table in (_lib.BOXES_TABLE, _lib.ADJ_TABLE, _lib.SHAPE_TABLE):
        assert table & (table - 1) == 0
    assert _lib.ADJ_TABLE > 3 * _lib.ADJ_TILE_H * _lib.ADJ_TILE_W and _lib.SHAPE_TABLE > _lib.ADJ_TILE_H * _lib.ADJ_TILE_W
    assert (_lib.SHAPE_SUMS, _lib.SHAPE_TABLE, _lib.MERGE_ROW_CAP) == (7, 1024, 2048)
    # the restatements hold the same bounds
    from tests import ground_restatement as G
    from tests import groundfilter_restatement as GF
    assert _lib.GROUND_MAX_COUNT == G.MAX_COUNT and (_lib.MORPH_MAX_RADIUS, _lib.GF_MAX_STEPS) == (GF.MAX_RADIUS, GF.MAX_STEPS) == (127, 16)
