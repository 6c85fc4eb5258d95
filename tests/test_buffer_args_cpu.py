"""The argument checks of the entry layer without a GPU (obia_amd/csrc/buffer_args.hpp; DESIGN.md, "The entry layer").

tests/buffer_args_check.cpp is a program of its own: it includes the header, keeps the functions and the conditions the header
replaced, and compares the two over pointers made from integers -- every residue of every element size, null / optional / needed if
n > 0, every overlap rule, the capacity, five real entry points over every combination of {null, aligned, one element on, one byte on,
where output 0 starts} per argument, and the text and code of every refusal.  It is built here with the host compiler and
-fsanitize=address,undefined and run once.  More buffers than the capacity are refused when the call runs (bad()), not by the compiler.

The rest reads the sources: no entry point of obia_amd/csrc keeps a check of the old spellings, and no file a refusal helper of its own."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "obia_amd", "csrc")
PROGRAM = os.path.join(ROOT, "tests", "buffer_args_check.cpp")
CONVERTED = ("seed_table", "boxes", "points", "ground", "groundfilter", "adjacency", "shapes", "merging", "sharpness", "training", "crowns")


def host_compiler():
    for cxx in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    raise AssertionError("no host C++ compiler (g++ or clang++) was found")


def hip_sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(".hip")}


def test_the_checker_gives_the_verdicts_of_the_expressions_it_replaced(tmp_path):
    exe = str(tmp_path / "buffer_args_check")
    build = subprocess.run([host_compiler(), "-std=c++17", "-Wall", "-Werror", "-O1", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", PROGRAM, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-4000:] + run.stderr[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    m = re.fullmatch(r"(\d+) checks, 0 failed", last)
    assert m and int(m.group(1)) > 1_000_000, last
    swept = re.findall(r"^(\S+: [a-z ]+?)\s+n1 \d+ n2 \d+: (\d+) cases, (\d+) refused$", run.stdout, re.M)
    assert {s[0] for s in swept} == {"boxes: pair write", "points: segment columns", "merging: pairs", "ground: query", "sharpness: box"}
    assert all(0 < int(refused) < int(cases) for _, cases, refused in swept)


@pytest.mark.parametrize("macro, why", [("TRY_VOID", "Pointee<void>"), ("TRY_CONST_OUT", "deleted")])
def test_a_pointer_to_void_or_an_output_to_const_does_not_compile(macro, why):
    cxx = host_compiler()
    ok = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", PROGRAM], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    bad = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-D" + macro, PROGRAM], capture_output=True, text=True)
    assert bad.returncode != 0 and why in bad.stderr, bad.stderr


def test_the_header_stands_alone():
    """no HIP header, and nothing of the library but the status codes and the declaration of set_error"""
    text = open(os.path.join(CSRC, "buffer_args.hpp")).read()
    assert re.findall(r"#include\s+(\S+)", text) == ["<cstddef>", "<cstdint>", '"../../include/obia_hip.h"']
    assert "hip/" not in open(os.path.join(ROOT, "include", "obia_hip.h")).read()
    assert len(text.splitlines()) < 150


def test_no_entry_point_keeps_a_check_of_the_old_spellings():
    sources = hip_sources()
    assert set(f + ".hip" for f in CONVERTED) <= set(sources)
    for f, text in sources.items():
        code = "\n".join(line.split("//")[0] for line in text.splitlines())
        assert not re.search(r"\bmisaligned\s*\([^()]*,", code), f"{f}: misaligned(p, a)"
        assert not re.search(r"\bshared_start\s*\(", code), f"{f}: shared_start"
        if f[:-4] in CONVERTED:
            # an argument check: an if whose condition -- up to the brace or the return that follows it -- tests pointer bits.  The
            # kernels' own byte arithmetic (`const int a = (int)((uintptr_t)out & 3);`) stands in no if and is not meant
            for m in re.finditer(r"\bif\s*\((?:(?!\{|\breturn\b|;).)*", code, re.S):
                assert not re.search(r"\(uintptr_t\)\s*\w+\s*&\s*(3|7)\b", m.group(0)), f"{f}: {m.group(0)[:120]}"
    common = open(os.path.join(CSRC, "common.hpp")).read()
    assert "shared_start" not in common and "misaligned(" not in common


def test_the_kernels_byte_arithmetic_is_not_what_the_pattern_above_catches():
    """image.hip and training.hip keep `(uintptr_t)p & 3` inside kernels: the source still has it, the argument-check pattern passes it by"""
    for f in ("image.hip", "training.hip"):
        assert re.search(r"\(uintptr_t\)\s*\w+\s*&\s*3\b", hip_sources()[f]), f


def test_no_file_keeps_a_refusal_helper_of_its_own():
    for f, text in hip_sources().items():
        for name in ("bad_buffers", "check_n", "check_raster", "check_labels", "check_count", "csr_missing", "tables_missing", "check_cloud"):
            assert not re.search(r"\b%s\s*\(" % name, text), f"{f}: {name}"


def test_the_csr_is_defined_once():
    texts = [open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".cpp"))]
    assert sum(len(re.findall(r"\bstruct\s+Csr\b", t)) for t in texts) == 1
    assert sum(len(re.findall(r"\bCsr\s+csr_of\s*\(", t)) for t in texts) == 1
    for f in ("adjacency.hip", "merging.hip"):
        assert '#include "csr.hpp"' in hip_sources()[f]


def test_the_makefile_rebuilds_on_the_new_headers():
    hdrs = re.search(r"^HDRS\s*=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "buffer_args.hpp" in hdrs and "csr.hpp" in hdrs
