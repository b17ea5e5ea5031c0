"""ForeignFilter and RowidMergeJoin through the C++ mirror: tests/cpp/structured_filter_test.cc includes only the reference's two
include paths for the operators (include/supersonic/cursor/core/foreign_filter.h, rowid_merge_join.h) and is built the way
tests/test_cpp_facade.py builds its programs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "structured_filter_test.cc")
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "structured_filter_test")
LIBDIR = os.path.join(ROOT, "supersonic_amd", "lib")
HEADERS = [os.path.join(ROOT, "include", "supersonic", "cursor", "core", "foreign_filter.h"),
           os.path.join(ROOT, "include", "supersonic", "cursor", "core", "rowid_merge_join.h")]


@pytest.fixture(scope="module")
def structured_filter_bin():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "ssgpu.h"), os.path.join(ROOT, "include", "supersonic_amd", "supersonic.h")] + HEADERS
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        tmp = "%s.%d.tmp" % (OUT, os.getpid())     # (a worker must never execute a half-written file: build aside, move into place)
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC, "-o", tmp,
                               "-L" + LIBDIR, "-lssgpu", "-Wl,-rpath," + LIBDIR])
        os.replace(tmp, OUT)
    return OUT


def _run(binary, mode):
    p = subprocess.run([binary, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert p.returncode == 0, p.stdout
    assert "PASSED" in p.stdout


def test_the_program_includes_only_the_two_forwarding_headers():
    with open(SRC) as f:
        includes = [line.strip() for line in f if line.startswith("#include \"")]
    assert includes == ['#include "supersonic/cursor/core/foreign_filter.h"', '#include "supersonic/cursor/core/rowid_merge_join.h"']
    for h in HEADERS:
        with open(h) as f:
            code = [ln.strip() for ln in f if ln.strip() and not ln.startswith("//")]
        assert len(code) == 4 and code[2] == '#include "../../../supersonic_amd/supersonic.h"', h       # a guard and the one include


def test_structured_filter_bind(structured_filter_bin):
    _run(structured_filter_bin, "bind")


@pytest.mark.gpu
def test_structured_filter_run(structured_filter_bin):
    _run(structured_filter_bin, "run")
