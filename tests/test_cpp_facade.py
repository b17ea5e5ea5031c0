"""C++ facade (include/supersonic_amd/supersonic.h) over the C ABI: the reference's own
builder API (supersonic/supersonic.h) driven from C++ exactly as its guide tests do."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "facade_test.cc")
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "facade_test")
LIBDIR = os.path.join(ROOT, "supersonic_amd", "lib")


@pytest.fixture(scope="module")
def facade_bin():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "ssgpu.h"), os.path.join(ROOT, "include", "supersonic_amd", "supersonic.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        # pytest-xdist may hand this module's two tests to different workers: build under a private name and move the
        # finished binary into place (a worker must never execute a half-written file)
        tmp = "%s.%d.tmp" % (OUT, os.getpid())
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC, "-o", tmp,
                               "-L" + LIBDIR, "-lssgpu", "-Wl,-rpath," + LIBDIR])
        os.replace(tmp, OUT)
    return OUT


def _run(binary, mode):
    p = subprocess.run([binary, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert p.returncode == 0, p.stdout
    assert "PASSED" in p.stdout


def test_facade_bind(facade_bin):
    _run(facade_bin, "bind")


@pytest.mark.gpu
def test_facade_run(facade_bin):
    _run(facade_bin, "run")


# ---- reference-style user code against the reference's include path: tests/cpp/guide_test.cc includes ONLY
# "supersonic/supersonic.h" and is built with -I<repo>/include (C++14, as plain as a user's build line gets) -------------
GUIDE_SRC = os.path.join(ROOT, "tests", "cpp", "guide_test.cc")
GUIDE_OUT = os.path.join(ROOT, "tests", "cpp", "_build", "guide_test")


@pytest.fixture(scope="module")
def guide_bin():
    os.makedirs(os.path.dirname(GUIDE_OUT), exist_ok=True)
    deps = [GUIDE_SRC, os.path.join(ROOT, "include", "ssgpu.h"), os.path.join(ROOT, "include", "supersonic_amd", "supersonic.h"),
            os.path.join(ROOT, "include", "supersonic", "supersonic.h")]
    if not os.path.exists(GUIDE_OUT) or any(os.path.getmtime(d) > os.path.getmtime(GUIDE_OUT) for d in deps):
        tmp = "%s.%d.tmp" % (GUIDE_OUT, os.getpid())
        subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), GUIDE_SRC, "-o", tmp,
                               "-L" + LIBDIR, "-lssgpu", "-Wl,-rpath," + LIBDIR])
        os.replace(tmp, GUIDE_OUT)
    return GUIDE_OUT


def test_guide_style_program_builds_and_binds(guide_bin):
    with open(GUIDE_SRC) as f:
        includes = [line.strip() for line in f if line.startswith("#include \"")]
    assert includes == ['#include "supersonic/supersonic.h"']        # the reference's umbrella header, nothing of this repository's own
    _run(guide_bin, "bind")


@pytest.mark.gpu
def test_guide_style_program_runs(guide_bin):
    _run(guide_bin, "run")


# ---- the reference's OWN guide programs, unchanged: the reference checkout's test/guide/{primer,group_sort}.cc are compiled where
# they lie (nothing is copied) against -I<repo>/include and linked with libssgpu; the binaries are built into oracle/_ref/ by
# __graft_entry__.build() where the reference exists and travel to the GPU machine with the tree, where they RUN: every TEST of the guide --
# bound a + b, Compute, Filter, grouped aggregates with STRING + BOOL keys, Sort drained 1024 rows at a time into a Block
# through ViewCopier -- must pass against the MI355X library ------------------------------------------------------------
from oracle import build_ref_guides  # noqa: E402


@pytest.mark.parametrize("name", build_ref_guides.GUIDES)
def test_reference_guide_compiles_and_links_unchanged(name):
    if not os.path.exists(build_ref_guides.source(name)):
        pytest.skip("no reference checkout here (the GPU machine): the binary build() left in oracle/_ref/ is what runs")
    out = build_ref_guides.build(name)
    assert out and os.access(out, os.X_OK)
    # and under -Wall -Werror as a pure syntax check of the facade's surface the guide touches
    # (-Wno-sign-compare: the guide itself compares an int loop index with an unsigned count, group_sort.cc:550)
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror", "-Wno-sign-compare", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "tests", "cpp", "minigtest"), build_ref_guides.source(name)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", build_ref_guides.GUIDES)
def test_reference_guide_runs_green(name):
    """The binary is built where a reference checkout exists (__graft_entry__.build(), into oracle/_ref/) and travels to the GPU machine
    with the tree.  build() leaves oracle/_ref/EXPECTED next to it: where that file (or SSGPU_EXPECT_REF_GUIDES=1) says the binaries
    were built, a missing one FAILS -- a skip here would read as a pass."""
    out = build_ref_guides.build(name) or build_ref_guides.binary(name)
    expected = os.environ.get("SSGPU_EXPECT_REF_GUIDES") == "1" or name in build_ref_guides.expected()
    if not os.path.exists(out):
        assert not expected, "oracle/_ref/ref_guide_%s is expected (oracle/_ref/EXPECTED / SSGPU_EXPECT_REF_GUIDES) and missing" % name
        pytest.skip("oracle/_ref/ref_guide_%s was not built (no reference checkout where this tree was built)" % name)
    p = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, text=True)
    assert p.returncode == 0 and "[  PASSED  ]" in p.stdout and "FAILED" not in p.stdout, p.stdout[-4000:]
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "ref_guides_ran.txt"), "a") as f:
            passed = [ln.strip() for ln in p.stdout.splitlines() if "[       OK ]" in ln]
            f.write("ref_guide_%s: rc 0, %d TESTs OK: %s\n" % (name, len(passed), "; ".join(passed)))
    except OSError:
        pass


# ---- the C++ host's multi-GPU driver (include/supersonic_amd/sharded.h): RCCL linked directly ---------------------------
SHARDED_SRC = os.path.join(ROOT, "tests", "cpp", "sharded_test.cc")
SHARDED_OUT = os.path.join(ROOT, "tests", "cpp", "_build", "sharded_test")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def sharded_bin():
    os.makedirs(os.path.dirname(SHARDED_OUT), exist_ok=True)
    deps = [SHARDED_SRC, os.path.join(ROOT, "include", "ssgpu.h"), os.path.join(ROOT, "include", "supersonic_amd", "supersonic.h"),
            os.path.join(ROOT, "include", "supersonic_amd", "sharded.h")]
    if not os.path.exists(SHARDED_OUT) or any(os.path.getmtime(d) > os.path.getmtime(SHARDED_OUT) for d in deps):
        tmp = "%s.%d.tmp" % (SHARDED_OUT, os.getpid())
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROCM, "include"), SHARDED_SRC, "-o", tmp, "-L" + LIBDIR, "-lssgpu", "-Wl,-rpath," + LIBDIR,
                               "-L" + os.path.join(ROCM, "lib"), "-lrccl", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib")])
        os.replace(tmp, SHARDED_OUT)
    return SHARDED_OUT


def test_sharded_driver_builds_against_rccl(sharded_bin):
    _run(sharded_bin, "build-only")


@pytest.mark.gpu
def test_sharded_driver_runs_one_rank(sharded_bin):
    _run(sharded_bin, "run")
