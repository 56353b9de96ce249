"""The searches by a set of row labels and a numeric range through the C++ mirror (include/phnsw.hpp):
Hnsw::search_many_exact_labelset_ranged / search_many_labelset_ranged / search_many_labelset_ranged_auto compiled with g++
against libphnsw.so and run (tests/cpp/test_labelset_ranged_shim.cpp) -- one exact call and one routed call against the C
ABI's rows, all three against the bitmap calls with the equivalent bitmaps per query, one-label sets against the calls by
label and range, and the arguments they refuse before the library is called.  There is no Rust toolchain here;
test_rust_shim.py compares the Rust declarations with the header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "parallel_hnsw_amd")


def _compile(tmp_path):
    exe = str(tmp_path / "test_labelset_ranged_shim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_labelset_ranged_shim.cpp"), "-o", exe, "-L", LIBDIR, "-lphnsw",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_labelset_ranged_shim_compiles_and_links(tmp_path):
    _compile(tmp_path)


@pytest.mark.gpu
def test_cpp_labelset_ranged_shim_rows_and_refusals(tmp_path):
    exe = _compile(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
