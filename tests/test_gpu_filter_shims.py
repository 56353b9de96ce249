"""The filtered search through the language mirrors (include/phnsw.hpp, rust/parallel-hnsw-gpu): both size their output
buffers by k, and the C call reads k 0 as "number_of_candidates entries per row" -- the wrappers must resolve that k
before they allocate and before they index the rows.  The C++ mirror is compiled with g++ against libphnsw.so and run
(tests/cpp/test_filter_shim.cpp); there is no Rust toolchain here, so the Rust wrapper is read as text, as
test_rust_shim.py reads the FFI surface."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "parallel_hnsw_amd")


def _compile(tmp_path):
    exe = str(tmp_path / "test_filter_shim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_filter_shim.cpp"), "-o", exe, "-L", LIBDIR, "-lphnsw",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_filter_shim_compiles_and_links(tmp_path):
    _compile(tmp_path)


@pytest.mark.gpu
def test_cpp_filter_shim_k0_k_cut_and_short_bitmaps(tmp_path):
    exe = _compile(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout


def test_rust_filter_shim_resolves_k_before_it_allocates():
    src = open(os.path.join(ROOT, "rust", "parallel-hnsw-gpu", "src", "lib.rs")).read()
    body = src[src.index("pub fn search_many_filtered"):]
    body = body[:body.index("\n    }\n")]
    resolve = re.search(r"let k = if k == 0 \{ sp\.number_of_candidates \} else \{ k \};", body)
    bound = re.search(r"assert!\(k <= sp\.number_of_candidates", body)
    alloc = body.index("vec![0u64; nq * k]")
    call = body.index("sys::phnsw_search_batch_filtered(")
    assert resolve and bound, "k 0 must become number_of_candidates, and k may not exceed it"
    assert resolve.end() < bound.start() < alloc < call
    assert "k as u64" in body[call:]  # the C call gets the resolved k: rows are written and read with one stride
