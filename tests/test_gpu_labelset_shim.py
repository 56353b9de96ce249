"""phnsw_search_exact_labelset through the C++ mirror (include/phnsw.hpp): Hnsw::search_many_exact_labelset compiled with
g++ against libphnsw.so and run (tests/cpp/test_labelset_shim.cpp) -- one batch against the rows the Python side computes
for the same vectors, labels and sets, against search_many_exact_filtered's with the union bitmaps, and the arguments it
refuses before the library is called.  There is no Rust toolchain here; test_rust_shim.py compares the Rust declarations
with the header."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "parallel_hnsw_amd")
NONE = 0xFFFFFFFF


def _compile(tmp_path):
    exe = str(tmp_path / "test_labelset_shim")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_labelset_shim.cpp"), "-o", exe, "-L", LIBDIR, "-lphnsw",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_labelset_shim_compiles_and_links(tmp_path):
    _compile(tmp_path)


def python_rows():
    """the program's vectors, labels and sets through Hnsw.search_exact_labelset -> (ids, d, len) at k = 40"""
    import parallel_hnsw_amd as ph
    from test_gpu_exact_filter import ring
    wide = np.array([((i * 37 % 17) - 8) / 8.0 for i in range(33 * 3)], dtype=np.float32).reshape(33, 3)
    store = ph.VectorStore(wide, metric=ph.METRIC_ONE_MINUS_DOT)
    hix = ph.Hnsw.from_layers(store, ring(np.arange(33)))
    lab = np.array([0xFFFFFFFE if v == 32 else (NONE if v == 1 else (70000 if v % 2 == 0 else 5)) for v in range(33)])
    sets = [[70000, 5], [0xFFFFFFFE], [999, NONE], [5, 5, 0xFFFFFFFE], [], [5, 999, 70000, 0xFFFFFFFE], [70000]]
    return hix.search_exact_labelset(queries=wide[:7], labels=ph.Labels(hix, lab), want=sets, k=40)


@pytest.mark.gpu
def test_cpp_labelset_shim_rows_and_refusals(tmp_path):
    exe = _compile(tmp_path)
    ids, d, ln = python_rows()
    assert ln.tolist() == [31, 1, 0, 16, 0, 32, 16]
    rows = tmp_path / "rows.txt"
    with open(rows, "w") as f:
        for i in range(7):
            n = int(ln[i])
            f.write(" ".join([str(n)] + ["%d %d" % (int(ids[i, j]), int(d[i, j:j + 1].view(np.uint32)[0])) for j in range(n)]) + "\n")
    r = subprocess.run([exe, str(rows)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
