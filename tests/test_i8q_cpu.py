"""CPU-only checks of the i8q store (int8 rows, int8 query, integer dot products).  The yardstick first: on `lattice`
rows (codes times a power of two) the numpy restatement of the i8q distance equals, bit for bit, the unchanged f32
oracle over the dequantised rows in both of its summation orders -- every partial sum of the oracle is an integer
multiple of one power of two and stays below 2^24, so no addition rounds -- which is what lets the GPU tests check an
i8q search against that oracle.  Then the new prototypes: declared alike in the header, the ctypes table, phnsw.hpp and
both Rust crates, and failing with the library's error where there is no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from parallel_hnsw_amd import _lib

import i8q_reference
from i8_reference import dequantize, quantize
from test_i8_cpu import args_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"phnsw_store_create_i8q": 2, "phnsw_i8q_search_batch": 9, "phnsw_i8q_search_batch_device": 13}
DIMS = [6, 100, 768, 1040, 1536]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("dim", DIMS)
def test_lattice_rows_quantise_to_their_own_codes_and_scales(dim):
    rows, c, k = i8q_reference.lattice(200, dim, np.random.default_rng(dim))
    codes, scales = quantize(rows)
    np.testing.assert_array_equal(codes, c)
    np.testing.assert_array_equal(bits(scales), bits(np.exp2(k.astype(np.float64)).astype(np.float32)))
    np.testing.assert_array_equal(bits(dequantize(codes, scales)), bits(rows))
    assert (np.abs(c).max(axis=1) == 127).all()


@pytest.mark.parametrize("metric", [oracle.METRIC_COSINE_HALF, oracle.METRIC_ONE_MINUS_DOT])
@pytest.mark.parametrize("dim", DIMS)
def test_the_unchanged_oracle_gives_the_i8q_distance_on_lattice_rows(dim, metric):
    rng = np.random.default_rng(1000 + dim)
    rows, c, k = i8q_reference.lattice(120, dim, rng)
    queries, cq, kq = i8q_reference.lattice(4, dim, rng)
    # the bound the argument needs, on these inputs: no partial sum of |cq * cr| reaches 2^24
    assert int(np.abs(c.astype(np.int64)).sum(axis=1).max()) * 127 < 2 ** 24
    codes, scales = quantize(rows)
    ix = oracle.Index(rows, metric=metric)
    for q in queries:
        want = i8q_reference.distance(q, codes, scales, metric)
        for mode in (oracle.SUM_BLOCKED64, oracle.SUM_SEQ):
            got = np.array([ix.distance(q, r, mode) for r in rows], dtype=np.float32)
            np.testing.assert_array_equal(bits(got), bits(want))
    # a stored query: the row's own codes and scale
    want = i8q_reference.distance_codes(codes[3], scales[3], codes, scales, metric)
    got = np.array([ix.distance(rows[3], r, oracle.SUM_BLOCKED64) for r in rows], dtype=np.float32)
    np.testing.assert_array_equal(bits(got), bits(want))


def test_reference_distance_on_hand_made_values():
    codes = np.array([[127, -3, 0, 2], [0, 0, 0, 0], [-127, 127, 127, -127]], dtype=np.int8)
    scales = np.array([0.5, 0.0, 0.25], dtype=np.float32)
    q = np.array([127.0, 1.0, -2.0, 0.0], dtype=np.float32)  # quantises to itself with scale 1
    d = i8q_reference.distance(q, codes, scales, oracle.METRIC_ONE_MINUS_DOT)
    np.testing.assert_array_equal(d, np.array([1 - 0.5 * (127 * 127 - 3), 1.0, 1 - 0.25 * (-127 * 127 + 127 - 254)], dtype=np.float32))
    z = i8q_reference.distance(np.zeros(4, dtype=np.float32), codes, scales, oracle.METRIC_COSINE_HALF)
    np.testing.assert_array_equal(z, np.full(3, 0.5, dtype=np.float32))  # a query of zeros: scale 0, dot 0


def test_new_prototypes_are_declared_everywhere_with_matching_argument_counts():
    strip = lambda s: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", s, flags=re.S))
    header = strip(open(os.path.join(ROOT, "include", "phnsw.h")).read())
    hpp = strip(open(os.path.join(ROOT, "include", "phnsw.hpp")).read())
    sys_rs = strip(open(os.path.join(ROOT, "rust", "phnsw-sys", "src", "lib.rs")).read())
    gpu_rs = strip(open(os.path.join(ROOT, "rust", "parallel-hnsw-gpu", "src", "lib.rs")).read())
    L = C.CDLL(_lib.LIB_PATH)
    for name, argc in NEW.items():
        assert args_of(header, r"\bint\s+%s\s*\(" % name) == argc, name + ": include/phnsw.h"
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == argc, name + ": _lib.SYMBOLS"
        assert hasattr(L, name), "libphnsw.so does not export " + name
        assert hasattr(ph.lib(), name)
        assert args_of(hpp, r"\b%s\s*\(" % name) == argc, name + ": include/phnsw.hpp"
        assert args_of(sys_rs, r"\bpub\s+fn\s+%s\s*\(" % name) == argc, name + ": phnsw-sys"
        assert args_of(gpu_rs, r"\bsys::%s\s*\(" % name) == argc, name + ": parallel-hnsw-gpu"
    assert issubclass(ph.I8QStore, ph.VectorStore) and not issubclass(ph.I8QStore, ph.I8Store)
    assert ph.I8QStore.from_full and ph.I8QStore.codes and ph.I8QStore.scales


def test_null_arguments_are_invalid():
    out = C.c_void_p()
    assert ph.lib().phnsw_store_create_i8q(None, C.byref(out)) == -1  # PHNSW_E_INVALID
    assert b"phnsw_store_create_i8q" in ph.lib().phnsw_last_error()
    assert not out.value
    sp = ph.SearchParameters(16, 16, 2)
    assert ph.lib().phnsw_i8q_search_batch(None, None, None, 0, C.byref(sp), 1, None, None, None) == -1
    assert b"phnsw_i8q_search_batch" in ph.lib().phnsw_last_error()
    assert ph.lib().phnsw_i8q_search_batch_device(None, None, None, 0, 0, C.byref(sp), 1, None, None, None, None, None,
                                                  None) == -1


@pytest.mark.skipif(ph.lib().phnsw_device_count() != 0, reason="a GPU is visible")
def test_no_cpu_fallback():
    fake = C.create_string_buffer(4096)
    out = C.c_void_p()
    assert ph.lib().phnsw_store_create_i8q(C.cast(fake, C.c_void_p), C.byref(out)) == -2  # PHNSW_E_NO_DEVICE
    assert not out.value
