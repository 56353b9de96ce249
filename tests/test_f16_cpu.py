"""CPU-only checks of the f16 store's surface: the new prototypes are in the header, in the ctypes table and exported
by the built library, and without a GPU the calls fail with the library's error instead of crashing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("phnsw_store_create_f16", "phnsw_f16_search_batch", "phnsw_f16_search_batch_device")


def test_new_prototypes_are_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "phnsw.h")).read(), flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in include/phnsw.h"
        assert name in _lib.SYMBOLS, name + " is not in _lib.SYMBOLS"
        assert hasattr(L, name), "libphnsw.so does not export " + name
        assert hasattr(ph.lib(), name)
    hpp = open(os.path.join(ROOT, "include", "phnsw.hpp")).read()
    assert "phnsw_store_create_f16" in hpp and "phnsw_f16_search_batch" in hpp
    assert ph.F16Store.from_full and ph.Hnsw.search_batch_reranked


def test_create_f16_rejects_null():
    out = C.c_void_p()
    assert ph.lib().phnsw_store_create_f16(None, C.byref(out)) == -1  # PHNSW_E_INVALID
    assert b"phnsw_store_create_f16" in ph.lib().phnsw_last_error()
    assert not out.value
    sp = ph.SearchParameters(16, 16, 2)
    assert ph.lib().phnsw_f16_search_batch(None, None, None, 0, C.byref(sp), 1, None, None, None) == -1
    assert ph.lib().phnsw_f16_search_batch_device(None, None, None, 0, 0, C.byref(sp), 1, None, None, None, None, None,
                                                  None) == -1


@pytest.mark.skipif(ph.lib().phnsw_device_count() != 0, reason="a GPU is visible")
def test_no_cpu_fallback():
    """F16Store.from_full needs an f32 store, which cannot exist without a GPU: the path fails with the library's error"""
    with pytest.raises(ph.PhnswError) as e:
        ph.F16Store.from_full(ph.VectorStore(np.zeros((4, 8), dtype=np.float32)))
    assert e.value.code == -2  # PHNSW_E_NO_DEVICE
