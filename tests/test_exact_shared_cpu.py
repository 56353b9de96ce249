"""What phnsw_search_exact_shared[_device] and phnsw_exact_shared_supported answer without a GPU, and the argument
handling of Hnsw.search_exact_shared that runs before any device call.  No index can exist without a device, so the
first check of the header's order -- a null index -- is the one every entry point reaches here: PHNSW_E_INVALID with a
message that names the call, never a crash and never a quiet success."""
import ctypes as C

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd import _lib
from parallel_hnsw_amd.hnsw import Hnsw, pack_allow

N = 70  # three bitmap words, the last one ragged


def last_error():
    return ph.lib().phnsw_last_error().decode()


def test_the_entry_points_are_bound_with_the_header_s_arity():
    assert len(_lib.SYMBOLS["phnsw_exact_shared_supported"][1]) == 2
    assert len(_lib.SYMBOLS["phnsw_search_exact_shared"][1]) == 10
    assert len(_lib.SYMBOLS["phnsw_search_exact_shared_device"][1]) == 13
    # the scan's arguments without filter_stride_words
    assert len(_lib.SYMBOLS["phnsw_search_exact_filtered"][1]) == 11
    assert len(_lib.SYMBOLS["phnsw_search_exact_filtered_device"][1]) == 14


def test_a_null_index_is_refused_first_by_every_entry_point():
    L = ph.lib()
    buf = (C.c_uint64 * 8)()
    for k in (10, 0, 1025):  # the index is looked at before k
        assert L.phnsw_exact_shared_supported(None, k) == -1
        assert last_error() == "phnsw_exact_shared_supported: null index or index without layers"
        assert L.phnsw_search_exact_shared(None, buf, None, 1, None, None, k, buf, buf, buf) == -1
        assert last_error() == "phnsw_search_exact_shared: null index or index without layers"
        assert L.phnsw_search_exact_shared_device(None, None, 0, buf, 1, None, None, k, buf, buf, buf, buf, None) == -1
        assert last_error() == "phnsw_search_exact_shared_device: null index or index without layers"
    # ... and before nq == 0 is taken as a no-op
    assert L.phnsw_search_exact_shared(None, None, None, 0, None, None, 10, None, None, None) == -1
    assert L.phnsw_search_exact_shared_device(None, None, 0, None, 0, None, None, 10, None, None, None, None, None) == -1


class FakeStore:
    n, dim = N, 4


def fake_index():
    """an Hnsw whose library handle is null: what the Python method does before the call, and that the call then fails"""
    ix = Hnsw.__new__(Hnsw)
    ix._h = None
    ix.store = FakeStore()
    return ix


def test_python_argument_handling_runs_before_the_call():
    ix = fake_index()
    q = np.zeros((3, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="exactly one"):
        ix.search_exact_shared()
    with pytest.raises(ValueError, match="exactly one"):
        ix.search_exact_shared(queries=q, qids=np.arange(3))
    with pytest.raises(ValueError, match="ONE bitmap"):  # a 2-D mask, bool or packed
        ix.search_exact_shared(queries=q, allow=np.ones((3, N), dtype=bool))
    with pytest.raises(ValueError, match="ONE bitmap"):
        ix.search_exact_shared(queries=q, allow=np.zeros((3, 3), dtype=np.uint32))
    with pytest.raises(ValueError):  # a mask of the wrong length
        ix.search_exact_shared(queries=q, allow=np.ones(N - 1, dtype=bool))
    with pytest.raises(ValueError):  # packed words shorter than one bitmap
        ix.search_exact_shared(queries=q, allow=np.zeros(2, dtype=np.uint32))
    with pytest.raises(TypeError):
        ix.search_exact_shared(queries=q, allow=np.ones(N, dtype=np.int64))
    # well-formed arguments reach the library, which refuses the null index by name
    for allow in (None, np.ones(N, dtype=bool), np.zeros(3, dtype=np.uint32)):
        with pytest.raises(ph.PhnswError) as e:
            ix.search_exact_shared(queries=q, allow=allow, k=5)
        assert e.value.code == -1 and "phnsw_search_exact_shared:" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:
        ix.search_exact_shared_device(3, 5, 8, 8, 8, 8, qids=8)
    assert e.value.code == -1 and "phnsw_search_exact_shared_device:" in str(e.value)
    assert ix.exact_shared_supported(5) == -1


def test_one_mask_packs_to_one_shared_bitmap():
    m = np.zeros(N, dtype=bool)
    m[[0, 31, 32, 69]] = True
    words, stride = pack_allow(m, N, 3)
    assert stride == 0 and words.dtype == np.uint32
    assert words.tolist() == [0x80000001, 1, 1 << 5]
