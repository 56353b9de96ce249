"""What phnsw_search_exact_grouped[_device] answer without a GPU, and the argument handling of
Hnsw.search_exact_grouped that runs before any device call.  No index can exist without a device, so the first check of
the header's order -- a null index -- is the one both entry points reach here: PHNSW_E_INVALID with a message that names
the call, never a crash and never a quiet success."""
import ctypes as C

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd import _lib
from parallel_hnsw_amd.hnsw import Hnsw, pack_allow_of, pack_allow_table

N = 70  # three bitmap words, the last one ragged


def last_error():
    return ph.lib().phnsw_last_error().decode()


def test_the_entry_points_are_bound_with_the_header_s_arity():
    # the scan's arguments plus nfilters and filter_of
    assert len(_lib.SYMBOLS["phnsw_search_exact_grouped"][1]) == len(_lib.SYMBOLS["phnsw_search_exact_filtered"][1]) + 2 == 13
    assert len(_lib.SYMBOLS["phnsw_search_exact_grouped_device"][1]) == 16
    assert len(_lib.SYMBOLS["phnsw_search_exact_filtered_device"][1]) + 2 == 16
    assert ph.FILTER_ALL == 0xFFFFFFFF


def test_a_null_index_is_refused_first_by_both_entry_points():
    L = ph.lib()
    buf = (C.c_uint64 * 8)()
    for k in (10, 0, 1025):  # the index is looked at before k
        assert L.phnsw_search_exact_grouped(None, buf, None, 1, None, buf, 3, 1, buf, k, buf, buf, buf) == -1
        assert last_error() == "phnsw_search_exact_grouped: null index or index without layers"
        assert L.phnsw_search_exact_grouped_device(None, None, 0, buf, 1, None, buf, 3, 1, buf, k, buf, buf, buf, buf, None) == -1
        assert last_error() == "phnsw_search_exact_grouped_device: null index or index without layers"
    # ... and before nq == 0 is taken as a no-op
    assert L.phnsw_search_exact_grouped(None, None, None, 0, None, None, 0, 0, None, 10, None, None, None) == -1
    assert L.phnsw_search_exact_grouped_device(None, None, 0, None, 0, None, None, 0, 0, None, 10, None, None, None, None,
                                               None) == -1


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
    masks = np.ones((2, N), dtype=bool)
    of = np.array([0, 1, -1])
    with pytest.raises(ValueError, match="exactly one"):
        ix.search_exact_grouped(allows=masks, allow_of=of)
    with pytest.raises(ValueError, match="exactly one"):
        ix.search_exact_grouped(queries=q, qids=np.arange(3), allows=masks, allow_of=of)
    with pytest.raises(ValueError, match="allows"):  # no table
        ix.search_exact_grouped(queries=q, allow_of=of)
    with pytest.raises(ValueError, match="allows"):  # one mask is not a table
        ix.search_exact_grouped(queries=q, allows=np.ones(N, dtype=bool), allow_of=of)
    with pytest.raises(ValueError, match="allows"):  # masks of the wrong length
        ix.search_exact_grouped(queries=q, allows=np.ones((2, N - 1), dtype=bool), allow_of=of)
    with pytest.raises(ValueError, match="allows"):  # packed words shorter than one bitmap
        ix.search_exact_grouped(queries=q, allows=np.zeros((2, 2), dtype=np.uint32), allow_of=of)
    with pytest.raises(ValueError, match="allows"):  # an empty table
        ix.search_exact_grouped(queries=q, allows=np.zeros((0, N), dtype=bool), allow_of=of)
    with pytest.raises(TypeError, match="allows"):
        ix.search_exact_grouped(queries=q, allows=np.ones((2, N), dtype=np.int64), allow_of=of)
    with pytest.raises(ValueError, match="allow_of"):  # none
        ix.search_exact_grouped(queries=q, allows=masks)
    with pytest.raises(ValueError, match="allow_of"):  # the wrong length
        ix.search_exact_grouped(queries=q, allows=masks, allow_of=np.array([0, 1]))
    with pytest.raises(ValueError, match="allow_of"):  # below -1
        ix.search_exact_grouped(queries=q, allows=masks, allow_of=np.array([0, 1, -2]))
    with pytest.raises(TypeError, match="allow_of"):
        ix.search_exact_grouped(queries=q, allows=masks, allow_of=np.array([0.0, 1.0, 1.0]))
    # well-formed arguments reach the library, which refuses the null index by name
    for allows in (masks, np.zeros((2, 3), dtype=np.uint32), np.zeros((2, 5), dtype=np.uint32)):
        with pytest.raises(ph.PhnswError) as e:
            ix.search_exact_grouped(queries=q, allows=allows, allow_of=of, k=5)
        assert e.value.code == -1 and "phnsw_search_exact_grouped:" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:
        ix.search_exact_grouped_device(3, 5, 8, 8, 8, 8, qids=8, allows=8, allow_stride=3, nallows=2, allow_of=8)
    assert e.value.code == -1 and "phnsw_search_exact_grouped_device:" in str(e.value)


def test_selectors_and_tables_pack_as_the_header_wants_them():
    np.testing.assert_array_equal(pack_allow_of(np.array([0, -1, 3, ph.FILTER_ALL]), 4),
                                  np.array([0, 0xFFFFFFFF, 3, 0xFFFFFFFF], dtype=np.uint32))
    assert pack_allow_of(np.array([2], dtype=np.uint32), 1).dtype == np.uint32
    m = np.zeros((2, N), dtype=bool)
    m[0, [0, 31, 32, 69]] = True
    m[1, 33] = True
    words, stride = pack_allow_table(m, N)
    assert stride == 3 and words.dtype == np.uint32 and words.shape == (2, 3)
    assert words.tolist() == [[0x80000001, 1, 1 << 5], [0, 2, 0]]
    wide = np.arange(10, dtype=np.uint32).reshape(2, 5)  # packed words pass through, the row length is the stride
    words, stride = pack_allow_table(wide, N)
    assert stride == 5 and words.shape == (2, 5) and (words == wide).all()
