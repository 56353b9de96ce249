"""The calls by a SET of row labels that walk the graph (phnsw_search_batch_labelset, phnsw_search_labelset_auto and their
device forms) without a GPU: the bindings' arity, what the library answers to a null index, and the argument handling of
the Python wrappers, which runs before any library call -- a handle that is no Labels, both or neither of queries / qids,
and every malformed `want` that pack_label_sets refuses."""
import ctypes as C

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd import _lib

from test_exact_labeled_cpu import N, fake_index, fake_labels, last_error


def test_the_entry_points_are_bound_with_the_header_s_arity():
    # (want_first, want_values) in place of want: one argument more; the device forms take nwant as well: two more
    for name, twin, more in (("phnsw_search_batch_labelset", "phnsw_search_batch_labeled", 1),
                             ("phnsw_search_batch_labelset_device", "phnsw_search_batch_labeled_device", 2),
                             ("phnsw_search_labelset_auto", "phnsw_search_labeled_auto", 1),
                             ("phnsw_search_labelset_auto_device", "phnsw_search_labeled_auto_device", 2)):
        assert len(_lib.SYMBOLS[name][1]) == len(_lib.SYMBOLS[twin][1]) + more, name
        assert hasattr(ph.lib(), name)


def test_a_null_index_is_refused_first_by_every_form():
    L = ph.lib()
    buf = (C.c_uint64 * 8)()
    sp = ph.SearchParameters(16, 16, 2)
    assert L.phnsw_search_batch_labelset(None, None, buf, None, 1, C.byref(sp), 0, None, buf, buf, 0, 0, buf, buf, buf, None) == -1
    assert "null index" in last_error()
    assert L.phnsw_search_batch_labelset_device(None, None, None, 0, buf, 1, C.byref(sp), 0, None, buf, buf, 1, 0, buf, buf, buf,
                                                None, buf, None) == -1
    assert "null index" in last_error()
    assert L.phnsw_search_labelset_auto(None, None, buf, None, 1, C.byref(sp), None, buf, buf, 3, 0, buf, buf, buf, None) == -1
    assert "null index" in last_error()
    assert L.phnsw_search_labelset_auto_device(None, None, None, 0, buf, 1, C.byref(sp), None, buf, buf, 1, 3, 0, buf, buf, buf,
                                               None, buf, None) == -1
    assert "null index" in last_error()
    # ... and before nq == 0 is taken as a no-op
    assert L.phnsw_search_batch_labelset(None, None, None, None, 0, C.byref(sp), 0, None, None, None, 0, 0, None, None, None,
                                         None) == -1
    assert L.phnsw_search_labelset_auto(None, None, None, None, 0, C.byref(sp), None, None, None, 3, 0, None, None, None, None) == -1


def test_python_argument_handling_runs_before_the_call():
    ix = fake_index()
    lb = fake_labels(ix)
    q = np.zeros((3, 4), dtype=np.float32)
    want = [[5, 6], [], [-1, 0xFFFFFFFE, 5, 5]]
    sp = ph.SearchParameters(16, 16, 2)
    for call in (ix.search_batch_labelset, ix.search_labelset):
        with pytest.raises(ValueError, match="exactly one"):
            call(sp=sp, labels=lb, want=want)
        with pytest.raises(ValueError, match="exactly one"):
            call(queries=q, qids=np.arange(3), sp=sp, labels=lb, want=want)
        with pytest.raises(TypeError, match="labels"):  # none, and a label column where a handle belongs
            call(queries=q, sp=sp, want=want)
        with pytest.raises(TypeError, match="labels"):
            call(queries=q, sp=sp, labels=np.zeros(N, dtype=np.uint32), want=want)
        with pytest.raises(ValueError, match="want"):  # none
            call(queries=q, sp=sp, labels=lb)
        with pytest.raises(ValueError, match="want"):  # the wrong number of sets
            call(queries=q, sp=sp, labels=lb, want=[[1], [2]])
        with pytest.raises(ValueError, match="want"):  # a set that is no sequence of labels
            call(queries=q, sp=sp, labels=lb, want=[[1], [[2, 3]], [4]])
        with pytest.raises(ValueError, match="want"):  # below -1
            call(queries=q, sp=sp, labels=lb, want=[[1], [2], [-2]])
        with pytest.raises(ValueError, match="want"):  # past u32
            call(queries=q, sp=sp, labels=lb, want=[[1], [2], [1 << 32]])
        with pytest.raises(TypeError, match="want"):  # labels that are no integers
            call(queries=q, sp=sp, labels=lb, want=[[1], [2.0], [3]])
        # a ready (first, values) pair: the wrong length, offsets that do not start at 0, offsets that run backwards
        v = np.array([1, 2, 3], dtype=np.int64)
        with pytest.raises(ValueError, match="want"):
            call(queries=q, sp=sp, labels=lb, want=(np.array([0, 1, 3]), v))
        with pytest.raises(ValueError, match="query 0"):
            call(queries=q, sp=sp, labels=lb, want=(np.array([1, 1, 2, 3]), v))
        with pytest.raises(ValueError, match="query 1"):
            call(queries=q, sp=sp, labels=lb, want=(np.array([0, 2, 1, 3]), v))
        with pytest.raises(TypeError, match="want"):
            call(queries=q, sp=sp, labels=lb, want=(np.array([0.0, 1.0, 2.0, 3.0]), v))
        with pytest.raises(ValueError, match="queries"):  # rows of another length than the store's
            call(queries=np.zeros((3, 5), dtype=np.float32), sp=sp, labels=lb, want=want)
        # well-formed arguments reach the library, which refuses the null index
        with pytest.raises(ph.PhnswError) as e:
            call(queries=q, sp=sp, labels=lb, want=want)
        assert e.value.code == -1 and "null index" in str(e.value)
    with pytest.raises(TypeError, match="labels"):
        ix.search_batch_labelset_device(np.zeros(N, dtype=np.uint32), 3, 4, sp, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)
    with pytest.raises(TypeError, match="labels"):
        ix.search_labelset_device(np.zeros(N, dtype=np.uint32), 3, 4, sp, 5, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)
    with pytest.raises(ph.PhnswError) as e:
        ix.search_batch_labelset_device(lb, 3, 4, sp, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)
    assert e.value.code == -1
    with pytest.raises(ph.PhnswError) as e:
        ix.search_labelset_device(lb, 3, 4, sp, 5, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)
    assert e.value.code == -1
