"""What the label calls (phnsw_labels_*, phnsw_search_exact_labeled[_device]) answer without a GPU, and the argument
handling of Labels / Hnsw.search_exact_labeled that runs before any device call.  No index can exist without a device,
so the first check of the header's order -- a null index -- is the one every entry point reaches here: PHNSW_E_INVALID
with a message that names the call, never a crash and never a quiet success."""
import ctypes as C

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd import _lib
from parallel_hnsw_amd.hnsw import Hnsw, Labels, pack_labels

import labeled_reference as lr

N = 70


def last_error():
    return ph.lib().phnsw_last_error().decode()


def test_the_entry_points_are_bound_with_the_header_s_arity():
    arity = {"phnsw_labels_create": 4, "phnsw_labels_create_device": 5, "phnsw_labels_info": 5, "phnsw_labels_count_device": 5,
             "phnsw_labels_destroy": 1, "phnsw_search_exact_labeled": 11, "phnsw_search_exact_labeled_device": 14}
    for name, n in arity.items():
        assert len(_lib.SYMBOLS[name][1]) == n, name
        assert hasattr(ph.lib(), name)
    # the scan's arguments: a handle and `want` in place of a bitmap and its stride
    assert len(_lib.SYMBOLS["phnsw_search_exact_filtered"][1]) == 11
    assert len(_lib.SYMBOLS["phnsw_search_exact_filtered_device"][1]) == 14
    assert ph.LABEL_NONE == lr.LABEL_NONE == 0xFFFFFFFF


def test_a_null_index_is_refused_first_by_every_form():
    L = ph.lib()
    buf = (C.c_uint64 * 8)()
    out = C.c_void_p()
    for k in (10, 0, 1025):  # the index is looked at before k, and before the handle
        assert L.phnsw_search_exact_labeled(None, None, buf, None, 1, None, buf, k, buf, buf, buf) == -1
        assert last_error() == "phnsw_search_exact_labeled: null index or index without layers"
        assert L.phnsw_search_exact_labeled_device(None, None, None, 0, buf, 1, None, buf, k, buf, buf, buf, buf, None) == -1
        assert last_error() == "phnsw_search_exact_labeled_device: null index or index without layers"
    # ... and before nq == 0 is taken as a no-op
    assert L.phnsw_search_exact_labeled(None, None, None, None, 0, None, None, 10, None, None, None) == -1
    assert L.phnsw_search_exact_labeled_device(None, None, None, 0, None, 0, None, None, 10, None, None, None, None, None) == -1
    assert L.phnsw_labels_create(None, buf, 2, C.byref(out)) == -1
    assert last_error() == "phnsw_labels_create: null index or index without layers" and not out.value
    assert L.phnsw_labels_create_device(None, buf, 2, None, C.byref(out)) == -1
    assert last_error() == "phnsw_labels_create_device: null index or index without layers" and not out.value


def test_a_null_handle():
    L = ph.lib()
    L.phnsw_labels_destroy(None)  # a no-op
    v = C.c_uint64()
    assert L.phnsw_labels_info(None, C.byref(v), None, None, None) == -1
    assert last_error() == "phnsw_labels_info: null labels"
    assert L.phnsw_labels_count_device(None, None, 0, None, None) == -1
    assert last_error() == "phnsw_labels_count_device: null labels"


class FakeStore:
    n, dim = N, 4


def fake_index():
    """an Hnsw whose library handle is null: what the Python layer does before the call, and that the call then fails"""
    ix = Hnsw.__new__(Hnsw)
    ix._h = None
    ix.store = FakeStore()
    return ix


def fake_labels(ix):
    lb = Labels.__new__(Labels)
    lb._h, lb.hnsw = None, ix
    return lb


def test_python_argument_handling_runs_before_the_call():
    ix = fake_index()
    lb = fake_labels(ix)
    q = np.zeros((3, 4), dtype=np.float32)
    want = np.array([5, -1, 0xFFFFFFFE])
    with pytest.raises(ValueError, match="exactly one"):
        ix.search_exact_labeled(labels=lb, want=want)
    with pytest.raises(ValueError, match="exactly one"):
        ix.search_exact_labeled(queries=q, qids=np.arange(3), labels=lb, want=want)
    with pytest.raises(TypeError, match="labels"):  # none, and a label column where a handle belongs
        ix.search_exact_labeled(queries=q, want=want)
    with pytest.raises(TypeError, match="labels"):
        ix.search_exact_labeled(queries=q, labels=np.zeros(N, dtype=np.uint32), want=want)
    with pytest.raises(TypeError, match="labels"):
        ix.search_exact_labeled_device(np.zeros(N, dtype=np.uint32), 3, 5, 8, 8, 8, 8, qids=8, want=8)
    with pytest.raises(ValueError, match="want"):  # none
        ix.search_exact_labeled(queries=q, labels=lb)
    with pytest.raises(ValueError, match="want"):  # the wrong length
        ix.search_exact_labeled(queries=q, labels=lb, want=np.array([1, 2]))
    with pytest.raises(ValueError, match="want"):  # below -1
        ix.search_exact_labeled(queries=q, labels=lb, want=np.array([1, 2, -2]))
    with pytest.raises(ValueError, match="want"):  # past u32
        ix.search_exact_labeled(queries=q, labels=lb, want=np.array([1, 2, 1 << 32]))
    with pytest.raises(TypeError, match="want"):
        ix.search_exact_labeled(queries=q, labels=lb, want=np.array([0.0, 1.0, 1.0]))
    # well-formed arguments reach the library, which refuses the null index by name
    with pytest.raises(ph.PhnswError) as e:
        ix.search_exact_labeled(queries=q, labels=lb, want=want, k=5)
    assert e.value.code == -1 and "phnsw_search_exact_labeled:" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:
        ix.search_exact_labeled_device(lb, 3, 5, 8, 8, 8, 8, qids=8, want=8)
    assert e.value.code == -1 and "phnsw_search_exact_labeled_device:" in str(e.value)
    # the same for the handle's constructors
    with pytest.raises(TypeError, match="Hnsw"):
        Labels(object(), np.zeros(N, dtype=np.uint32))
    with pytest.raises(ValueError, match="labels"):
        Labels(ix, np.zeros(N - 1, dtype=np.uint32))
    with pytest.raises(TypeError, match="labels"):
        Labels(ix, np.zeros(N))
    with pytest.raises(ValueError, match="labels"):
        Labels(ix, np.full(N, -2))
    with pytest.raises(ph.PhnswError) as e:
        Labels(ix, np.zeros(N, dtype=np.int64))
    assert e.value.code == -1 and "phnsw_labels_create:" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:
        Labels.from_device(ix, 8)
    assert e.value.code == -1 and "phnsw_labels_create_device:" in str(e.value)


def test_labels_pack_as_the_header_wants_them():
    np.testing.assert_array_equal(pack_labels(np.array([0, -1, 3, ph.LABEL_NONE, 0x7FFFFFFF]), 5, "want"),
                                  np.array([0, 0xFFFFFFFF, 3, 0xFFFFFFFF, 0x7FFFFFFF], dtype=np.uint32))
    assert pack_labels(np.array([2], dtype=np.uint32), 1, "want").dtype == np.uint32
    np.testing.assert_array_equal(pack_labels(np.array([0xFFFFFFFE], dtype=np.uint64), 1, "want"), [0xFFFFFFFE])


def test_the_reference_s_masks():
    labels = np.array([5, 5, -1, 9, 0xFFFFFFFF, 0xFFFFFFFE, 9])
    m = lr.masks_of(labels, np.array([5, 9, -1, 0xFFFFFFFF, 0xFFFFFFFE, 77]))
    assert m.shape == (6, 7)
    assert m.astype(int).tolist() == [[1, 1, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 1], [0] * 7, [0] * 7, [0, 0, 0, 0, 0, 1, 0], [0] * 7]
