"""The parts of the searches by a set of row labels and a numeric range that need no GPU: the bitmaps the yardstick makes
against a loop-written mask on a tiny column, the CSR staging of the sets, the key maps of the bounds, the refusals the
wrappers decide before any device call, and what the seven new entry points answer where there is no device and no
index."""
import ctypes as C

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd.hnsw import pack_label_sets

import label_ranged_reference as lr
import labelset_ranged_reference as sr
import ranged_reference as rr

NONE = 0xFFFFFFFF

LABELS = np.array([1, 1, 2, 2, NONE, 1, 0x80000000, 0xFFFFFFFE, 0x7FFFFFFF, 2], dtype=np.uint32)
KEYS = np.array([5, 9, 5, NONE, 5, 0xFFFFFFFE, 0, 7, 7, 0], dtype=np.uint32)
SETS = [[1], [1, 2], [2, 1, 1], [], [NONE], [NONE, 0x80000000], [3], [0x7FFFFFFF, 0x80000000, 0xFFFFFFFE], [1, 2], [2]]
LO = np.array([5, 0, 5, 0, 0, 0, 0, 0, 9, 1], dtype=np.uint32)
HI = np.array([5, NONE, 9, NONE, NONE, NONE, NONE, 7, 5, NONE], dtype=np.uint32)


def test_masks_of_against_a_loop_written_mask_on_a_tiny_column():
    m = sr.masks_of(LABELS, KEYS, SETS, LO, HI)
    assert m.shape == (10, 10) and m.dtype == np.bool_
    loop = np.zeros((10, 10), dtype=bool)
    for q in range(10):
        for v in range(10):
            listed = int(LABELS[v]) != NONE and int(KEYS[v]) != NONE
            wanted = any(int(x) == int(LABELS[v]) for x in SETS[q] if int(x) != NONE)
            loop[q, v] = listed and wanted and int(LO[q]) <= int(KEYS[v]) <= int(HI[q])
    np.testing.assert_array_equal(m, loop)
    assert [np.flatnonzero(r).tolist() for r in m] == [[0], [0, 1, 2, 5, 9], [0, 1, 2], [], [], [6], [], [6, 7, 8], [], [2]]
    members = np.array([0, 1, 1, 1, 1, 1, 0, 1, 1, 1], dtype=bool)
    assert [np.flatnonzero(r).tolist() for r in sr.masks_of(LABELS, KEYS, SETS, LO, HI, members)] == \
        [[], [1, 2, 5, 9], [1, 2], [], [], [], [], [7, 8], [], [2]]
    # sets of one label are the masks of the yardstick by label and range
    one = np.array([1, 2, NONE, 3, 0x80000000], dtype=np.uint32)
    np.testing.assert_array_equal(sr.masks_of(LABELS, KEYS, [[int(x)] for x in one], LO[:5], HI[:5]),
                                  lr.masks_of(LABELS, KEYS, one, LO[:5], HI[:5]))
    # the order inside a set and a label twice change nothing
    np.testing.assert_array_equal(sr.masks_of(LABELS, KEYS, [list(reversed(s)) + s for s in SETS], LO, HI), m)


class FakeLabeledAttr(ph.LabeledAttribute):
    """a LabeledAttribute without a handle: bounds() and key() look at the dtype alone"""

    def __init__(self, dtype):
        self._h, self.dtype = None, np.dtype(dtype)


def test_the_sets_are_staged_in_csr_form_and_the_bounds_go_through_the_key_map():
    hix = object.__new__(ph.Hnsw)
    at = FakeLabeledAttr(np.int32)
    q, qi, nq, first, values, lo, hi = hix._labelset_ranged_args("call", None, np.arange(4), at, [[3, -1], [], [0x80000000, 3, 3], [NONE]],
                                                                 np.array([-5, 0, 7, 1]), None)
    assert q is None and nq == 4 and qi.dtype == np.uint64
    assert first.tolist() == [0, 2, 2, 5, 6] and first.dtype == np.uint32
    assert values.tolist() == [3, NONE, 0x80000000, 3, 3, NONE] and values.dtype == np.uint32
    np.testing.assert_array_equal(lo, rr.keys_of(np.array([-5, 0, 7, 1], dtype=np.int32)))
    assert hi.tolist() == [NONE] * 4 and lo.dtype == hi.dtype == np.uint32
    # a ready (first, values) pair is taken as it is
    ready = (np.array([0, 2, 2, 5, 6], dtype=np.uint32), np.array([3, NONE, 0x80000000, 3, 3, NONE], dtype=np.uint32))
    f2, v2 = hix._labelset_ranged_args("call", None, np.arange(4), at, ready, 0, 1)[3:5]
    assert f2.tolist() == first.tolist() and v2.tolist() == values.tolist()
    f3, v3 = pack_label_sets([[], []], 2)
    assert f3.tolist() == [0, 0, 0] and len(v3) == 0
    af = FakeLabeledAttr(np.float32)
    lo, hi = hix._labelset_ranged_args("call", None, np.arange(2), af, [[1], [2]], -1.5, np.array([0.0, 2.0], dtype=np.float32))[5:]
    np.testing.assert_array_equal(lo, rr.keys_of(np.full(2, -1.5, dtype=np.float32)))
    np.testing.assert_array_equal(hi, rr.keys_of(np.array([0.0, 2.0], dtype=np.float32)))


def test_the_calls_check_their_arguments_before_the_library():
    hix = object.__new__(ph.Hnsw)
    plain = object.__new__(ph.Attribute)  # the handle of the range calls is not the handle of these
    plain._h, plain.dtype = None, np.dtype(np.uint32)
    at = FakeLabeledAttr(np.float32)
    q = np.zeros((2, 4), dtype=np.float32)
    for name in ("search_exact_labelset_ranged", "search_batch_labelset_ranged", "search_labelset_ranged"):
        call = getattr(hix, name)
        for attr in (None, plain):
            with pytest.raises(TypeError, match="%s: attr must be a LabeledAttribute" % name):
                call(queries=q, attr=attr, want=[[1], [2]], lo=0.0, hi=1.0)
        with pytest.raises(ValueError, match="%s: pass queries or qids" % name):
            call(attr=at, want=[[1], [2]], lo=0.0, hi=1.0)
        with pytest.raises(ValueError, match="%s: pass queries or qids" % name):
            call(queries=q, qids=np.arange(2), attr=at, want=[[1], [2]], lo=0.0, hi=1.0)
        with pytest.raises(ValueError, match="want: 2 sets of labels"):
            call(qids=np.arange(2), attr=at, want=[[1]], lo=0.0, hi=1.0)
        with pytest.raises(ValueError, match="want: 2 sets of labels are required"):
            call(qids=np.arange(2), attr=at, want=None, lo=0.0, hi=1.0)
        with pytest.raises(ValueError, match="want: offsets start at 0 and never run backwards \\(query 1\\)"):
            call(qids=np.arange(3), attr=at, want=(np.array([0, 2, 1, 3]), np.array([1, 2, 3], dtype=np.uint32)), lo=0.0, hi=1.0)
        with pytest.raises(TypeError, match="want: set 1: integer labels"):
            call(qids=np.arange(2), attr=at, want=[[1], [2.5]], lo=0.0, hi=1.0)
        with pytest.raises(ValueError, match="%s: hi: query 1: NaN" % name):
            call(qids=np.arange(2), attr=at, want=[[1], [2]], lo=None, hi=np.array([0.0, np.nan], dtype=np.float32))
        with pytest.raises(TypeError, match="%s: lo: bounds in the column's dtype float32" % name):
            call(qids=np.arange(2), attr=at, want=[[1], [2]], lo=np.array([1, 2]), hi=None)
        with pytest.raises(ValueError, match=r"%s: lo: .*shape \[2\]" % name):
            call(qids=np.arange(2), attr=at, want=[[1], [2]], lo=np.zeros(3, dtype=np.float32), hi=None)
        with pytest.raises(TypeError, match="%s_device: attr must be a LabeledAttribute" % name):
            getattr(hix, name + "_device")(plain, 1, 1, *([8] * 6))
    with pytest.raises(ValueError, match="search_batch_labelset_ranged: k must not be negative"):
        hix.search_batch_labelset_ranged(qids=np.arange(2), attr=at, want=[[1], [2]], lo=0.0, hi=1.0, k=-1)


def test_without_a_device_nothing_falls_back_and_the_entry_points_name_themselves():
    """Every new entry point refuses a null index or handle with PHNSW_E_INVALID and its own name before it touches a
    device: there is no CPU path behind any of them."""
    lib = ph.lib()
    sp = ph.SearchParams()
    assert lib.phnsw_label_attr_count_set_device(None, None, None, None, None, 1, 0, None, None) == -1
    assert lib.phnsw_last_error().decode().startswith("phnsw_label_attr_count_set_device: null label and attribute keys")
    assert lib.phnsw_search_exact_labelset_ranged(None, None, None, None, 1, None, None, None, None, None, 3, None, None, None) == -1
    assert lib.phnsw_last_error().decode().startswith("phnsw_search_exact_labelset_ranged: null index")
    assert lib.phnsw_search_exact_labelset_ranged_device(None, None, None, 0, None, 1, None, None, None, 0, None, None, 3, None, None,
                                                         None, None, None) == -1
    assert lib.phnsw_last_error().decode().startswith("phnsw_search_exact_labelset_ranged_device: null index")
    assert lib.phnsw_search_batch_labelset_ranged(None, None, None, None, 1, C.byref(sp), 0, None, None, None, None, None, 0, 0, None,
                                                  None, None, None) == -1
    assert lib.phnsw_search_batch_labelset_ranged_device(None, None, None, 0, None, 1, C.byref(sp), 0, None, None, None, 0, None, None, 0,
                                                         None, None, None, None, None, None) == -1
    assert lib.phnsw_search_labelset_ranged_auto(None, None, None, None, 1, C.byref(sp), None, None, None, None, None, 3, 0, None, None,
                                                 None, None) == -1
    assert lib.phnsw_search_labelset_ranged_auto_device(None, None, None, 0, None, 1, C.byref(sp), None, None, None, 0, None, None, 3, 0,
                                                        None, None, None, None, None, None) == -1
