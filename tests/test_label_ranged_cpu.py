"""The parts of the searches by a row label and a numeric range that need no GPU: the bitmaps the yardstick makes, the
key maps through LabeledAttribute.bounds, the wanted labels, the argument checks of LabeledAttribute and of the calls,
and what the new entry points answer where there is no device and no index."""
import ctypes as C

import numpy as np
import pytest

import parallel_hnsw_amd as ph

import label_ranged_reference as lr
import ranged_reference as rr

NONE = 0xFFFFFFFF


def test_masks_of_on_hand_written_cases():
    labels = np.array([1, 1, 2, 2, NONE, 1, 0x80000000, 0xFFFFFFFE], dtype=np.uint32)
    keys = np.array([5, 9, 5, NONE, 5, 0xFFFFFFFE, 0, 7], dtype=np.uint32)
    want = np.array([1, 2, 1, NONE, 0x80000000, 0xFFFFFFFE, 3, 1], dtype=np.uint32)
    lo = np.array([5, 0, 9, 0, 0, 7, 0, 0], dtype=np.uint32)
    hi = np.array([5, NONE, 5, NONE, 0, NONE, NONE, NONE], dtype=np.uint32)
    m = lr.masks_of(labels, keys, want, lo, hi)
    assert m.shape == (8, 8) and m.dtype == np.bool_
    assert [np.flatnonzero(r).tolist() for r in m] == [[0], [2], [], [], [6], [7], [], [0, 1, 5]]
    members = np.array([0, 1, 1, 1, 1, 1, 0, 1], dtype=bool)
    m = lr.masks_of(labels, keys, want, lo, hi, members)
    assert [np.flatnonzero(r).tolist() for r in m] == [[], [2], [], [], [], [7], [], [1, 5]]


class FakeLabeledAttr(ph.LabeledAttribute):
    """a LabeledAttribute without a handle: bounds(), key() and wanted() look at the dtype alone"""

    def __init__(self, dtype):
        self._h, self.dtype = None, np.dtype(dtype)


def test_bounds_go_through_the_key_maps_of_the_columns_dtype():
    at = FakeLabeledAttr(np.float32)
    lo, hi = at.bounds("call", -1.5, None, 3)
    np.testing.assert_array_equal(lo, rr.keys_of(np.full(3, -1.5, dtype=np.float32)))
    assert hi.tolist() == [NONE] * 3 and lo.dtype == hi.dtype == np.uint32
    lo, hi = at.bounds("call", None, np.array([0.0, -0.0, 2.0], dtype=np.float32), 3)
    assert lo.tolist() == [0, 0, 0] and hi[0] == hi[1] == 0x80000000
    ai = FakeLabeledAttr(np.int32)
    lo, hi = ai.bounds("call", np.array([-5, 7]), 2 ** 31 - 1, 2)
    np.testing.assert_array_equal(lo, rr.keys_of(np.array([-5, 7], dtype=np.int32)))
    assert hi.tolist() == [NONE] * 2
    assert ai.key(-1) == 0x7FFFFFFF and FakeLabeledAttr(np.uint32).key(9) == 9
    with pytest.raises(ValueError, match="search_label_ranged: hi: query 1: NaN"):
        at.bounds("search_label_ranged", None, np.array([0.0, np.nan, np.nan], dtype=np.float32), 3)
    with pytest.raises(TypeError, match="search_batch_label_ranged: lo: bounds in the column's dtype float32"):
        at.bounds("search_batch_label_ranged", np.array([1, 2, 3]), None, 3)
    with pytest.raises(ValueError, match=r"search_exact_label_ranged: lo: .*shape \[3\]"):
        at.bounds("search_exact_label_ranged", np.zeros(2, dtype=np.float32), None, 3)


def test_wanted_labels_broadcast_and_are_refused_naming_the_call_and_the_query():
    at = FakeLabeledAttr(np.uint32)
    w = at.wanted("call", 7, 3)
    assert w.tolist() == [7, 7, 7] and w.dtype == np.uint32
    assert at.wanted("call", np.array([0, -1, 0xFFFFFFFE]), 3).tolist() == [0, NONE, 0xFFFFFFFE]
    assert at.wanted("call", np.array([0x80000000, NONE], dtype=np.uint32), 2).tolist() == [0x80000000, NONE]
    assert at.wanted("call", -1, 2).tolist() == [NONE, NONE]
    with pytest.raises(ValueError, match="search_exact_label_ranged: want: query 2: .* is not a 32-bit label"):
        at.wanted("search_exact_label_ranged", np.array([1, 2, 2 ** 32, -7]), 4)
    with pytest.raises(ValueError, match="search_label_ranged: want: query 0: .* is not a 32-bit label"):
        at.wanted("search_label_ranged", np.array([-2, 1]), 2)
    with pytest.raises(ValueError, match=r"search_batch_label_ranged: want: .*shape \[3\]"):
        at.wanted("search_batch_label_ranged", np.array([1, 2]), 3)
    with pytest.raises(TypeError, match="call: want: an integer array, got float64"):
        at.wanted("call", np.array([1.0, 2.0]), 2)
    with pytest.raises(ValueError, match="call: want: a label or an integer array"):
        at.wanted("call", None, 2)


def test_labeled_attribute_and_the_calls_check_their_arguments_before_the_library():
    with pytest.raises(TypeError, match="LabeledAttribute: hnsw must be an Hnsw"):
        ph.LabeledAttribute(object(), np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint32))
    with pytest.raises(TypeError, match="LabeledAttribute.from_device: hnsw must be an Hnsw"):
        ph.LabeledAttribute.from_device(object(), 8, 8)
    hix = object.__new__(ph.Hnsw)
    plain = object.__new__(ph.Attribute)  # the handle of the range calls is not the handle of these
    plain._h, plain.dtype = None, np.dtype(np.uint32)
    for name in ("search_exact_label_ranged", "search_batch_label_ranged", "search_label_ranged"):
        for attr in (None, plain):
            with pytest.raises(TypeError, match="%s: attr must be a LabeledAttribute" % name):
                getattr(hix, name)(queries=np.zeros((1, 4), dtype=np.float32), attr=attr, want=1, lo=0, hi=1)
        with pytest.raises(ValueError, match="%s: pass queries or qids" % name):
            getattr(hix, name)(attr=FakeLabeledAttr(np.uint32), want=1, lo=0, hi=1)
        with pytest.raises(ValueError, match="%s: want: query 1" % name):
            getattr(hix, name)(qids=np.arange(3), attr=FakeLabeledAttr(np.uint32), want=np.array([0, 2 ** 33, 1]), lo=0, hi=1)
        with pytest.raises(TypeError, match="%s_device: attr must be a LabeledAttribute" % name):
            getattr(hix, name + "_device")(plain, 1, *([8] * 6))
    assert not isinstance(FakeLabeledAttr(np.uint32), ph.Attribute)


def test_without_a_device_nothing_falls_back_and_the_entry_points_name_themselves():
    """Where no GPU is visible the store a handle needs answers PHNSW_E_NO_DEVICE (-2): there is no CPU path to a
    LabeledAttribute.  With or without one, every new entry point refuses a null index or handle with PHNSW_E_INVALID
    and its own name before it touches a device."""
    lib = ph.lib()
    if lib.phnsw_device_count() == 0:
        with pytest.raises(ph.PhnswError) as e:
            ph.VectorStore(np.zeros((4, 8), dtype=np.float32))
        assert e.value.code == -2  # PHNSW_E_NO_DEVICE
    out = C.c_void_p()
    sp = ph.SearchParams()
    assert lib.phnsw_label_attr_create(None, None, None, 0, C.byref(out)) == -1 and not out.value
    assert lib.phnsw_last_error().decode().startswith("phnsw_label_attr_create: null index")
    assert lib.phnsw_label_attr_create_device(None, None, None, 0, None, C.byref(out)) == -1
    assert lib.phnsw_last_error().decode().startswith("phnsw_label_attr_create_device: null index")
    assert lib.phnsw_label_attr_info(None, None, None, None, None) == -1
    assert lib.phnsw_label_attr_count_device(None, None, None, None, 1, None, None) == -1
    assert lib.phnsw_last_error().decode().startswith("phnsw_label_attr_count_device: null label and attribute keys")
    lib.phnsw_label_attr_destroy(None)  # a no-op
    assert lib.phnsw_search_exact_label_ranged(None, None, None, None, 1, None, None, None, None, 3, None, None, None) == -1
    assert lib.phnsw_last_error().decode().startswith("phnsw_search_exact_label_ranged: null index")
    assert lib.phnsw_search_exact_label_ranged_device(None, None, None, 0, None, 1, None, None, None, None, 3, None, None, None,
                                                      None, None) == -1
    assert lib.phnsw_last_error().decode().startswith("phnsw_search_exact_label_ranged_device: null index")
    assert lib.phnsw_search_batch_label_ranged(None, None, None, None, 1, C.byref(sp), 0, None, None, None, None, 0, 0, None, None,
                                               None, None) == -1
    assert lib.phnsw_search_batch_label_ranged_device(None, None, None, 0, None, 1, C.byref(sp), 0, None, None, None, None, 0, None,
                                                      None, None, None, None, None) == -1
    assert lib.phnsw_search_label_ranged_auto(None, None, None, None, 1, C.byref(sp), None, None, None, None, 3, 0, None, None, None,
                                              None) == -1
    assert lib.phnsw_search_label_ranged_auto_device(None, None, None, 0, None, 1, C.byref(sp), None, None, None, None, 3, 0, None,
                                                     None, None, None, None, None) == -1
