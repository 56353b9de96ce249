"""The parts of the searches by a numeric range that need no GPU: the order-preserving key maps (hnsw.attr_keys against
ranged_reference.keys_of, which is written independently), the bitmaps the yardstick makes, and the argument checks of
Attribute and of lo / hi."""
import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd import hnsw as H

import ranged_reference as rr

F32_MAX = np.finfo(np.float32).max
DENORM = np.float32(1e-45)
F32_LADDER = np.array([-np.inf, -F32_MAX, -1.0, -DENORM, -0.0, 0.0, DENORM, 1.0, F32_MAX, np.inf], dtype=np.float32)
I32_LADDER = np.array([-2 ** 31, -2 ** 31 + 1, -65536, -1, 0, 1, 65535, 2 ** 31 - 2, 2 ** 31 - 1], dtype=np.int32)
U32_LADDER = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE], dtype=np.uint32)


@pytest.mark.parametrize("maps", [H.attr_keys, rr.keys_of], ids=["hnsw", "reference"])
def test_the_maps_are_strictly_monotone_over_a_sorted_ladder(maps):
    k = maps(F32_LADDER).astype(np.int64)
    assert k.dtype == np.int64 and maps(F32_LADDER).dtype == np.uint32
    d = np.diff(k)
    assert d[4] == 0 and (np.delete(d, 4) > 0).all()  # -0.0 and +0.0: one key; strictly ascending everywhere else
    assert k[5] == 0x80000000
    assert (np.diff(maps(I32_LADDER).astype(np.int64)) > 0).all()
    assert maps(I32_LADDER)[0] == 0 and maps(I32_LADDER)[-1] == 0xFFFFFFFF
    np.testing.assert_array_equal(maps(U32_LADDER), U32_LADDER)


def test_both_maps_agree_on_random_values():
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32)
    f = bits.view(np.float32)
    f = f[~np.isnan(f)]
    np.testing.assert_array_equal(H.attr_keys(f), rr.keys_of(f))
    order = np.argsort(f, kind="stable")
    assert (np.diff(H.attr_keys(f)[order].astype(np.int64)) >= 0).all()
    i = bits.view(np.int32)
    np.testing.assert_array_equal(H.attr_keys(i), rr.keys_of(i))
    assert (np.diff(H.attr_keys(np.sort(i)).astype(np.int64)) >= 0).all()


def test_nan_and_the_none_word_are_refused_naming_the_first_index():
    for maps in (H.attr_keys, rr.keys_of):
        with pytest.raises(ValueError, match="index 2"):
            maps(np.array([1.0, 2.0, np.nan, np.nan], dtype=np.float32))
        with pytest.raises(ValueError, match="index 1"):
            maps(np.array([5, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32))
        with pytest.raises(TypeError):
            maps(np.array([1, 2], dtype=np.int64))
        with pytest.raises(TypeError):
            maps(np.array([1.0], dtype=np.float64))


def test_masks_of_on_hand_written_cases():
    keys = np.array([5, 0, 9, rr.ATTR_NONE, 5, 0xFFFFFFFE, 7], dtype=np.uint32)
    lo = np.array([5, 0, 6, 9, 0, 8, 0xFFFFFFFF], dtype=np.uint32)
    hi = np.array([5, 4, 8, 5, 0xFFFFFFFF, 8, 0xFFFFFFFF], dtype=np.uint32)
    m = rr.masks_of(keys, lo, hi)
    assert m.shape == (7, 7) and m.dtype == np.bool_
    assert [np.flatnonzero(r).tolist() for r in m] == [[0, 4], [1], [6], [], [0, 1, 2, 4, 5, 6], [], []]
    members = np.array([1, 0, 1, 1, 0, 1, 1], dtype=bool)
    m = rr.masks_of(keys, lo, hi, members)
    assert [np.flatnonzero(r).tolist() for r in m] == [[0], [], [6], [], [0, 2, 5, 6], [], []]


class FakeAttr(ph.Attribute):
    """an Attribute without a handle: bounds() and key() look at the dtype alone"""

    def __init__(self, dtype):
        self._h, self.dtype = None, np.dtype(dtype)


def test_bounds_broadcast_scalars_open_ends_and_map_in_the_columns_dtype():
    at = FakeAttr(np.float32)
    lo, hi = at.bounds("call", -1.5, None, 3)
    np.testing.assert_array_equal(lo, rr.keys_of(np.full(3, -1.5, dtype=np.float32)))
    assert hi.tolist() == [0xFFFFFFFF] * 3 and lo.dtype == hi.dtype == np.uint32
    lo, hi = at.bounds("call", None, np.array([0.0, -0.0, 2.0], dtype=np.float32), 3)
    assert lo.tolist() == [0, 0, 0] and hi[0] == hi[1] == 0x80000000
    ai = FakeAttr(np.int32)
    lo, hi = ai.bounds("call", np.array([-5, 7]), 2 ** 31 - 1, 2)  # int64 values that are int32 values
    np.testing.assert_array_equal(lo, rr.keys_of(np.array([-5, 7], dtype=np.int32)))
    assert hi.tolist() == [0xFFFFFFFF] * 2
    assert ai.key(-1) == 0x7FFFFFFF and FakeAttr(np.uint32).key(9) == 9


def test_bounds_refuse_what_is_not_a_bound_naming_the_call_and_the_query():
    at = FakeAttr(np.float32)
    with pytest.raises(ValueError, match=r"search_exact_ranged: lo: .*shape \[3\]"):
        at.bounds("search_exact_ranged", np.zeros(2, dtype=np.float32), None, 3)
    with pytest.raises(ValueError, match="search_ranged: hi: query 1: NaN"):
        at.bounds("search_ranged", None, np.array([0.0, np.nan, np.nan], dtype=np.float32), 3)
    with pytest.raises(TypeError, match="search_batch_ranged: lo: bounds in the column's dtype float32"):
        at.bounds("search_batch_ranged", np.array([1, 2, 3]), None, 3)
    ai = FakeAttr(np.int32)
    with pytest.raises(ValueError, match="call: hi: query 2: .* is not a value of dtype int32"):
        ai.bounds("call", None, np.array([0, 1, 2 ** 31]), 3)
    with pytest.raises(TypeError):
        ai.bounds("call", 0.5, None, 3)
    au = FakeAttr(np.uint32)
    with pytest.raises(ValueError, match="call: lo: query 0: .* is not a value of dtype uint32"):
        au.bounds("call", np.array([-1, 1, 2]), None, 3)
    with pytest.raises(ValueError, match="call: hi: query 0: 0xFFFFFFFF is ATTR_NONE"):
        au.bounds("call", 3, 0xFFFFFFFF, 2)  # a u32 BOUND of 0xFFFFFFFF is refused like a value: None is the open end


def test_attribute_and_the_calls_check_their_arguments_before_the_library():
    with pytest.raises(TypeError, match="Attribute: hnsw must be an Hnsw"):
        ph.Attribute(object(), np.zeros(3, dtype=np.uint32))
    with pytest.raises(TypeError, match="Attribute.from_device: hnsw must be an Hnsw"):
        ph.Attribute.from_device(object(), 8)
    hix = object.__new__(ph.Hnsw)
    for name in ("search_exact_ranged", "search_batch_ranged", "search_ranged"):
        with pytest.raises(TypeError, match="%s: attr must be an Attribute" % name):
            getattr(hix, name)(queries=np.zeros((1, 4), dtype=np.float32), attr=None, lo=0, hi=1)
        with pytest.raises(ValueError, match="%s: pass queries or qids" % name):
            getattr(hix, name)(attr=FakeAttr(np.uint32), lo=0, hi=1)
        with pytest.raises(TypeError, match="%s_device: attr must be an Attribute" % name):
            getattr(hix, name + "_device")(None, 1, *([8] * 6))
