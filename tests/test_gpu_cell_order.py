"""The stable counting sort behind the table order of a launch and the anchors' means (group.hip): its output is
the stable argsort of the keys, whatever the run."""
import ctypes as C

import numpy as np
import pytest

from parallel_hnsw_amd._lib import check, lib

pytestmark = pytest.mark.gpu

BINS = 4096


def cell_order(keys, bins=BINS):
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    out = np.empty(len(keys), dtype=np.uint32)
    f = lib().phnsw_debug_cell_order
    f.restype = C.c_int
    check(f(keys.ctypes.data_as(C.c_void_p), C.c_uint32(len(keys)), C.c_uint32(bins), out.ctypes.data_as(C.c_void_p)))
    return out


def check_order(keys, order):
    n = len(keys)
    assert sorted(order.tolist()) == list(range(n)), "not a permutation of the queries"
    along = keys[order]
    assert (along[1:] >= along[:-1]).all(), "keys decrease along the order"
    same = along[1:] == along[:-1]
    assert (order[1:][same] > order[:-1][same]).all(), "equal keys out of query order"
    np.testing.assert_array_equal(order, np.argsort(keys, kind="stable").astype(np.uint32))


@pytest.mark.parametrize("n", [2048, 2049, 4095])
@pytest.mark.parametrize("spread", ["clustered", "uniform", "equal"])
def test_order_is_the_stable_argsort(n, spread):
    rng = np.random.default_rng(n)
    if spread == "clustered":  # about ten queries per key, as a batch over clustered data has them
        keys = rng.choice(rng.integers(0, BINS, n // 10), n).astype(np.uint32)
    elif spread == "uniform":
        keys = rng.integers(0, BINS, n).astype(np.uint32)
    else:
        keys = np.full(n, 1234, dtype=np.uint32)
    a = cell_order(keys)
    check_order(keys, a)
    np.testing.assert_array_equal(a, cell_order(keys))  # two runs, one output


def test_first_and_last_cell_and_few_bins():
    keys = np.array([BINS - 1, 0, BINS - 1, 0, 7] * 500, dtype=np.uint32)
    check_order(keys, cell_order(keys))
    rng = np.random.default_rng(3)
    for bins in (1, 2, 1500):  # fewer cells than the prefix kernel has threads, and a count that divides nothing
        k = rng.integers(0, bins, 3000).astype(np.uint32)
        check_order(k, cell_order(k, bins))
