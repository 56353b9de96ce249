"""The calls by row label that walk the graph (phnsw_search_batch_labeled, phnsw_search_labeled_auto and their device
forms) without a GPU: the composition restated from the label column against filter_auto_reference.compose over
labeled_reference.masks_of on a toy case, the bindings' arity, what the library answers to a null index, and the
argument handling of the Python wrappers, which runs before any library call."""
import ctypes as C

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd import _lib

import exact_filter_reference as xr
import filter_auto_reference as ar
import labeled_auto_reference as lar
import labeled_reference as lr
from test_exact_labeled_cpu import N, fake_index, fake_labels, last_error


def toy(seed, n=60, nq=24, ef=8, k=3):
    """a column, wanted labels, excludes, and made-up strict rows and exact rows that respect the masks"""
    rng = np.random.default_rng(seed)
    members = np.arange(n) % 5 != 4
    labels = rng.choice([1, 2, 3, 9, -1, 0xFFFFFFFE], size=n, p=[0.5, 0.2, 0.05, 0.1, 0.1, 0.05])
    want = rng.choice([1, 2, 3, 9, -1, 0xFFFFFFFE, 77], size=nq)
    exclude = rng.integers(0, n + 5, nq).astype(np.uint64)
    masks = lr.masks_of(labels, want) & members[None, :]
    D = rng.random((nq, n)).astype(np.float32)
    scan = xr.exact_topk(D, lr.masks_of(labels, want), exclude, members, k)
    walk_ids = np.full((nq, ef), xr.EMPTY, dtype=np.uint64)
    walk_d = np.full((nq, ef), xr.FMAX, dtype=np.float32)
    walk_len = np.zeros(nq, dtype=np.uint64)
    for q in range(nq):  # a strict row: some of the candidates, ascending; sometimes too few of them
        cand = np.nonzero(masks[q])[0]
        take = cand[rng.random(len(cand)) < (0.3 if q % 2 else 0.9)]
        take = take[np.lexsort((take, D[q, take]))][:ef]
        walk_ids[q, :len(take)], walk_d[q, :len(take)], walk_len[q] = take, D[q, take], len(take)
    return labels, want, exclude, members, (walk_ids, walk_d, walk_len), scan, ef, k


@pytest.mark.parametrize("scan_below", [1, 4, 12])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_composition_from_the_column_is_the_composition_over_the_masks(seed, scan_below):
    labels, want, exclude, members, walk, scan, ef, k = toy(seed)
    n_nodes = int(members.sum())
    for ex in (None, exclude):
        got = lar.compose(walk, scan, labels, want, ef, k, n_nodes, ex, members, scan_below)
        ref = ar.compose(walk, scan, len(labels), ef, k, n_nodes, lr.masks_of(labels, want), ex, members, scan_below)
        for a, b in zip(got, ref):
            np.testing.assert_array_equal(a, b)
        assert len(set(got[3].tolist())) >= 2
    np.testing.assert_array_equal(lar.counts_of(labels, want, members),
                                  (lr.masks_of(labels, want) & members[None, :]).sum(axis=1))
    assert lar.SCAN_BELOW_LABELED == 20000  # filter_route.h, PH_AUTO_SCAN_BELOW_LABELED


def test_the_entry_points_are_bound_with_the_header_s_arity():
    arity = {"phnsw_search_batch_labeled": 15, "phnsw_search_batch_labeled_device": 17, "phnsw_search_labeled_auto": 14,
             "phnsw_search_labeled_auto_device": 17}
    for name, n in arity.items():
        assert len(_lib.SYMBOLS[name][1]) == n, name
        assert hasattr(ph.lib(), name)
    # (lb, want) in place of (filter, stride): the same number of arguments as the bitmap calls
    for a, b in (("phnsw_search_batch_labeled", "phnsw_search_batch_filtered"),
                 ("phnsw_search_batch_labeled_device", "phnsw_search_batch_filtered_device"),
                 ("phnsw_search_labeled_auto", "phnsw_search_filtered_auto"),
                 ("phnsw_search_labeled_auto_device", "phnsw_search_filtered_auto_device")):
        assert len(_lib.SYMBOLS[a][1]) == len(_lib.SYMBOLS[b][1])


def test_a_null_index_is_refused_first_by_every_form():
    L = ph.lib()
    buf = (C.c_uint64 * 8)()
    sp = ph.SearchParameters(16, 16, 2)
    assert L.phnsw_search_batch_labeled(None, None, buf, None, 1, C.byref(sp), 0, None, buf, 0, 0, buf, buf, buf, None) == -1
    assert "null index" in last_error()
    assert L.phnsw_search_batch_labeled_device(None, None, None, 0, buf, 1, C.byref(sp), 0, None, buf, 0, buf, buf, buf, None, buf,
                                               None) == -1
    assert "null index" in last_error()
    assert L.phnsw_search_labeled_auto(None, None, buf, None, 1, C.byref(sp), None, buf, 3, 0, buf, buf, buf, None) == -1
    assert "null index" in last_error()
    assert L.phnsw_search_labeled_auto_device(None, None, None, 0, buf, 1, C.byref(sp), None, buf, 3, 0, buf, buf, buf, None, buf,
                                              None) == -1
    assert "null index" in last_error()
    # ... and before nq == 0 is taken as a no-op
    assert L.phnsw_search_batch_labeled(None, None, None, None, 0, C.byref(sp), 0, None, None, 0, 0, None, None, None, None) == -1
    assert L.phnsw_search_labeled_auto(None, None, None, None, 0, C.byref(sp), None, None, 3, 0, None, None, None, None) == -1


def test_python_argument_handling_runs_before_the_call():
    ix = fake_index()
    lb = fake_labels(ix)
    q = np.zeros((3, 4), dtype=np.float32)
    want = np.array([5, -1, 0xFFFFFFFE])
    sp = ph.SearchParameters(16, 16, 2)
    for call in (ix.search_batch_labeled, ix.search_labeled):
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
        with pytest.raises(ValueError, match="want"):  # the wrong length
            call(queries=q, sp=sp, labels=lb, want=np.array([1, 2]))
        with pytest.raises(ValueError, match="want"):  # the wrong shape
            call(queries=q, sp=sp, labels=lb, want=np.zeros((3, 1), dtype=np.int64))
        with pytest.raises(ValueError, match="want"):  # below -1
            call(queries=q, sp=sp, labels=lb, want=np.array([1, 2, -2]))
        with pytest.raises(ValueError, match="want"):  # past u32
            call(queries=q, sp=sp, labels=lb, want=np.array([1, 2, 1 << 32]))
        with pytest.raises(TypeError, match="want"):
            call(queries=q, sp=sp, labels=lb, want=np.array([0.0, 1.0, 1.0]))
        with pytest.raises(ValueError, match="queries"):  # rows of another length than the store's
            call(queries=np.zeros((3, 5), dtype=np.float32), sp=sp, labels=lb, want=want)
        # well-formed arguments reach the library, which refuses the null index
        with pytest.raises(ph.PhnswError) as e:
            call(queries=q, sp=sp, labels=lb, want=want)
        assert e.value.code == -1 and "null index" in str(e.value)
    with pytest.raises(TypeError, match="labels"):
        ix.search_batch_labeled_device(np.zeros(N, dtype=np.uint32), 3, sp, 8, 8, 8, 8, qids=8, want=8)
    with pytest.raises(TypeError, match="labels"):
        ix.search_labeled_device(np.zeros(N, dtype=np.uint32), 3, sp, 5, 8, 8, 8, 8, qids=8, want=8)
    with pytest.raises(ph.PhnswError) as e:
        ix.search_batch_labeled_device(lb, 3, sp, 8, 8, 8, 8, qids=8, want=8)
    assert e.value.code == -1
    with pytest.raises(ph.PhnswError) as e:
        ix.search_labeled_device(lb, 3, sp, 5, 8, 8, 8, 8, qids=8, want=8)
    assert e.value.code == -1
