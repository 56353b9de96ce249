"""The subset form of the scan by label sets (the scan covers the queries of a list; which query owns a pair is still
decided over the whole batch), reached through the routed call: phnsw_search_labelset_auto_device with scan_below =
ALWAYS_SCAN puts every query on the scan list.  On a batch where some Stored ids are bad and some ranges overlap, every
status and every row must equal phnsw_search_exact_labelset_device's for the same arrays -- ids, distance bits, lengths,
statuses, no tolerance."""
import numpy as np
import pytest

import parallel_hnsw_amd as ph

import filter_auto_reference as ar
from test_gpu_exact_labelset import staged_labelset
from test_gpu_exact_shared import fetch
from test_gpu_filter_auto import EMPTY, K, N, NQ, SP, same, world
from test_gpu_i8q import env
from test_gpu_labelset_auto import device_sauto, edge_world, spread

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("knobs", [dict(), dict(PHNSW_LABEL_TILE="1", PHNSW_LABEL_SLICES="3")])
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("pq", 24)])
def test_the_subset_scan_equals_the_whole_scan_on_bad_ids_and_overlapping_ranges(monkeypatch, kind, dim, knobs):
    import torch
    w = world(kind, dim)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    lab, sets, _ = edge_world(w)
    lb = ph.Labels(hix, lab)
    want = spread(sets)
    first, values = ph.hnsw.pack_label_sets(want, NQ)
    # ranges: query 38 runs backwards, query 39 starts inside the range of the lower query 19 (which keeps its pairs), the
    # last query ends past nwant; Stored ids: 5 and 39 (bad twice: 8 wins) are past n
    f = first.astype(np.int64).copy()
    f[39] = first[19] + 2
    f[NQ] = len(values) + 3
    assert f[38] > f[39] and first[19] < f[39] < first[20]
    qids = w["qids"].copy()
    qids[[5, 39]] = [N + 1, 0xFFFFFFFE]
    ex = (w["qids"] * 3 + 1) % N
    with env(monkeypatch, **knobs):
        launch, out = staged_labelset(hix, lb, K, f.astype(np.uint32), values, qids=qids, exclude=ex.astype(np.uint32))
        torch.cuda.synchronize()
        launch()
        exact = fetch(out)
        got = device_sauto(hix, lb, spp, K, qids=qids, want=want, exclude=ex, scan_below=ar.ALWAYS_SCAN, first=f.astype(np.uint32))
    assert sorted(np.nonzero(exact[3] == 8)[0].tolist()) == [38, 39, NQ - 1] and exact[3][5] == 4
    assert set(exact[3].tolist()) == {0, 4, 8} and (exact[2] > 0).any()
    np.testing.assert_array_equal(got[4], exact[3])
    same(got, exact)
    assert (got[3] == ar.SCAN).all()
    assert (got[0][exact[3] != 0] == EMPTY).all() and not got[2][exact[3] != 0].any()


def test_a_scan_list_of_a_few_queries_leaves_the_other_rows_to_the_walk():
    """scan_below = 100 on the edge sets: the scan list holds the routed queries only, the graph rows are written by the
    walk -- and every scanned row is still the whole-batch scan's row"""
    w = world("f32", 24)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    lab, sets, _ = edge_world(w)
    lb = ph.Labels(hix, lab)
    want = spread(sets)
    got = hix.search_labelset(queries=w["q"], sp=spp, labels=lb, want=want, k=K, scan_below=100, route=True)
    scanned = got[3] != ar.GRAPH
    assert scanned.any() and not scanned.all()
    whole = hix.search_exact_labelset(queries=w["q"], labels=lb, want=want, k=K)
    same([x[scanned] for x in got[:3]], [x[scanned] for x in whole])
