"""The contract of phnsw_search_filtered_auto restated without a GPU (tests/filter_auto_reference.py) and checked
against itself on the toy worlds of tests/test_filter_cpu.py: the rule's edges, the composition of the strict graph row
(tests/filter_reference.py: search + strict, exclude dropped) with the exact row (tests/exact_filter_reference.py), the
fallback, and the completeness the call promises -- which the restatement must satisfy before the GPU test leans on
it."""
import numpy as np

import oracle

import exact_filter_reference as xr
import filter_auto_reference as ar
import filter_reference as fr
from test_filter_cpu import N, NQ, built


def test_rule_edges():
    ef, k, n = 16, 10, 1500
    edge = ar.first_graph_count(ef, k, n)
    assert edge == 938 and (edge - 1) * ef < k * n <= edge * ef
    assert ar.rule(edge - 1, 100, ef, k, n) == ar.SCAN and ar.rule(edge, 100, ef, k, n) == ar.GRAPH
    assert ar.rule(100, 100, 1024, 1, n) == ar.SCAN and ar.rule(101, 100, 1024, 1, n) == ar.GRAPH
    assert ar.rule(0, 1, ef, k, n) == ar.SCAN
    assert ar.rule(n, ar.ALWAYS_SCAN, 1024, 1, n) == ar.SCAN
    # scan_below 0: the defaults, by bitmap kind
    assert ar.rule(13000, 0, 1024, 1, 10 ** 6, per_query=False) == ar.SCAN
    assert ar.rule(13001, 0, 1024, 1, 10 ** 6, per_query=False) == ar.GRAPH
    assert ar.rule(10000, 0, 1024, 1, 10 ** 6, per_query=True) == ar.SCAN
    assert ar.rule(10001, 0, 1024, 1, 10 ** 6, per_query=True) == ar.GRAPH
    # products past 2^32 (Python integers: the yardstick of the C rule's 64-bit arithmetic)
    assert ar.rule(2 ** 22, 1, 1024, 1024, 2 ** 22 + 1) == ar.SCAN and ar.rule(2 ** 22, 1, 1024, 1024, 2 ** 22) == ar.GRAPH


def routed(dim, sp, k, allow, exclude, scan_below, stored):
    ix, layers, q = built(dim)
    qids = np.arange(3, N, N // NQ, dtype=np.uint64)[:NQ]
    D = fr.distance_rows(ix, qids=qids) if stored else fr.distance_rows(ix, queries=q)
    walk = fr.strict(fr.search(ix, D, sp, allow=allow, exclude=exclude, layers=layers),
                     np.ones(N, dtype=bool) if allow is None else allow)
    scan = xr.exact_topk(D, allow, exclude, None, k)
    res = ar.compose(walk, scan, N, sp[0], k, N, allow=allow, exclude=exclude, scan_below=scan_below)
    return res, walk, scan, D


def test_composition_is_complete_and_uses_all_three_routes():
    sp, k = (16, 16, 2), 10
    rng = np.random.default_rng(11)
    edge = ar.first_graph_count(sp[0], k, N)
    counts = [0, 1, k - 1, k, 100, 101, edge - 1, edge, N] + [edge + 64] * (NQ - 9)
    for stored in (False, True):
        D = routed(6, sp, k, None, None, 100, stored)[3]
        allow = np.zeros((NQ, N), dtype=bool)
        for i, c in enumerate(counts):
            if i < 12:
                allow[i, rng.permutation(N)[:c]] = True
            else:  # the rows farthest from the query: the rule says graph, the walk can hardly fill the row
                allow[i, np.argsort(D[i], kind="stable")[N - c:]] = True
        entry = int(built(6)[1][0][0][0])
        exclude = np.array([entry if i % 2 else xr.EMPTY for i in range(NQ)], dtype=np.uint64)
        for ex in (None, exclude):
            res, walk, scan, _ = routed(6, sp, k, allow, ex, 100, stored)
            ar.assert_complete(res, N, k, allow, ex)
            want = [ar.rule(c, 100, sp[0], k, N) for c in counts]
            assert [int(r) for r in res[3][:7]] == want[:7] == [ar.SCAN] * 7
            assert all(int(r) in (ar.GRAPH, ar.GRAPH_THEN_SCAN) for r in res[3][7:])
            # the far-rows queries: the walk keeps what its upper layers happened to pass, mostly fewer than k
            short = walk[2][12:] < k
            assert short.sum() >= 3
            np.testing.assert_array_equal(res[3][12:] == ar.GRAPH_THEN_SCAN, short)
            for q in range(NQ):
                if res[3][q] != ar.GRAPH:
                    np.testing.assert_array_equal(res[0][q], scan[0][q])
                elif ex is not None:
                    assert int(ex[q]) not in res[0][q].tolist()
        res = routed(6, sp, k, allow, None, ar.ALWAYS_SCAN, stored)[0]
        assert (res[3] == ar.SCAN).all()


def test_a_dense_shared_filter_walks_the_graph_and_no_filter_is_every_vector():
    sp, k = (64, 32, 2), 10
    allow = np.random.default_rng(3).random(N) < 0.9
    entry = int(built(100)[1][0][0][0])
    exclude = np.full(NQ, entry, dtype=np.uint64)
    for a in (allow, None):
        for ex in (None, exclude):
            res, walk, _, _ = routed(100, sp, k, a, ex, 100, False)
            ar.assert_complete(res, N, k, a, ex)
            assert (res[3] == ar.GRAPH).all()
            if ex is None:
                np.testing.assert_array_equal(res[0], walk[0][:, :k])
            else:
                assert not (res[0] == np.uint64(entry)).any()
