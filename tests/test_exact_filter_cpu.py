"""CPU checks of tests/exact_filter_reference.py, the yardstick of the exact scan over an allow-list
(phnsw_search_exact_filtered): hand-written cases first, then the oracle's toy index, where a graph search with
number_of_candidates >= n and the exact top-k must agree on every id both return."""
import numpy as np

import oracle

import exact_filter_reference as xr
import filter_reference as fr
from helpers import toy_vectors
from test_oracle_golden import fixture_hnsw
from value_families import bits

E, M = xr.EMPTY, xr.FMAX


def test_hand_written_cases():
    #            id:  0    1    2    3    4    5
    D = np.array([[0.5, 0.2, 0.5, 0.1, 0.2, 0.9],
                  [0.3, 0.3, 0.3, 0.3, 0.3, 0.3]], dtype=np.float32)
    ids, d, ln = xr.exact_topk(D, k=4)
    assert ids.tolist() == [[3, 1, 4, 0], [0, 1, 2, 3]]  # ties in id order
    assert bits(d).tolist() == bits(np.array([[0.1, 0.2, 0.2, 0.5], [0.3] * 4], dtype=np.float32)).tolist()
    assert ln.tolist() == [4, 4]
    # a shared bitmap; fewer candidates than k: padding
    allow = np.array([0, 1, 0, 0, 1, 1], dtype=bool)
    ids, d, ln = xr.exact_topk(D, allow=allow, k=4)
    assert ids.tolist() == [[1, 4, 5, E], [1, 4, 5, E]] and ln.tolist() == [3, 3]
    assert bits(d[:, 3]).tolist() == [int(bits(M)[0])] * 2
    # per-query bitmaps, exclude (an allowed id for query 0, a disallowed one for query 1), members
    allow2 = np.array([[1, 1, 1, 1, 0, 0], [0, 0, 1, 1, 1, 1]], dtype=bool)
    ids, d, ln = xr.exact_topk(D, allow=allow2, exclude=np.array([3, 0], dtype=np.uint64), k=3)
    assert ids.tolist() == [[1, 0, 2], [2, 3, 4]] and ln.tolist() == [3, 3]
    ids, d, ln = xr.exact_topk(D, allow=allow2, members=np.array([1, 0, 1, 0, 1, 0], dtype=bool), k=3)
    assert ids.tolist() == [[0, 2, E], [2, 4, E]] and ln.tolist() == [2, 2]
    # nothing allowed; an exclude that is EMPTY (None in the reference) changes nothing
    ids, d, ln = xr.exact_topk(D, allow=np.zeros(6, dtype=bool), k=2)
    assert ids.tolist() == [[E, E]] * 2 and ln.tolist() == [0, 0] and (bits(d) == bits(M)).all()
    a = xr.exact_topk(D, exclude=np.array([E, E], dtype=np.uint64), k=6)
    b = xr.exact_topk(D, k=6)
    assert all((x == y).all() for x, y in zip(a, b))
    # k = 1
    assert xr.exact_topk(D, k=1)[0].tolist() == [[3], [0]]


def test_agrees_with_the_strict_graph_search_on_the_toy_index():
    n = 9
    data = toy_vectors()
    rng = np.random.default_rng(3)
    q = np.ascontiguousarray(data[[0, 4, 8]] * np.float32(0.75) + rng.random((3, data.shape[1]), dtype=np.float32) * np.float32(0.25))
    for entry in (0, 3):
        ix = fixture_hnsw(entry, oracle.SUM_BLOCKED64)
        D = fr.distance_rows(ix, queries=q, mode=oracle.SUM_BLOCKED64)
        for allow in (np.ones(n, dtype=bool), np.arange(n) % 2 == 0, np.arange(n) >= 6,
                      rng.random((3, n)) < 0.5):
            graph = fr.strict(fr.search(ix, D, (16, 16, 2), allow=allow), allow)
            ids, d, ln = xr.exact_topk(D, allow=allow, k=n)
            for i in range(3):
                g = [int(v) for v in graph[0][i, :int(graph[2][i])]]
                x = [int(v) for v in ids[i, :int(ln[i])]]
                assert set(g) <= set(x)  # the scan returns EVERY candidate (k >= their number), the walk a part
                assert [v for v in x if v in g] == g  # ... in the same (distance, id) order
                for j, v in enumerate(g):
                    assert bits(graph[1][i, j]) == bits(d[i, x.index(v)])
                a = allow if allow.ndim == 1 else allow[i]
                assert x == sorted(np.nonzero(a)[0].tolist(), key=lambda v: (float(D[i, v]), v))
