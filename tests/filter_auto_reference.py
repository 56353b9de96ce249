"""phnsw_search_filtered_auto restated in numpy: the route rule of phnsw.h and the composition of the two established
results into the routed one.  Nothing here computes a distance or walks a graph: the strict graph rows and the exact
rows come from the caller -- tests/filter_reference.py and tests/exact_filter_reference.py on the CPU, the two existing
library calls on the GPU."""
import numpy as np

import exact_filter_reference as xr

GRAPH, SCAN, GRAPH_THEN_SCAN = 0, 1, 2
SCAN_BELOW_SHARED, SCAN_BELOW_PER_QUERY = 13000, 10000  # phnsw.h: the defaults of scan_below == 0
ALWAYS_SCAN = 2 ** 64 - 1


def scan_below_of(scan_below, per_query):
    if scan_below:
        return int(scan_below)
    return SCAN_BELOW_PER_QUERY if per_query else SCAN_BELOW_SHARED


def rule(c, scan_below, ef, k, n_nodes, per_query=True):
    """the route of a query with c candidates, in Python integers: scan iff c <= scan_below or c * ef < k * N"""
    c = int(c)
    return SCAN if c <= scan_below_of(scan_below, per_query) or c * int(ef) < int(k) * int(n_nodes) else GRAPH


def first_graph_count(ef, k, n_nodes):
    """the smallest c with c * ef >= k * N: ceil(k * N / ef)"""
    return -(-int(k) * int(n_nodes) // int(ef))


def compose(walk, scan, n, ef, k, n_nodes, allow=None, exclude=None, members=None, scan_below=0):
    """walk: (ids[nq, ef], d, len) -- the PHNSW_FILTER_STRICT rows of the graph search for EVERY query of the batch;
    scan: (ids[nq, k], d, len) -- the exact rows for every query.  -> ids[nq, k] u64, d f32, len u64, route u32 as
    the contract composes them: a scanned query takes its exact row; a graph query its strict row without exclude[q],
    cut to k, unless that holds fewer than min(k, c - e) entries -- then the exact row, route 2"""
    nq = len(scan[2])
    per_query = allow is not None and np.ndim(allow) == 2
    ids = np.full((nq, k), xr.EMPTY, dtype=np.uint64)
    d = np.full((nq, k), xr.FMAX, dtype=np.float32)
    ln = np.zeros(nq, dtype=np.uint64)
    route = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        c = int(np.count_nonzero(xr.candidates(n, allow, None, members, q)))        # what filter_count reports
        left = int(np.count_nonzero(xr.candidates(n, allow, exclude, members, q)))  # c - e
        r = rule(c, scan_below, ef, k, n_nodes, per_query)
        if r == GRAPH:
            m = int(walk[2][q])
            keep = np.ones(m, dtype=bool) if exclude is None else walk[0][q, :m] != np.uint64(int(exclude[q]))
            wi, wd = walk[0][q, :m][keep][:k], walk[1][q, :m][keep][:k]
            if len(wi) < min(k, left):
                r = GRAPH_THEN_SCAN
            else:
                ids[q, :len(wi)], d[q, :len(wi)], ln[q] = wi, wd, len(wi)
        if r != GRAPH:
            ids[q], d[q], ln[q] = scan[0][q], scan[1][q], scan[2][q]
        route[q] = r
    return ids, d, ln, route


def assert_complete(res, n, k, allow=None, exclude=None, members=None):
    """the call's guarantee: len == min(k, candidates), candidates only, ascending (distance, id), padded"""
    ids, d, ln = res[0], res[1], res[2]
    for q in range(len(ln)):
        cand = xr.candidates(n, allow, exclude, members, q)
        m = int(ln[q])
        assert m == min(k, int(np.count_nonzero(cand))), (q, m, int(np.count_nonzero(cand)))
        assert cand[ids[q, :m].astype(np.int64)].all(), (q, "an id that is not a candidate")
        assert len(set(ids[q, :m].tolist())) == m
        keys = list(zip(d[q, :m].tolist(), ids[q, :m].tolist()))
        assert keys == sorted(keys), (q, "not ascending by (distance, id)")
        assert (ids[q, m:] == xr.EMPTY).all() and (d[q, m:].view(np.uint32) == xr.FMAX.view(np.uint32)).all()
