"""search_layers / Layer::closest_vectors / Layer::closest_nodes (src/search.rs:93-140, src/lib.rs:175-277) restated in
Python with an ARBITRARY `include` closure -- the reference is generic over it (lib.rs:250-277) while search_layers and
the oracle instantiate only `|v| Some(v) != exclude`.  Built on the oracle's own pieces, so nothing about them is
derived a second time:
  * distances: one exhaustive orc_bruteforce per query set (value_families.oracle_matrix), looked up by VectorId;
  * queues: oracle.PriorityQueue (the ctypes orc_pq): the quirks of insert and merge are the oracle's;
  * layers: oracle.Index.layer.
tests/test_filter_cpu.py pins this restatement to the unchanged oracle (all-ones filter = oracle.search, one cleared bit
= oracle.search(exclude=...)); tests/test_gpu_filter.py then uses it as the yardstick of the filtered GPU searches."""
import heapq

import numpy as np

import oracle

EMPTY = 0xFFFFFFFFFFFFFFFF
FMAX = np.float32(3.4028234663852886e38)


def pack(allow):
    """bool [..., n] -> u32 words [..., ceil(n/32)]: bit v % 32 of word v // 32 = allow[v] (the layout of phnsw.h)"""
    a = np.asarray(allow, dtype=np.bool_)
    n = a.shape[-1]
    padded = np.zeros(a.shape[:-1] + ((n + 31) // 32 * 32,), dtype=np.bool_)
    padded[..., :n] = a
    out = np.zeros(a.shape[:-1] + ((n + 31) // 32,), dtype=np.uint32)
    for b in range(32):
        out |= padded[..., b::32].astype(np.uint32) << np.uint32(b)
    return out


def distance_rows(ix, queries=None, qids=None, mode=None):
    """[nq, n] f32: the oracle's distance of every query to every stored vector, in `mode` (default: the index's)"""
    from value_families import oracle_matrix
    rows = ix.rows
    q = rows[np.asarray(qids, dtype=np.int64), :ix.dim] if queries is None else np.atleast_2d(queries)[:, :ix.dim]
    return oracle_matrix(rows, np.ascontiguousarray(q, dtype=np.float32), ix.metric, ix._sum_mode if mode is None else mode)


def layers_of(ix):
    """[(nodes, neighbors[n, W], vec -> node dict)] top first"""
    out = []
    for l in range(ix.layer_count):
        nodes, nb = ix.layer(l)
        out.append((nodes, nb, {int(v): i for i, v in enumerate(nodes)}))
    return out


def _iter_len(pq):
    """PriorityQueueIter stops at the first empty id (priority_queue.rs:207-222)"""
    e = np.nonzero(pq.data == EMPTY)[0]
    return int(e[0]) if len(e) else len(pq.data)


def closest_nodes(nodes, nb, queue, drow, probe_depth, stats):
    """Layer::closest_nodes  lib.rs:175-248 as orc_closest_nodes runs it (visit_queue = a heap on (d, id, -seq))"""
    ninit = _iter_len(queue)
    heap = [(float(queue.priorities[i]), int(queue.data[i]), -(ninit - i)) for i in range(ninit)]
    heapq.heapify(heap)
    visited = set(int(x) for x in queue.data[:ninit])
    seq = ninit + 1
    while heap:
        _, cur, _ = heapq.heappop(heap)
        stats[1] += 1
        row = nb[cur]
        final = len(row)
        while final and row[final - 1] == EMPTY:  # get_final_neighbor_idx: trailing sentinels only
            final -= 1
        batch = []
        for n in row[:final]:
            n = int(n)
            if n in visited:
                continue
            batch.append((float(drow[int(nodes[n])]), n))
            stats[0] += 1
        batch.sort()  # by (OrderedFloat(d), id)  lib.rs:206
        for d, n in batch:
            visited.add(n)
            heapq.heappush(heap, (d, n, -seq))
            seq += 1
        did = queue.merge([n for _, n in batch], [d for d, _ in batch])
        if not did:
            probe_depth -= 1
            if probe_depth == 0:
                break


def closest_vectors(layer, cand, candidate_count, probe_depth, include, drow, stats):
    """Layer::closest_vectors  lib.rs:250-277 with the caller's `include`"""
    nodes, nb, vec2node = layer
    np_ = _iter_len(cand)
    pairs = [(vec2node[int(cand.data[i])], cand.priorities[i]) for i in range(np_)]  # get_node(v).unwrap()
    queue = oracle.PriorityQueue.new(len(cand.data))
    queue.merge_pairs(pairs)
    closest_nodes(nodes, nb, queue, drow, probe_depth, stats)
    out = []
    for i in range(_iter_len(queue)):
        if len(out) >= candidate_count:
            break
        v = int(nodes[int(queue.data[i])])
        if include(v):
            out.append((v, queue.priorities[i]))
    return out


def search_one(layers, drow, sp, include, upto=0):
    """search_layers  search.rs:93-140 for one query -> ids[ef], d[ef], len, [evaluations, hops]"""
    ef, upper, pd = sp
    nl = len(layers) if upto == 0 or upto > len(layers) else upto
    cand = oracle.PriorityQueue.new(ef)
    entry = int(layers[0][0][0])
    stats = [1, 0]
    cand.insert(entry, drow[entry])  # before any filter runs  search.rs:102-111
    for i in range(nl):
        count = ef if (nl == 1 or i == nl - 1) else upper
        cand.merge_pairs(closest_vectors(layers[i], cand, count, pd, include, drow, stats))
    ln = _iter_len(cand)
    ids, d = cand.data.copy(), cand.priorities.copy()
    ids[ln:] = EMPTY
    d[ln:] = FMAX
    return ids, d, ln, stats


def search(ix, D, sp, allow=None, exclude=None, upto=0, layers=None):
    """batched: D = distance_rows(...) [nq, n]; allow: bool [n] or [nq, n] or None; exclude: [nq] ids or None.
    -> ids[nq, ef] u64, d[nq, ef] f32, len[nq] u64, stats[nq, 2] u64 (evaluations, hops as orc_search.c counts them)"""
    layers = layers or layers_of(ix)
    nq, ef = D.shape[0], sp[0]
    ids = np.empty((nq, ef), dtype=np.uint64)
    d = np.empty((nq, ef), dtype=np.float32)
    ln = np.zeros(nq, dtype=np.uint64)
    st = np.zeros((nq, 2), dtype=np.uint64)
    allow = None if allow is None else np.asarray(allow, dtype=np.bool_)
    for q in range(nq):
        a = None if allow is None else (allow if allow.ndim == 1 else allow[q])
        ex = EMPTY if exclude is None else int(exclude[q])

        def include(v, a=a, ex=ex):
            return v != ex and (a is None or bool(a[v]))

        ids[q], d[q], ln[q], st[q] = search_one(layers, D[q], sp, include, upto)
    return ids, d, ln, st


def strict(res, allow):
    """PHNSW_FILTER_STRICT applied to a non-strict result: disallowed ids leave the rows, in order"""
    ids, d, ln = res[0].copy(), res[1].copy(), res[2].copy()
    allow = np.asarray(allow, dtype=np.bool_)
    for q in range(ids.shape[0]):
        a = allow if allow.ndim == 1 else allow[q]
        n = int(ln[q])
        keep = np.array([bool(a[int(v)]) for v in ids[q, :n]], dtype=np.bool_)
        k = int(keep.sum())
        ids[q, :k], d[q, :k] = ids[q, :n][keep], d[q, :n][keep]
        ids[q, k:], d[q, k:] = EMPTY, FMAX
        ln[q] = k
    return (ids, d, ln) + tuple(res[3:])
