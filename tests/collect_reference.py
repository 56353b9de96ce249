"""The collecting search (phnsw_search_collect*, include/phnsw.h) restated in Python on the pieces of filter_reference:
the plain search of search_layers with `exclude` alone, whose LAST layer's closest_nodes carries a second queue `kept` --
an oracle.PriorityQueue of capacity k over (distance, VectorId) -- seeded with the qualifying entries of the queue the
layer starts with and merged, at every hop, with the qualifying members of that hop's evaluated batch.  A row qualifies
iff it is allowed, is not exclude[q] and lies at most f32::MAX away.  With `extend` a hop that changed `kept` counts as
one that did something (the only change to the walk).  The result row is `kept`.

(A layer's nodes ascend in VectorId, so ordering `kept` by VectorId orders it by NodeId.)

tests/test_collect_cpu.py pins this to the unchanged oracle; tests/test_gpu_collect.py uses it as the yardstick."""
import heapq

import numpy as np

import oracle

from filter_reference import EMPTY, FMAX, _iter_len, closest_vectors, layers_of


def closest_nodes_collecting(nodes, nb, queue, kept, qualifies, drow, probe_depth, stats, extend):
    """filter_reference.closest_nodes (Layer::closest_nodes, lib.rs:175-248) with the `kept` queue beside `queue`"""
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
        while final and row[final - 1] == EMPTY:
            final -= 1
        batch = []
        for n in row[:final]:
            n = int(n)
            if n in visited:
                continue
            batch.append((float(drow[int(nodes[n])]), n))
            stats[0] += 1
        batch.sort()
        for d, n in batch:
            visited.add(n)
            heapq.heappush(heap, (d, n, -seq))
            seq += 1
        # every member of the batch merge_pairs sees, whether or not the layer's queue has room for it
        entering = sorted((d, int(nodes[n])) for d, n in batch if qualifies(int(nodes[n]), d))
        changed = False
        if entering:
            before = kept.data.copy()
            kept.merge([v for _, v in entering], [d for d, _ in entering])
            changed = bool((kept.data != before).any())
        did = queue.merge([n for _, n in batch], [d for d, _ in batch])
        if extend and changed:
            did = True
        if not did:
            probe_depth -= 1
            if probe_depth == 0:
                break


def search_one(layers, drow, sp, k, allowed, ex, extend, upto=0):
    """one query -> ids[k], d[k], len, [evaluations, hops]"""
    ef, upper, pd = sp
    nl = len(layers) if upto == 0 or upto > len(layers) else upto
    cand = oracle.PriorityQueue.new(ef)
    entry = int(layers[0][0][0])
    stats = [1, 0]
    cand.insert(entry, drow[entry])

    def include(v):  # the plain search's: closest_vectors' closure of search_layers
        return v != ex

    def qualifies(v, d):
        return v != ex and bool(allowed(v)) and np.float32(d) <= FMAX

    for i in range(nl - 1):
        cand.merge_pairs(closest_vectors(layers[i], cand, upper, pd, include, drow, stats))
    # the last layer: closest_vectors up to its call of closest_nodes; its tail and the merge into the running
    # candidates make the plain search's row, which a collecting search does not return
    nodes, nb, vec2node = layers[nl - 1]
    np_ = _iter_len(cand)
    queue = oracle.PriorityQueue.new(len(cand.data))
    queue.merge_pairs([(vec2node[int(cand.data[i])], cand.priorities[i]) for i in range(np_)])
    kept = oracle.PriorityQueue.new(k)
    seeds = sorted((float(cand.priorities[i]), int(cand.data[i])) for i in range(np_)
                   if qualifies(int(cand.data[i]), cand.priorities[i]))
    if seeds:
        kept.merge([v for _, v in seeds], [d for d, _ in seeds])
    closest_nodes_collecting(nodes, nb, queue, kept, qualifies, drow, pd, stats, extend)
    ln = _iter_len(kept)
    ids, d = kept.data.copy(), kept.priorities.copy()
    ids[ln:] = EMPTY
    d[ln:] = FMAX
    return ids, d, ln, stats


def search(ix, D, sp, k, allow=None, exclude=None, extend=False, upto=0, layers=None):
    """batched: D = filter_reference.distance_rows(...) [nq, n]; allow: bool [n] or [nq, n] or None (every row);
    exclude: [nq] ids or None -> ids[nq, k] u64, d[nq, k] f32, len[nq] u64, stats[nq, 2] u64"""
    layers = layers or layers_of(ix)
    nq = D.shape[0]
    ids = np.empty((nq, k), dtype=np.uint64)
    d = np.empty((nq, k), dtype=np.float32)
    ln = np.zeros(nq, dtype=np.uint64)
    st = np.zeros((nq, 2), dtype=np.uint64)
    allow = None if allow is None else np.asarray(allow, dtype=np.bool_)
    for q in range(nq):
        a = None if allow is None else (allow if allow.ndim == 1 else allow[q])
        ex = EMPTY if exclude is None else int(exclude[q])
        ids[q], d[q], ln[q], st[q] = search_one(layers, D[q], sp, k, (lambda v, a=a: a is None or a[v]), ex, extend, upto)
    return ids, d, ln, st
