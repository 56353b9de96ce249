"""phnsw_search_exact_radius restated in numpy: per query the candidates with d < radius, ascending by (distance, id), as
CSR.  The distances come from the caller (a matrix D[nq, n] made by a yardstick that is not the code under test:
filter_reference.distance_rows, value_families.oracle_matrix), so nothing here computes one."""
import numpy as np

from exact_filter_reference import candidates


def radii(radius, nq):
    """radius as the call takes it: f32 [nq], a scalar broadcast"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))


def exact_radius(D, radius, allow=None, exclude=None, members=None):
    """-> first[nq + 1] u64, ids[total] u64, d[total] f32.  A candidate (exact_filter_reference.candidates) is kept iff
    D[q, v] < radius[q] in float32 -- false for a NaN on either side and for +inf < +inf -- and the radius is above zero
    (the call's rule: a zero or negative radius matches nothing, whatever sign a metric's distance has).  Order: a
    stable sort by distance over ascending ids.  A kept -0.0 is reported as +0.0, as the exact top-k calls report it."""
    D = np.asarray(D, dtype=np.float32)
    nq, n = D.shape
    r = radii(radius, nq)
    first = np.zeros(nq + 1, dtype=np.uint64)
    ids, d = [], []
    for q in range(nq):
        v = np.nonzero(candidates(n, allow, exclude, members, q))[0]
        with np.errstate(invalid="ignore"):
            v = v[(D[q, v] < r[q]) & (r[q] > np.float32(0))]
        v = v[np.argsort(D[q, v], kind="stable")]
        ids.append(v.astype(np.uint64))
        d.append(D[q, v] + np.float32(0))
        first[q + 1] = first[q] + np.uint64(len(v))
    return first, np.concatenate(ids) if ids else np.zeros(0, np.uint64), np.concatenate(d) if d else np.zeros(0, np.float32)


def segment(res, q):
    """(ids, d) of query q"""
    first, ids, d = res
    return ids[int(first[q]):int(first[q + 1])], d[int(first[q]):int(first[q + 1])]


def mth_smallest(D, m, allow=None, exclude=None, members=None):
    """f32 [nq]: the m[q]-th smallest distance (0 = the smallest) among the candidates of query q; m a scalar or [nq]"""
    D = np.asarray(D, dtype=np.float32)
    nq, n = D.shape
    m = np.broadcast_to(np.asarray(m, dtype=np.int64), (nq,))
    out = np.zeros(nq, dtype=np.float32)
    for q in range(nq):
        v = np.nonzero(candidates(n, allow, exclude, members, q))[0]
        out[q] = np.sort(D[q, v], kind="stable")[m[q]]
    return out


# ---------------------------------------------------------------- the walk (phnsw_search_batch_radius)
CAP_LIMIT = 1024  # the LDS queues of the kernels
ST_CAPACITY = 6
EMPTY = 0xFFFFFFFFFFFFFFFF
FMAX = np.float32(3.4028234663852886e38)


def growth_loop(layer, queue, drow, radius, probe_depth, stats, cap_limit=None):
    """threshold_nn's loop (lib.rs:944-953) on `queue` over a bottom layer, restated on filter_reference.closest_nodes and
    oracle.PriorityQueue; resize_capacity re-wraps the padded arrays.  -> (queue, trace): trace = closest_nodes calls,
    the capacity before each call, and whether a doubling past cap_limit ended the loop (`over`)"""
    import oracle
    import filter_reference as fr
    nodes, nb = layer[0], layer[1]
    r = np.float32(radius)
    last, last_size = np.float32(0.0), 0
    trace = dict(calls=0, caps=[], over=False, start=fr._iter_len(queue))
    while last < r and fr._iter_len(queue) > last_size:
        last_size = fr._iter_len(queue)
        trace["caps"].append(len(queue.data))
        fr.closest_nodes(nodes, nb, queue, drow, probe_depth, stats)
        trace["calls"] += 1
        n = fr._iter_len(queue)
        last = queue.priorities[n - 1]
        if last < r and n == len(queue.data):
            if cap_limit is not None and 2 * n > cap_limit:
                trace["over"] = True
                break
            queue = oracle.PriorityQueue(np.concatenate([queue.data, np.full(n, EMPTY, dtype=np.uint64)]),
                                         np.concatenate([queue.priorities, np.full(n, FMAX, dtype=np.float32)]))
    trace["capacity"] = len(queue.data)
    return queue, trace


def queue_result(layer, queue, radius, skip_node=None, skip_vector=None):
    """lib.rs:954-959: the queue's entries other than the skipped one, taken while d < radius, as VectorIds"""
    import filter_reference as fr
    nodes = layer[0]
    out = []
    for i in range(fr._iter_len(queue)):
        n = int(queue.data[i])
        v = int(nodes[n])
        if n == skip_node or v == skip_vector:
            continue
        if not queue.priorities[i] < np.float32(radius):
            break
        out.append((v, queue.priorities[i]))
    return out


def search_radius_one(layers, drow, sp, radius, exclude=EMPTY, max_out=64, cap_limit=CAP_LIMIT):
    """the walk for one query: search_layers over layers[0 .. L-1) (search.rs:93-140), the running candidates mapped into
    a bottom-layer queue of capacity number_of_candidates (lib.rs:258-266), growth_loop, queue_result.
    -> ids[max_out] u64, d[max_out] f32, out_len, status, [evaluations, hops], trace"""
    import oracle
    import filter_reference as fr
    ef, upper, pd = sp
    cand = oracle.PriorityQueue.new(ef)
    entry = int(layers[0][0][0])
    stats = [1, 0]
    cand.insert(entry, drow[entry])
    include = lambda v: v != exclude
    for i in range(len(layers) - 1):
        cand.merge_pairs(fr.closest_vectors(layers[i], cand, upper, pd, include, drow, stats))
    ids = np.full(max_out, EMPTY, dtype=np.uint64)
    d = np.full(max_out, FMAX, dtype=np.float32)
    if not np.float32(radius) > 0:  # `while last < threshold` with last = 0.0: no bottom-layer call
        return ids, d, 0, 0, stats, dict(calls=0, caps=[], over=False, capacity=ef, start=0)
    nodes, nb, vec2node = layers[-1]
    queue = oracle.PriorityQueue.new(ef)
    queue.merge_pairs([(vec2node[int(cand.data[i])], cand.priorities[i]) for i in range(fr._iter_len(cand))])
    queue, trace = growth_loop(layers[-1], queue, drow, radius, pd, stats, cap_limit)
    if trace["over"]:
        return ids, d, 0, ST_CAPACITY, stats, trace
    res = queue_result(layers[-1], queue, radius, skip_vector=exclude)
    for j, (v, dv) in enumerate(res[:max_out]):
        ids[j], d[j] = v, dv
    return ids, d, len(res), 0, stats, trace


def search_radius(layers, D, sp, radius, exclude=None, max_out=64):
    """batched -> ids[nq, max_out], d, len[nq] u64, status[nq] u32, stats[nq, 2] u64, traces"""
    nq = D.shape[0]
    r = radii(radius, nq)
    ids = np.empty((nq, max_out), dtype=np.uint64)
    d = np.empty((nq, max_out), dtype=np.float32)
    ln, status, st, traces = np.zeros(nq, np.uint64), np.zeros(nq, np.uint32), np.zeros((nq, 2), np.uint64), []
    for q in range(nq):
        ex = EMPTY if exclude is None else int(exclude[q])
        ids[q], d[q], ln[q], status[q], st[q], t = search_radius_one(layers, D[q], sp, r[q], ex, max_out)
        traces.append(t)
    return ids, d, ln, status, st, traces
