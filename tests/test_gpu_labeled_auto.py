"""phnsw_search_labeled_auto[_device]: one call by row label that picks the posting-list scan or the label walk per query
and rescans what the walk left short.  Every comparison is on ids, distance bits, lengths, routes and statuses, no
tolerance anywhere.

Yardsticks, named per assertion below:
  * ROWS    -- tests/filter_auto_reference.compose of the two established BITMAP calls (search_batch_filtered strict,
               search_exact_filtered) over tests/labeled_reference.masks_of(column, want): masks the code under test
               never saw.
  * ROUTES  -- filter_auto_reference.rule evaluated on Labels.count(want).
  * COMPLETE-- filter_auto_reference.assert_complete: len == min(k, candidates), candidates only.

The world is that of tests/test_gpu_filter_auto.py (N = 5000, 70 queries: more than one wave of ballot lanes, no
multiple of 64).  The list lengths sit on the rule's edges by sizing labels to exactly those counts; a column is a
partition, so the edges are spread over three columns."""
import functools

import numpy as np
import pytest

import parallel_hnsw_amd as ph

import filter_auto_reference as ar
import labeled_reference as lr
from test_gpu_exact_filter import ring
from test_gpu_filter_auto import BELOW, EMPTY, K, KINDS, N, NQ, SP, same, world
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

NONE = lr.LABEL_NONE
ABSENT = 4242
E_INVALID = -1


def sized_column(sizes, seed, members=None, entry=None):
    """i64 [N]: label j + 1 on exactly sizes[j] vectors of the index, chosen at random (never `entry`, if given); the
    index's other vectors carry no label; vectors the index does not hold carry random ones of the same labels -- they
    are not listed, so no count changes"""
    rng = np.random.default_rng(seed)
    pool = np.arange(N) if members is None else np.nonzero(members)[0]
    if entry is not None:
        pool = pool[pool != entry]
    pool = rng.permutation(pool)
    lab = np.full(N, -1, dtype=np.int64)
    at = 0
    for j, c in enumerate(sizes):
        lab[pool[at:at + c]] = j + 1
        at += c
    assert at <= len(pool)
    if members is not None:
        out = np.nonzero(~members)[0]
        lab[out] = rng.integers(1, len(sizes) + 1, len(out))
    return lab


def edge_columns(w, ef=SP[0], k=K):
    """[(column, wanted labels)]: between them lists of 0, 1, k - 1, k, BELOW, BELOW + 1, e - 1, e rows and one of every
    vector of the index, e = the first count the second rule routes to the graph"""
    e, n = ar.first_graph_count(ef, k, w["n_nodes"]), w["n_nodes"]
    a = [1, k - 1, k, BELOW, BELOW + 1, e - 1]
    assert sum(a) <= n and e <= n
    return [(sized_column(a, 11, w["members"]), [ABSENT, NONE] + list(range(1, len(a) + 1))),
            (sized_column([e, n - e], 12, w["members"]), [1, 2]),
            (sized_column([n], 13, w["members"]), [1])]


def spread(values):
    return np.array([values[i % len(values)] for i in range(NQ)], dtype=np.int64)


def device_lauto(hix, lb, sp, k, queries=None, qids=None, want=None, exclude=None, scan_below=0, stream=0):
    """phnsw_search_labeled_auto_device with torch buffers -> ids u64, d, len u64, route, status; 64 guard words behind
    every buffer must come back as they went in"""
    import torch
    dev = torch.device("cuda", 0)
    keep = []

    def up(a, dt):
        t = torch.from_numpy(np.ascontiguousarray(a).view(dt) if dt is not None else np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t

    nq = len(queries) if queries is not None else len(qids)
    qd = qi = ex = ld = 0
    if queries is not None:
        ld = hix.store.ld
        qp = np.zeros((nq, ld), dtype=np.float32)
        qp[:, :queries.shape[1]] = queries
        qd = up(qp, None).data_ptr()
    else:
        qi = up(np.asarray(qids, dtype=np.uint32), np.int32).data_ptr()
    if exclude is not None:
        e32 = np.asarray(exclude, dtype=np.uint64).copy()
        e32[e32 >= N] = 0xFFFFFFFF
        ex = up(e32.astype(np.uint32), np.int32).data_ptr()
    wd = up(ph.hnsw.pack_labels(want, nq, "want"), np.int32).data_ptr()
    G = 64
    ids = torch.full((nq * k + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * k + G,), -1.0, dtype=torch.float32, device=dev)
    ln, route, status = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    hix.search_labeled_device(lb, nq, sp, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd, ldq=ld,
                              qids=qi, exclude=ex, want=wd, scan_below=scan_below, out_route=route.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert (ids[nq * k:] == 7).all() and (d[nq * k:] == -1.0).all()
    for t in (ln, route, status):
        assert (t[nq:] == -1).all()
    i64 = ids[:nq * k].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, k)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return (i64, d[:nq * k].cpu().numpy().reshape(nq, k), ln[:nq].cpu().numpy().view(np.uint32).astype(np.uint64),
            route[:nq].cpu().numpy().view(np.uint32), status[:nq].cpu().numpy())


def check(w, lab, lb, want, exclude=None, k=K, sp=SP, scan_below=BELOW, device=False, stored=(False, True), q=None,
          routes=True):
    """the host form (and the device form) on raw and stored queries against ROWS, ROUTES and COMPLETE; routes=False
    (the library's own scan_below): COMPLETE only.  Returns the host results."""
    hix = w["hix"]
    spp = ph.SearchParameters(*sp)
    masks = lr.masks_of(lab, want)
    out = []
    for st in stored:
        kw = dict(qids=w["qids"]) if st else dict(queries=w["q"] if q is None else q)
        got = hix.search_labeled(sp=spp, labels=lb, want=want, exclude=exclude, k=k, scan_below=scan_below, route=True, **kw)
        ar.assert_complete(got, N, k, masks, exclude, w["members"])  # COMPLETE
        if routes:
            walk = hix.search_batch_filtered(sp=spp, allow=masks, strict=True, exclude=exclude, **kw)
            scan = hix.search_exact_filtered(allow=masks, exclude=exclude, k=k, **kw)
            ref = ar.compose(walk, scan, N, sp[0], k, w["n_nodes"], masks, exclude, w["members"], scan_below)
            print("routes", np.bincount(got[3], minlength=3).tolist(), "expected", np.bincount(ref[3], minlength=3).tolist())
            np.testing.assert_array_equal(got[3], ref[3])  # ROWS: which graph rows the strict bitmap call leaves short
            same(got, ref)                                  # ROWS
            counts = lb.count(want)
            for i in range(NQ):                             # ROUTES
                r = ar.rule(counts[i], scan_below, sp[0], k, w["n_nodes"])
                assert got[3][i] == r or (got[3][i] == ar.GRAPH_THEN_SCAN and r == ar.GRAPH), (i, got[3][i], r)
        if device:
            dv = device_lauto(hix, lb, spp, k, want=want, exclude=exclude, scan_below=scan_below, **kw)
            assert not dv[4].any()
            same(dv, got)
            np.testing.assert_array_equal(dv[3], got[3])
        out.append(got)
    return out


# ---------------------------------------------------------------- 1: routes and rows on the rule's edges
@pytest.mark.parametrize("kind,dim", KINDS)
def test_routes_follow_the_rule_and_rows_are_the_established_calls(kind, dim):
    w = world(kind, dim)
    e = ar.first_graph_count(SP[0], K, N)
    seen = {}
    for lab, values in edge_columns(w):
        lb = ph.Labels(w["hix"], lab)
        want = spread(values)
        raw, st = check(w, lab, lb, want, device=True)
        counts = lb.count(want)
        for got in (raw, st):
            for c, r in zip(counts.tolist(), got[3].tolist()):
                seen.setdefault(c, set()).add(r)
        # exclude: each query's nearest candidate (EMPTY where there is none); every third query the entry vector
        ex = w["hix"].search_exact_labeled(queries=w["q"], labels=lb, want=want, k=1)[0][:, 0].copy()
        ex[2::3] = w["entry"]
        got = check(w, lab, lb, want, exclude=ex, device=True, stored=(False,))[0]
        assert not ((got[0] == ex[:, None]) & (ex[:, None] != EMPTY)).any()
        # ... and the rows are those of the routed BITMAP call with the same scan_below
        same(got, w["hix"].search_filtered(queries=w["q"], sp=ph.SearchParameters(*SP), allow=lr.masks_of(lab, want), exclude=ex,
                                           k=K, scan_below=BELOW))
    assert sorted(seen) == sorted([0, 1, K - 1, K, BELOW, BELOW + 1, e - 1, e, N - e, N])
    for c in (0, 1, K - 1, K, BELOW, BELOW + 1, e - 1, N - e):
        assert seen[c] == {ar.SCAN}, (c, seen[c])
    assert ar.SCAN not in seen[e] and seen[N] == {ar.GRAPH}  # every vector listed: the walk fills its row


def test_wider_queues_and_other_k():
    w = world("f32", 24)
    for sp, k in (((200, 200, 2), 10), ((64, 32, 2), 16), ((1024, 300, 2), 1)):
        for lab, values in edge_columns(w, sp[0], k)[:2]:
            check(w, lab, ph.Labels(w["hix"], lab), spread(values), sp=sp, k=k, device=sp[0] == 200, stored=(False,))


def test_the_scan_default_is_complete():
    w = world("f32", 24)
    for lab, values in edge_columns(w):
        check(w, lab, ph.Labels(w["hix"], lab), spread(values), scan_below=0, routes=False)
        check(w, lab, ph.Labels(w["hix"], lab), spread(values), scan_below=ar.ALWAYS_SCAN, stored=(False,))


# ---------------------------------------------------------------- 2: the fallback
FAR = ar.first_graph_count(SP[0], K, N) + 64  # a list long enough for the graph


@functools.lru_cache(maxsize=None)
def far_query(kind, dim):
    """(j, rows): the first query whose strict BITMAP walk over the FAR rows farthest from it (smallest cosine, numpy on the
    store's rows) comes back shorter than K, and those rows.  What the walk's upper layers pass on can still fill a row,
    so the precondition is looked for query by query, on the established call"""
    w = world(kind, dim)
    for j in range(NQ):
        rows = np.argsort(-w["cos"][j], kind="stable")[N - FAR:]
        allow = np.zeros((1, N), dtype=bool)
        allow[0, rows] = True
        if w["hix"].search_batch_filtered(queries=w["q"][j:j + 1], sp=ph.SearchParameters(*SP), allow=allow, strict=True)[2][0] < K:
            return j, rows
    raise AssertionError("no query's strict walk is short: the precondition of the fallback tests does not hold")


@pytest.mark.parametrize("kind,dim", KINDS)
def test_the_fallback_really_runs(kind, dim):
    """Label 1 goes to the ceil(K * N / 16) + 64 rows FARTHEST (smallest cosine) from one query (far_query), label 2 to the
    rest; that query, copied to five places of the batch, wants label 1: the rule says graph, and a walk towards the
    query ends among rows it may not return.  The precondition -- the strict bitmap call returns fewer than K -- is
    asserted."""
    w = world(kind, dim)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    j, far = far_query(kind, dim)
    c = FAR
    lab = np.full(N, 2, dtype=np.int64)
    lab[far] = 1
    lb = ph.Labels(hix, lab)
    assert ar.rule(c, BELOW, SP[0], K, N) == ar.GRAPH and lb.count([1])[0] == c
    copies = [0, 7, 33, 64, 69]
    q = w["q"].copy()
    q[copies] = w["q"][j]
    want = np.full(NQ, 2, dtype=np.int64)
    want[copies] = 1
    masks = lr.masks_of(lab, want)
    strict = hix.search_batch_filtered(queries=q, sp=spp, allow=masks, strict=True)
    short = strict[2] < K
    print("strict graph rows shorter than k:", int(short.sum()), "of", NQ, "lengths", strict[2].tolist())
    assert short[copies].all()  # the precondition, on the established call
    got = check(w, lab, lb, want, device=True, stored=(False,), q=q)[0]
    assert (got[3] == ar.GRAPH_THEN_SCAN).sum() >= 1
    np.testing.assert_array_equal(np.nonzero(got[3] == ar.GRAPH_THEN_SCAN)[0], copies)  # the others want label 2: scanned
    assert (np.delete(got[3], copies) == ar.SCAN).all()
    short = got[3] == ar.GRAPH_THEN_SCAN
    scan = hix.search_exact_labeled(queries=q, labels=lb, want=want, k=K)
    same([x[short] for x in got[:3]], [x[short] for x in scan])  # those rows are the scan's
    assert (got[2] == K).all()


# ---------------------------------------------------------------- 3: the order of the batch, the scan's knobs
@pytest.mark.parametrize("kind,dim", KINDS)
def test_results_do_not_depend_on_the_order_of_the_batch_or_the_slices(monkeypatch, kind, dim):
    w = world(kind, dim)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    j, far = far_query(kind, dim)
    lab = np.full(N, -1, dtype=np.int64)
    lab[far] = 1  # the walk of query j leaves it short
    rest = np.random.default_rng(9).permutation(np.setdiff1d(np.arange(N), far))
    lab[rest[:BELOW]] = 2
    lab[rest[BELOW:BELOW + K - 1]] = 3
    lb = ph.Labels(hix, lab)
    want = spread([1, 2, 3, ABSENT, 1])
    want[j] = 1
    ex = hix.search_exact_labeled(queries=w["q"], labels=lb, want=want, k=1)[0][:, 0].copy()
    ex[j] = EMPTY  # (its nearest candidate stays: the walk is short without help)
    base = hix.search_labeled(queries=w["q"], sp=spp, labels=lb, want=want, exclude=ex, k=K, scan_below=BELOW, route=True)
    assert len(set(base[3].tolist())) == 3  # all three routes are in play
    for perm in (np.arange(NQ)[::-1], np.random.default_rng(3).permutation(NQ)):
        got = hix.search_labeled(queries=w["q"][perm], sp=spp, labels=lb, want=want[perm], exclude=ex[perm], k=K,
                                 scan_below=BELOW, route=True)
        same(got, [x[perm] for x in base])
        np.testing.assert_array_equal(got[3], base[3][perm])
    for kv in (dict(PHNSW_LABEL_SLICES="1"), dict(PHNSW_LABEL_SLICES="3"), dict(PHNSW_LABEL_TILE="1")):
        with env(monkeypatch, **kv):
            got = hix.search_labeled(queries=w["q"], sp=spp, labels=lb, want=want, exclude=ex, k=K, scan_below=BELOW, route=True)
        same(got, base)
        np.testing.assert_array_equal(got[3], base[3])


# ---------------------------------------------------------------- 4: an index over part of its store
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("i8q", 24)])
def test_an_index_over_every_second_vector(kind, dim):
    w = world(kind, dim, 2)
    assert w["n_nodes"] == N // 2 and ar.first_graph_count(SP[0], K, w["n_nodes"]) == 1563
    for lab, values in edge_columns(w):
        lb = ph.Labels(w["hix"], lab)
        assert lb.listed <= N // 2
        want = spread(values)
        raw, _ = check(w, lab, lb, want, device=True)
        assert not (raw[0][raw[0] != EMPTY] % 2).any()
        # exclude: odd ids (labelled, not listed: e_q = 0), the entry vector, the nearest candidate
        ex = w["hix"].search_exact_labeled(queries=w["q"], labels=lb, want=want, k=1)[0][:, 0].copy()
        ex[0::3] = np.arange(NQ)[0::3] * 2 + 1
        ex[8::9] = w["entry"]
        check(w, lab, lb, want, exclude=ex, device=True, stored=(False,))


# ---------------------------------------------------------------- 5: the device form on a stream of its own
def test_device_form_on_a_side_stream():
    import torch
    w = world("f32", 24)
    spp = ph.SearchParameters(*SP)
    lab, values = edge_columns(w)[1]  # a list at the first graph count, and the rest of the index: scanned
    lb = ph.Labels(w["hix"], lab)
    want = spread(values + [ABSENT, NONE])
    ex = w["hix"].search_exact_labeled(qids=w["qids"], labels=lb, want=want, k=1)[0][:, 0].copy()
    host = w["hix"].search_labeled(qids=w["qids"], sp=spp, labels=lb, want=want, exclude=ex, k=K, scan_below=BELOW, route=True)
    assert (host[3] != ar.SCAN).any() and (host[3] == ar.SCAN).any()
    stream = torch.cuda.Stream()
    dv = device_lauto(w["hix"], lb, spp, K, qids=w["qids"], want=want, exclude=ex, scan_below=BELOW, stream=stream.cuda_stream)
    assert set(dv[4].tolist()) == {0}
    same(dv, host)
    np.testing.assert_array_equal(dv[3], host[3])
    # a Stored id at or past n: scanned whatever its count, status 4, an empty row; its neighbours are untouched by it
    bad = w["qids"].copy()
    bad[[5, 69]] = [N, 0xFFFFFFF0]
    dv = device_lauto(w["hix"], lb, spp, K, qids=bad, want=want, exclude=ex, scan_below=BELOW, stream=stream.cuda_stream)
    ok = np.ones(NQ, dtype=bool)
    ok[[5, 69]] = False
    assert (dv[4][~ok] == 4).all() and not dv[4][ok].any() and not dv[2][~ok].any() and (dv[0][~ok] == EMPTY).all()
    assert (dv[3][~ok] == ar.SCAN).all()
    same([x[ok] for x in dv[:3]], [x[ok] for x in host[:3]])


# ---------------------------------------------------------------- 6: argument checks
def test_argument_checks():
    w = world("f32", 24)
    hix, q = w["hix"], w["q"]
    lab = sized_column([100, 200], 3)
    lb = ph.Labels(hix, lab)
    want = spread([1, 2])
    sp = ph.SearchParameters(16, 16, 2)
    for k in (0, 17):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_labeled(queries=q, sp=sp, labels=lb, want=want, k=k)
        assert e.value.code == E_INVALID
        assert str(e.value) == ("phnsw error -1: phnsw_search_labeled_auto: k must be 1..number_of_candidates (got %d, "
                                "number_of_candidates 16)" % k)
        with pytest.raises(ph.PhnswError) as e:
            hix.search_labeled_device(lb, 4, sp, k, 8, 8, 8, 8, qids=8, want=8)
        assert e.value.code == E_INVALID and "k must be 1..number_of_candidates" in str(e.value)
    other = ph.Hnsw.from_layers(hix.store, ring(np.arange(N)))  # a handle of another index
    for call in (lambda: other.search_labeled(queries=q, sp=sp, labels=lb, want=want, k=3),
                 lambda: other.search_labeled_device(lb, 4, sp, 3, 8, 8, 8, 8, qids=8, want=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == E_INVALID and "the labels are stale" in str(e.value) and "phnsw_search_labeled_auto" in str(e.value)
    for bad in (dict(qids=8), dict(queries=16, ldq=24, qids=8, want=8), dict(want=8)):  # no want, both, neither
        with pytest.raises(ph.PhnswError) as e:
            hix.search_labeled_device(lb, 4, sp, 3, 8, 8, 8, 8, **bad)
        assert e.value.code == E_INVALID and "phnsw_search_labeled_auto_device: invalid argument" in str(e.value)
    ids, d, ln = hix.search_labeled(queries=np.zeros((0, 24), dtype=np.float32), sp=sp, labels=lb, want=np.zeros(0, dtype=np.int64), k=3)
    assert ids.shape == (0, 3)  # nq == 0: a no-op
