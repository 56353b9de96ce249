"""phnsw_search_labelset_auto[_device]: one call by a SET of row labels per query that picks the scan by set or the walk by
set per query and rescans what the walk left short.  Every comparison is on ids, distance bits, lengths, routes and
statuses, no tolerance anywhere.

Yardsticks, named per assertion below:
  * ROWS    -- tests/filter_auto_reference.compose of the two established BITMAP calls (search_batch_filtered strict,
               search_exact_filtered) over tests/labelset_reference.masks_of_sets(column, sets): masks the code under test
               never saw.
  * ROUTES  -- filter_auto_reference.rule evaluated on Labels.count_sets(want).
  * COMPLETE-- filter_auto_reference.assert_complete: len == min(k, candidates), candidates only.

The world is that of tests/test_gpu_filter_auto.py (N = 5000, 70 queries).  One column carries lists sized so that the
UNIONS of two of them sit on the rule's edges."""
import numpy as np
import pytest

import parallel_hnsw_amd as ph

import filter_auto_reference as ar
from test_gpu_exact_filter import ring
from test_gpu_exact_labelset import staged_labelset
from test_gpu_exact_shared import fetch
from test_gpu_filter_auto import BELOW, EMPTY, K, KINDS, N, NQ, SP, same, world
from test_gpu_i8q import env
from test_gpu_labeled_auto import ABSENT, FAR, NONE, far_query, sized_column
from test_gpu_labelset_walk import masks_for

pytestmark = pytest.mark.gpu

E_INVALID = -1


def edge_world(w, ef=SP[0], k=K, seed=21):
    """(column, sets, counts): labels 1..11 on lists of 1, 4, 5, 6, 40, 60, 61, e - 125, 124, 125 and the rest of the index's
    vectors, and sets whose unions count exactly counts = [0, 0, 1, k - 1, k, BELOW, BELOW + 1, e - 1, e, n_nodes] -- every
    count of 2 or more the union of at least two non-empty lists; some sets carry a duplicate and a NONE.  e = the first
    count the second rule routes to the graph"""
    assert (k, BELOW) == (10, 100)
    n, e = w["n_nodes"], ar.first_graph_count(ef, k, w["n_nodes"])
    sizes = [1, 4, 5, 6, 40, 60, 61, e - 125, 124, 125]
    sizes.append(n - sum(sizes))
    assert min(sizes) >= 1
    lab = sized_column(sizes, seed, w["members"])
    sets = [[], [ABSENT, NONE], [1, 1, NONE], [2, 3], [2, 4, NONE], [5, 6], [5, 7, 5], [8, 9], [10, NONE, 8],
            list(range(1, 12)) + [NONE]]
    return lab, sets, [0, 0, 1, k - 1, k, BELOW, BELOW + 1, e - 1, e, n]


def spread(sets):
    return [list(sets[i % len(sets)]) for i in range(NQ)]


def device_sauto(hix, lb, sp, k, queries=None, qids=None, want=None, exclude=None, scan_below=0, stream=0, first=None):
    """phnsw_search_labelset_auto_device with torch buffers -> ids u64, d, len u64, route, status; 64 guard words behind
    every buffer must come back as they went in.  first: offsets of the test's own over the values of `want`"""
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
    f32, v32 = ph.hnsw.pack_label_sets(want, nq)
    if first is not None:
        f32 = np.asarray(first, dtype=np.uint32)
    fd = up(f32, np.int32).data_ptr()
    vd = up(v32, np.int32).data_ptr() if len(v32) else 0
    G = 64
    ids = torch.full((nq * k + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * k + G,), -1.0, dtype=torch.float32, device=dev)
    ln, route, status = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    hix.search_labelset_device(lb, nq, len(v32), sp, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(),
                               queries=qd, ldq=ld, qids=qi, exclude=ex, want_first=fd, want_values=vd, scan_below=scan_below,
                               out_route=route.data_ptr(), stream=stream)
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
    """the host form (and the device form) on raw and stored queries against ROWS, ROUTES and COMPLETE; routes=False:
    COMPLETE only.  Returns the host results."""
    hix = w["hix"]
    spp = ph.SearchParameters(*sp)
    masks = masks_for(lab, want)
    out = []
    for st in stored:
        kw = dict(qids=w["qids"]) if st else dict(queries=w["q"] if q is None else q)
        got = hix.search_labelset(sp=spp, labels=lb, want=want, exclude=exclude, k=k, scan_below=scan_below, route=True, **kw)
        ar.assert_complete(got, N, k, masks, exclude, w["members"])  # COMPLETE
        if routes:
            walk = hix.search_batch_filtered(sp=spp, allow=masks, strict=True, exclude=exclude, **kw)
            scan = hix.search_exact_filtered(allow=masks, exclude=exclude, k=k, **kw)
            ref = ar.compose(walk, scan, N, sp[0], k, w["n_nodes"], masks, exclude, w["members"], scan_below)
            print("routes", np.bincount(got[3], minlength=3).tolist(), "expected", np.bincount(ref[3], minlength=3).tolist())
            np.testing.assert_array_equal(got[3], ref[3])  # ROWS: which graph rows the strict bitmap call leaves short
            same(got, ref)                                  # ROWS
            counts = lb.count_sets(want)
            for i in range(NQ):                             # ROUTES
                r = ar.rule(counts[i], scan_below, sp[0], k, w["n_nodes"])
                assert got[3][i] == r or (got[3][i] == ar.GRAPH_THEN_SCAN and r == ar.GRAPH), (i, got[3][i], r)
        if device:
            dv = device_sauto(hix, lb, spp, k, want=want, exclude=exclude, scan_below=scan_below, **kw)
            assert not dv[4].any()
            same(dv, got)
            np.testing.assert_array_equal(dv[3], got[3])
        out.append(got)
    return out


# ---------------------------------------------------------------- 1: routes and rows on the rule's edges
@pytest.mark.parametrize("kind,dim", KINDS)
def test_routes_follow_the_rule_and_rows_are_the_established_calls(kind, dim):
    w = world(kind, dim)
    hix = w["hix"]
    e = ar.first_graph_count(SP[0], K, N)
    lab, sets, counts = edge_world(w)
    assert counts == [0, 0, 1, K - 1, K, BELOW, BELOW + 1, e - 1, e, N]
    lb = ph.Labels(hix, lab)
    want = spread(sets)
    np.testing.assert_array_equal(lb.count_sets(want), [counts[i % len(counts)] for i in range(NQ)])
    raw, st = check(w, lab, lb, want, device=True)
    seen = {}
    for got in (raw, st):
        for i, r in enumerate(got[3].tolist()):
            seen.setdefault(counts[i % len(counts)], set()).add(r)
    for c in (0, 1, K - 1, K, BELOW, BELOW + 1, e - 1):
        assert seen[c] == {ar.SCAN}, (c, seen[c])
    assert ar.SCAN not in seen[e] and seen[N] == {ar.GRAPH}  # every vector listed: the walk fills its row
    # exclude: each query's nearest candidate (EMPTY where there is none); every third query the entry vector
    ex = hix.search_exact_labelset(queries=w["q"], labels=lb, want=want, k=1)[0][:, 0].copy()
    ex[2::3] = w["entry"]
    got = check(w, lab, lb, want, exclude=ex, device=True, stored=(False,))[0]
    assert not ((got[0] == ex[:, None]) & (ex[:, None] != EMPTY)).any()
    # ... and the rows are those of the routed BITMAP call with the same scan_below
    same(got, hix.search_filtered(queries=w["q"], sp=ph.SearchParameters(*SP), allow=masks_for(lab, want), exclude=ex, k=K,
                                  scan_below=BELOW))


# ---------------------------------------------------------------- 2: the fallback
@pytest.mark.parametrize("kind,dim", KINDS)
def test_the_fallback_really_runs(kind, dim):
    """The construction of test_gpu_labeled_auto.test_the_fallback_really_runs with the FAR rows farthest from one query
    split between labels 1 and 3 and that query, copied to five places of the batch, wanting both: the rule says graph,
    and a walk towards the query ends among rows it may not return.  The precondition -- the strict bitmap call returns
    fewer than K -- is asserted."""
    w = world(kind, dim)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    j, far = far_query(kind, dim)
    lab = np.full(N, 2, dtype=np.int64)
    lab[far[0::2]] = 1
    lab[far[1::2]] = 3
    lb = ph.Labels(hix, lab)
    assert ar.rule(FAR, BELOW, SP[0], K, N) == ar.GRAPH and lb.count_sets([[1, 3]])[0] == FAR
    assert 0 < lb.count([1])[0] < FAR and 0 < lb.count([3])[0] < FAR
    copies = [0, 7, 33, 64, 69]
    q = w["q"].copy()
    q[copies] = w["q"][j]
    want = [[2]] * NQ
    for c in copies:
        want[c] = [3, 1]
    masks = masks_for(lab, want)
    strict = hix.search_batch_filtered(queries=q, sp=spp, allow=masks, strict=True)
    short = strict[2] < K
    print("strict graph rows shorter than k:", int(short.sum()), "of", NQ, "lengths", strict[2].tolist())
    assert short[copies].all()  # the precondition, on the established call
    got = check(w, lab, lb, want, device=True, stored=(False,), q=q)[0]
    np.testing.assert_array_equal(np.nonzero(got[3] == ar.GRAPH_THEN_SCAN)[0], copies)  # the others want label 2: scanned
    assert (np.delete(got[3], copies) == ar.SCAN).all()
    short = got[3] == ar.GRAPH_THEN_SCAN
    scan = hix.search_exact_labelset(queries=q, labels=lb, want=want, k=K)
    same([x[short] for x in got[:3]], [x[short] for x in scan])  # those rows are the scan's
    assert (got[2] == K).all()


# ---------------------------------------------------------------- 3: the order of the batch, the scan's knobs
@pytest.mark.parametrize("kind,dim", KINDS)
def test_results_do_not_depend_on_the_order_of_the_batch_or_the_slices(monkeypatch, kind, dim):
    w = world(kind, dim)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    j, far = far_query(kind, dim)
    lab = np.full(N, -1, dtype=np.int64)
    lab[far[0::2]] = 1  # the walk of query j over labels 1 and 4 leaves it short
    lab[far[1::2]] = 4
    rest = np.random.default_rng(9).permutation(np.setdiff1d(np.arange(N), far))
    lab[rest[:BELOW // 2]] = 2
    lab[rest[BELOW // 2:BELOW]] = 5
    lab[rest[BELOW:BELOW + K - 1]] = 3
    lb = ph.Labels(hix, lab)
    want = spread([[1, 4], [2, 5], [3, NONE, 3], [ABSENT], [4, 1, 4]])
    want[j] = [1, 4]
    ex = hix.search_exact_labelset(queries=w["q"], labels=lb, want=want, k=1)[0][:, 0].copy()
    ex[j] = EMPTY  # (its nearest candidate stays: the walk is short without help)
    base = hix.search_labelset(queries=w["q"], sp=spp, labels=lb, want=want, exclude=ex, k=K, scan_below=BELOW, route=True)
    assert len(set(base[3].tolist())) == 3  # all three routes are in play
    for perm in (np.arange(NQ)[::-1], np.random.default_rng(3).permutation(NQ)):
        got = hix.search_labelset(queries=w["q"][perm], sp=spp, labels=lb, want=[want[i] for i in perm], exclude=ex[perm], k=K,
                                  scan_below=BELOW, route=True)
        same(got, [x[perm] for x in base])
        np.testing.assert_array_equal(got[3], base[3][perm])
    for kv in (dict(PHNSW_LABEL_SLICES="1"), dict(PHNSW_LABEL_SLICES="3"), dict(PHNSW_LABEL_TILE="1")):
        with env(monkeypatch, **kv):
            got = hix.search_labelset(queries=w["q"], sp=spp, labels=lb, want=want, exclude=ex, k=K, scan_below=BELOW, route=True)
        same(got, base)
        np.testing.assert_array_equal(got[3], base[3])


# ---------------------------------------------------------------- 4: the library's own threshold, and always scan
def test_the_scan_default_and_always_scan_are_complete():
    w = world("f32", 24)
    lab, sets, _ = edge_world(w)
    lb = ph.Labels(w["hix"], lab)
    check(w, lab, lb, spread(sets), scan_below=0, routes=False)
    check(w, lab, lb, spread(sets), scan_below=ar.ALWAYS_SCAN, routes=False, stored=(False,))


# ---------------------------------------------------------------- 5: an index over part of its store
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("i8q", 24)])
def test_an_index_over_every_second_vector(kind, dim):
    w = world(kind, dim, 2)
    assert w["n_nodes"] == N // 2
    lab, sets, counts = edge_world(w)
    lb = ph.Labels(w["hix"], lab)
    assert lb.listed <= N // 2
    want = spread(sets)
    np.testing.assert_array_equal(lb.count_sets(want), [counts[i % len(counts)] for i in range(NQ)])
    raw, _ = check(w, lab, lb, want, device=True)
    assert not (raw[0][raw[0] != EMPTY] % 2).any()
    # exclude: odd ids (labelled, not listed: e_q = 0), the entry vector, the nearest candidate
    ex = w["hix"].search_exact_labelset(queries=w["q"], labels=lb, want=want, k=1)[0][:, 0].copy()
    ex[0::3] = np.arange(NQ)[0::3] * 2 + 1
    ex[8::9] = w["entry"]
    check(w, lab, lb, want, exclude=ex, device=True, stored=(False,))


# ---------------------------------------------------------------- 6: the device form on a stream of its own
def test_device_form_on_a_side_stream():
    import torch
    w = world("f32", 24)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    lab, sets, counts = edge_world(w)
    lb = ph.Labels(hix, lab)
    want = spread(sets)
    ex = hix.search_exact_labelset(qids=w["qids"], labels=lb, want=want, k=1)[0][:, 0].copy()
    host = hix.search_labelset(qids=w["qids"], sp=spp, labels=lb, want=want, exclude=ex, k=K, scan_below=BELOW, route=True)
    assert (host[3] != ar.SCAN).any() and (host[3] == ar.SCAN).any()
    stream = torch.cuda.Stream()
    dv = device_sauto(hix, lb, spp, K, qids=w["qids"], want=want, exclude=ex, scan_below=BELOW, stream=stream.cuda_stream)
    assert set(dv[4].tolist()) == {0}
    same(dv, host)
    np.testing.assert_array_equal(dv[3], host[3])
    # a Stored id at or past n: scanned whatever its count, status 4, an empty row; its neighbours are untouched by it
    bad = w["qids"].copy()
    bad[[9, 69]] = [N, 0xFFFFFFF0]  # query 9 wants every label: its count alone would send it to the graph
    dv = device_sauto(hix, lb, spp, K, qids=bad, want=want, exclude=ex, scan_below=BELOW, stream=stream.cuda_stream)
    ok = np.ones(NQ, dtype=bool)
    ok[[9, 69]] = False
    assert (dv[4][~ok] == 4).all() and not dv[4][ok].any() and not dv[2][~ok].any() and (dv[0][~ok] == EMPTY).all()
    assert (dv[3][~ok] == ar.SCAN).all()
    same([x[ok] for x in dv[:3]], [x[ok] for x in host[:3]])
    # Offsets that are not sound.  want_first[29] is pulled back into the range of query 9: query 28 (a count of e: the
    # graph) now runs backwards, and query 29 (every label: the graph) starts inside the range of the LOWER query 9, which
    # keeps its pairs.  The last query ends one past nwant.  Every other query keeps the range it had.
    first, values = ph.hnsw.pack_label_sets(want, NQ)
    f = first.astype(np.int64).copy()
    assert counts[28 % len(counts)] == ar.first_graph_count(SP[0], K, N) and counts[29 % len(counts)] == N
    f[29] = first[9] + 3
    f[NQ] = len(values) + 1
    spoilt = [28, 29, NQ - 1]
    assert f[28] > f[29] and first[9] < f[29] < first[10] and f[30] <= len(values)
    launch, out = staged_labelset(hix, lb, K, f.astype(np.uint32), values, qids=w["qids"],
                                  exclude=np.where(ex < N, ex, 0xFFFFFFFF).astype(np.uint32))
    torch.cuda.synchronize()
    launch()
    exact = fetch(out)  # what phnsw_search_exact_labelset_device reports for the same arrays
    good = np.setdiff1d(np.arange(NQ), spoilt)
    assert (exact[3][spoilt] == 8).all() and not exact[3][good].any()
    dv = device_sauto(hix, lb, spp, K, qids=w["qids"], want=want, exclude=ex, scan_below=BELOW, stream=stream.cuda_stream,
                      first=f.astype(np.uint32))
    np.testing.assert_array_equal(dv[4], exact[3])  # status 8 exactly where the exact call reports it
    assert (dv[3][spoilt] == ar.SCAN).all() and not dv[2][spoilt].any() and (dv[0][spoilt] == EMPTY).all()
    same([x[good] for x in dv[:3]], [x[good] for x in host[:3]])  # the lower query 9 among them: its row is intact
    np.testing.assert_array_equal(dv[3][good], host[3][good])


# ---------------------------------------------------------------- 7: argument checks
def test_argument_checks():
    w = world("f32", 24)
    hix, q = w["hix"], w["q"]
    lab = sized_column([100, 200], 3)
    lb = ph.Labels(hix, lab)
    want = spread([[1, 2], [2]])
    sp = ph.SearchParameters(16, 16, 2)
    for k in (0, 17):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_labelset(queries=q, sp=sp, labels=lb, want=want, k=k)
        assert e.value.code == E_INVALID
        assert str(e.value) == ("phnsw error -1: phnsw_search_labelset_auto: k must be 1..number_of_candidates (got %d, "
                                "number_of_candidates 16)" % k)
        with pytest.raises(ph.PhnswError) as e:
            hix.search_labelset_device(lb, 4, 4, sp, k, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)
        assert e.value.code == E_INVALID and "k must be 1..number_of_candidates" in str(e.value)
    other = ph.Hnsw.from_layers(hix.store, ring(np.arange(N)))  # a handle of another index
    for call in (lambda: other.search_labelset(queries=q, sp=sp, labels=lb, want=want, k=3),
                 lambda: other.search_labelset_device(lb, 4, 4, sp, 3, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == E_INVALID and "the labels are stale" in str(e.value) and "phnsw_search_labelset_auto" in str(e.value)
    # no want_first, want_values null with nwant > 0, both of queries and qids, neither
    for bad in (dict(qids=8, want_values=8), dict(qids=8, want_first=8), dict(queries=16, ldq=24, qids=8, want_first=8, want_values=8),
                dict(want_first=8, want_values=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_labelset_device(lb, 4, 4, sp, 3, 8, 8, 8, 8, **bad)
        assert e.value.code == E_INVALID and "phnsw_search_labelset_auto_device: invalid argument" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:
        hix.search_labelset(qids=np.array([1, N + 5], dtype=np.uint64), sp=sp, labels=lb, want=[[1], [2]], k=3)
    assert e.value.code == E_INVALID and "phnsw_search_labelset_auto: query 1" in str(e.value) and "out of range" in str(e.value)
    ids, d, ln = hix.search_labelset(queries=np.zeros((0, 24), dtype=np.float32), sp=sp, labels=lb, want=[], k=3)
    assert ids.shape == (0, 3)  # nq == 0: a no-op
