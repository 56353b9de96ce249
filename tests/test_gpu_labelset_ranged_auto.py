"""phnsw_search_labelset_ranged_auto[_device]: one call by a SET of row labels and a numeric range that picks the span
scan or the walk per query and rescans what the walk left short.  Every comparison is on ids, distance bits, lengths,
routes and statuses, no tolerance anywhere.

The yardstick is the routed BITMAP call, search_filtered, over tests/labelset_ranged_reference.masks_of(labels, keys,
sets, lo, hi) -- masks the code under test never saw -- at the same scan_below: rows, lengths and routes must be equal.
COMPLETE is filter_auto_reference.assert_complete: len == min(k, candidates - e), candidates only.

The world is that of tests/test_gpu_filter_auto.py (N = 5000, 70 queries, number_of_candidates 16, k = 10: the second
rule routes to the graph from e = 3125 candidates on) and the key column that of tests/test_gpu_ranged_auto.py: the FAR
rows FARTHEST from one query (test_gpu_labeled_auto.far_query: its strict walk over them comes back short) take the first
FAR ranks, the others follow in a random order, 50 rows carry no value; keys are 10 * rank.  The seven labels of
tests/test_gpu_exact_labelset_ranged.py are dealt over the ranks; every 37th id that is not one of the far rows carries
no label.  The inputs are chosen on the CPU from the counts of the masks: the set of all seven labels over the far rows
holds FAR >= e rows (graph; short for the far query: graph, then scan), over everything nearly all rows (graph), every
smaller set fewer than e (scan)."""
import functools

import numpy as np
import pytest

import parallel_hnsw_amd as ph

import filter_auto_reference as ar
import labelset_ranged_reference as sr
from test_gpu_exact_filter import ring
from test_gpu_exact_labelset_ranged import LABELS, LONG, NONE, csr, labeled_attribute
from test_gpu_filter_auto import BELOW, EMPTY, K, N, NQ, SP, same, world
from test_gpu_i8 import bits
from test_gpu_i8q import env
from test_gpu_labeled_auto import FAR, far_query
from test_gpu_ranged_auto import NMISSING, ranked_column, span, values_of

pytestmark = pytest.mark.gpu

ALL = list(LABELS)
E = ar.first_graph_count(SP[0], K, N)
E_INVALID = -1


def labels_by_rank(keys, keep):
    """u32 labels [N]: LABELS[rank % 7] by the rank of the key (rows without a value: by id); NONE for every 37th id that is
    not one of `keep`"""
    labels = np.array([LABELS[(int(k) // 10) % 7] if k != NONE else LABELS[v % 7] for v, k in enumerate(keys)], dtype=np.uint32)
    bare = np.arange(len(keys)) % 37 == 5
    bare[np.asarray(keep, dtype=np.int64)] = False
    labels[bare] = NONE
    return labels


@functools.lru_cache(maxsize=None)
def far_columns(kind, dim):
    j, far = far_query(kind, dim)
    keys = ranked_column(far, 21)
    labels = labels_by_rank(keys, far)
    keys.setflags(write=False), labels.setflags(write=False)
    return j, labels, keys, labeled_attribute(world(kind, dim)["hix"], labels, keys)


# (set, lo, hi): what a query wants
WANTS = [(ALL,) + span(0, FAR), (ALL, 0, NONE), (LONG, 0, NONE), ([3, 4], 0, NONE), ([3], ) + span(500, 700), ([], 0, NONE),
         ([NONE, 0x80000000], 0, NONE), ([5], 0, NONE), (ALL, 9000, 3000), (ALL,) + span(FAR + 50, E), ([4, 3, 3],) + span(FAR, 7 * K),
         ([0, 0xFFFFFFFE],) + span(200, 35)]


def spread(wants, j=None):
    """(sets, lo, hi) [NQ]: the queries go round `wants`; query j, the far query, wants all seven labels over the far rows"""
    sets = [wants[i % len(wants)][0] for i in range(NQ)]
    lo = np.array([wants[i % len(wants)][1] for i in range(NQ)], dtype=np.uint32)
    hi = np.array([wants[i % len(wants)][2] for i in range(NQ)], dtype=np.uint32)
    if j is not None:
        sets[j], (lo[j], hi[j]) = ALL, span(0, FAR)
    return sets, lo, hi


def device_auto(hix, at, sp, k, first, values, lo, hi, queries=None, qids=None, exclude=None, scan_below=0, stream=0, nwant=None):
    """phnsw_search_labelset_ranged_auto_device with torch buffers -> ids u64, d, len u64, route, status; 64 guard words
    behind every buffer must come back as they went in"""
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
    fd, lod, hid = (up(np.asarray(x, dtype=np.uint32), np.int32).data_ptr() for x in (first, lo, hi))
    vd = up(np.asarray(values, dtype=np.uint32), np.int32).data_ptr() if len(values) else 0
    G = 64
    ids = torch.full((nq * k + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * k + G,), -1.0, dtype=torch.float32, device=dev)
    ln, route, status = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    hix.search_labelset_ranged_device(at, nq, len(values) if nwant is None else nwant, sp, k, ids.data_ptr(), d.data_ptr(),
                                      ln.data_ptr(), status.data_ptr(), queries=qd, ldq=ld, qids=qi, exclude=ex, want_first=fd,
                                      want_values=vd, lo=lod, hi=hid, scan_below=scan_below, out_route=route.data_ptr(),
                                      stream=stream)
    torch.cuda.synchronize()
    assert (ids[nq * k:] == 7).all() and (d[nq * k:] == -1.0).all()
    for t in (ln, route, status):
        assert (t[nq:] == -1).all()
    i64 = ids[:nq * k].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, k)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return (i64, d[:nq * k].cpu().numpy().reshape(nq, k), ln[:nq].cpu().numpy().view(np.uint32).astype(np.uint64),
            route[:nq].cpu().numpy().view(np.uint32), status[:nq].cpu().numpy())


def check(w, cols, at, sets, lo, hi, exclude=None, k=K, sp=SP, scan_below=BELOW, device=False, stored=(False, True), q=None):
    """the host form (and the device form) on raw and stored queries against the routed bitmap call and COMPLETE.
    Returns (the host results, the reference's) of the last form"""
    hix = w["hix"]
    spp = ph.SearchParameters(*sp)
    masks = sr.masks_of(cols[0], cols[1], sets, lo, hi, w["members"])
    vlo, vhi = values_of(lo), values_of(hi)
    counts = at.count_sets(sets, vlo, vhi)
    np.testing.assert_array_equal(counts, masks.sum(1))
    for st in stored:
        kw = dict(qids=w["qids"]) if st else dict(queries=w["q"] if q is None else q)
        got = hix.search_labelset_ranged(sp=spp, attr=at, want=sets, lo=vlo, hi=vhi, exclude=exclude, k=k, scan_below=scan_below,
                                         route=True, **kw)
        ref = hix.search_filtered(sp=spp, allow=masks, exclude=exclude, k=k, scan_below=scan_below, route=True, **kw)
        same(got, ref)
        np.testing.assert_array_equal(got[3], ref[3])
        ar.assert_complete(got, N, k, masks, exclude, w["members"])  # COMPLETE
        for i in range(NQ):  # the routes follow the rule on the count call's figure
            r = ar.rule(counts[i], scan_below, sp[0], k, w["n_nodes"])
            assert got[3][i] == r or (got[3][i] == ar.GRAPH_THEN_SCAN and r == ar.GRAPH), (i, got[3][i], r)
        if device:
            dv = device_auto(hix, at, spp, k, *csr(sets), lo, hi, exclude=exclude, scan_below=scan_below, **kw)
            assert not dv[4].any()
            same(dv, got)
            np.testing.assert_array_equal(dv[3], got[3])
    return got, ref


# ---------------------------------------------------------------- 1: rows, lengths and routes are the routed bitmap call's
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("i8q", 24), ("pq", 24)])
def test_rows_lengths_and_routes_are_the_routed_bitmap_calls(kind, dim):
    w = world(kind, dim)
    j, labels, keys, at = far_columns(kind, dim)
    listed = (labels != NONE) & (keys != NONE)
    assert at.listed == listed.sum() > E + 1000 and FAR >= E
    sets, lo, hi = spread(WANTS, j)
    counts = sr.masks_of(labels, keys, sets, lo, hi).sum(1)  # the inputs were chosen from these
    assert counts[j] == FAR and sorted(set((counts >= E).tolist())) == [False, True]
    assert (counts == 0).any() and ((counts > 0) & (counts <= BELOW)).any() and ((counts > BELOW) & (counts < E)).any()
    q = w["q"].copy()
    copies = [j, (j + 12) % NQ, (j + 24) % NQ]  # queries that want what the far query wants, and are the far query
    for c in copies:
        q[c] = w["q"][j]
        sets[c], lo[c], hi[c] = sets[j], lo[j], hi[j]
    got, ref = check(w, (labels, keys), at, sets, lo, hi, device=True, stored=(False,), q=q)
    assert set(ref[3].tolist()) == {ar.GRAPH, ar.SCAN, ar.GRAPH_THEN_SCAN}  # the reference call alone shows all three
    assert (ref[3][copies] == ar.GRAPH_THEN_SCAN).all()
    check(w, (labels, keys), at, sets, lo, hi, device=True, stored=(True,))
    # exclude INSIDE the spans: each query's nearest candidate (EMPTY where there is none); every third query the entry
    # vector, every fifth a row without a value -- OUTSIDE every span
    ex = w["hix"].search_exact_labelset_ranged(queries=q, attr=at, want=sets, lo=values_of(lo), hi=values_of(hi), k=1)[0][:, 0].copy()
    inside = ex != EMPTY
    ex[2::3] = w["entry"]
    ex[4::5] = int(np.nonzero(keys == NONE)[0][0])
    got, _ = check(w, (labels, keys), at, sets, lo, hi, exclude=ex, device=True, stored=(False,), q=q)
    assert not ((got[0] == ex[:, None]) & (ex[:, None] != EMPTY)).any()
    masks = sr.masks_of(labels, keys, sets, lo, hi)
    e_q = np.array([ex[i] != EMPTY and masks[i, int(ex[i])] for i in range(NQ)])
    assert (e_q & inside).any() and (~e_q & (ex != EMPTY)).any()
    np.testing.assert_array_equal(got[2], np.minimum(K, masks.sum(1) - e_q))  # out_len == min(k, c - e)


def test_scan_below_values():
    w = world("f32", 24)
    hix = w["hix"]
    j, labels, keys, at = far_columns("f32", 24)
    sets, lo, hi = spread(WANTS, j)
    seen = set()
    for below in (1, 2000, 4000, ar.ALWAYS_SCAN, 0):  # 0: the library's own threshold, 20 000: every query is scanned here
        got, ref = check(w, (labels, keys), at, sets, lo, hi, scan_below=below, stored=(False,))
        seen |= set(ref[3].tolist())
        if below in (ar.ALWAYS_SCAN, 0):
            assert (got[3] == ar.SCAN).all()
            same(got, hix.search_exact_labelset_ranged(queries=w["q"], attr=at, want=sets, lo=values_of(lo), hi=values_of(hi), k=K))
    assert seen == {ar.GRAPH, ar.SCAN, ar.GRAPH_THEN_SCAN}


# ---------------------------------------------------------------- 2: the order of the batch, the scan's knob
def test_results_do_not_depend_on_the_order_of_the_batch_or_the_slices(monkeypatch):
    w = world("f32", 24)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    j, labels, keys, at = far_columns("f32", 24)
    sets, lo, hi = spread(WANTS, j)
    vlo, vhi = values_of(lo), values_of(hi)
    a = dict(sp=spp, attr=at, k=K, scan_below=BELOW, route=True)
    base = hix.search_labelset_ranged(queries=w["q"], want=sets, lo=vlo, hi=vhi, **a)
    assert len(set(base[3].tolist())) == 3  # all three routes are in play
    for perm in (np.arange(NQ)[::-1], np.random.default_rng(3).permutation(NQ)):
        got = hix.search_labelset_ranged(queries=w["q"][perm], want=[sets[i] for i in perm], lo=vlo[perm], hi=vhi[perm], **a)
        same(got, [x[perm] for x in base])
        np.testing.assert_array_equal(got[3], base[3][perm])
    for slices in ("1", "3"):
        with env(monkeypatch, PHNSW_LABELSET_RANGE_SLICES=slices):
            got = hix.search_labelset_ranged(queries=w["q"], want=sets, lo=vlo, hi=vhi, **a)
        same(got, base)
        np.testing.assert_array_equal(got[3], base[3])


# ---------------------------------------------------------------- 3: an index over part of its store
def test_an_index_over_every_second_vector():
    w = world("f32", 24, 2)
    assert w["n_nodes"] == N // 2
    keys = ranked_column([], 31, members=w["members"])
    labels = labels_by_rank(keys, [])  # the odd rows carry labels and values too: unlisted
    at = labeled_attribute(w["hix"], labels, keys)
    e2 = ar.first_graph_count(SP[0], K, w["n_nodes"])
    wants = [(ALL, 0, NONE), (ALL,) + span(100, e2 + 100), ([3, 4], 0, NONE), ([3],) + span(500, 300), ([], 0, NONE), (LONG,) + span(0, 20),
             ([NONE, 5], 0, NONE)]
    sets, lo, hi = spread(wants)
    got, ref = check(w, (labels, keys), at, sets, lo, hi, device=True)
    assert ar.SCAN in ref[3] and (ref[3] != ar.SCAN).any()
    assert not (got[0][got[0] != EMPTY] % 2).any()
    # exclude: odd ids (they carry labels and values and are not listed: e_q = 0), the entry vector, the nearest candidate
    ex = w["hix"].search_exact_labelset_ranged(queries=w["q"], attr=at, want=sets, lo=values_of(lo), hi=values_of(hi), k=1)[0][:, 0].copy()
    ex[0::3] = np.arange(NQ)[0::3] * 2 + 1
    ex[8::9] = w["entry"]
    check(w, (labels, keys), at, sets, lo, hi, exclude=ex, device=True, stored=(False,))


# ---------------------------------------------------------------- 4: the device form: a side stream, offsets, Stored ids
def test_device_form_on_a_side_stream_and_status_8_reads_scan():
    import torch
    w = world("f32", 24)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    j, labels, keys, at = far_columns("f32", 24)
    sets, lo, hi = spread(WANTS, j)
    vlo, vhi = values_of(lo), values_of(hi)
    host = hix.search_labelset_ranged(qids=w["qids"], sp=spp, attr=at, want=sets, lo=vlo, hi=vhi, exclude=w["qids"], k=K,
                                      scan_below=BELOW, route=True)
    assert (host[3] != ar.SCAN).any() and (host[3] == ar.SCAN).any()
    stream = torch.cuda.Stream()
    first, values = csr(sets)
    dv = device_auto(hix, at, spp, K, first, values, lo, hi, qids=w["qids"], exclude=w["qids"], scan_below=BELOW, stream=stream.cuda_stream)
    assert set(dv[4].tolist()) == {0}
    same(dv, host)
    np.testing.assert_array_equal(dv[3], host[3])
    # offsets the call cannot trust.  Queries 3 and 5 want all seven labels over everything (graph, by their counts); then
    # query 4 is made to run backwards and query 5 to start inside query 3's range: status 8, an empty row and
    # PHNSW_ROUTE_SCAN for both, where the exact device form reports it, whatever their counts.  The others are untouched
    sets2 = [list(s) for s in sets]
    for i in (3, 5):
        sets2[i], lo[i], hi[i] = ALL, 0, NONE
    first, values = csr(sets2)
    nwant = len(values)
    bad_first = first.copy()
    bad_first[5] = first[4] - 2  # query 3 keeps [first[3], first[4]); query 4 = [first[4], first[4] - 2); query 5 starts two pairs early
    refused = [4, 5]
    good = np.ones(NQ, dtype=bool)
    good[refused] = False
    ref = hix.search_filtered(queries=w["q"], sp=spp, allow=sr.masks_of(labels, keys, sets2, lo, hi), k=K, scan_below=BELOW, route=True)
    assert ref[3][3] != ar.SCAN and ref[3][5] != ar.SCAN
    ex = device_auto(hix, at, spp, K, bad_first, values, lo, hi, queries=w["q"], scan_below=BELOW, stream=stream.cuda_stream, nwant=nwant)
    assert (ex[4][refused] == 8).all() and not ex[4][good].any()
    assert (ex[3][refused] == ar.SCAN).all() and not ex[2][refused].any() and (ex[0][refused] == EMPTY).all()
    assert (bits(ex[1][refused]) == 0x7F7FFFFF).all()
    same([x[good] for x in ex[:3]], [x[good] for x in ref[:3]])
    np.testing.assert_array_equal(ex[3][good], ref[3][good])
    past = first.copy()
    past[NQ] = nwant + 9              # the last query ends past nwant
    ex = device_auto(hix, at, spp, K, past, values, lo, hi, queries=w["q"], scan_below=BELOW, nwant=nwant)
    assert ex[4][NQ - 1] == 8 and not ex[4][:NQ - 1].any() and ex[3][NQ - 1] == ar.SCAN and not ex[2][NQ - 1]
    # a Stored id at or past n: scanned whatever its count, status 4, an empty row; its neighbours are untouched by it
    bad = w["qids"].copy()
    bad[[4, 69]] = [N, 0xFFFFFFF0]
    first, values = csr(sets)
    lo, hi = spread(WANTS, j)[1:]
    dv = device_auto(hix, at, spp, K, first, values, lo, hi, qids=bad, exclude=w["qids"], scan_below=BELOW, stream=stream.cuda_stream)
    ok = np.ones(NQ, dtype=bool)
    ok[[4, 69]] = False
    assert (dv[4][~ok] == 4).all() and not dv[4][ok].any() and not dv[2][~ok].any() and (dv[0][~ok] == EMPTY).all()
    assert (dv[3][~ok] == ar.SCAN).all()
    same([x[ok] for x in dv[:3]], [x[ok] for x in host[:3]])


# ---------------------------------------------------------------- 5: argument checks
def test_argument_checks():
    w = world("f32", 24)
    hix, q = w["hix"], w["q"][:4]
    j, labels, keys, at = far_columns("f32", 24)
    sp = ph.SearchParameters(16, 16, 2)
    sets = [[3], [3, 4], [], [5]]
    for k in (0, 17):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_labelset_ranged(queries=q, sp=sp, attr=at, want=sets, lo=0, hi=50, k=k)
        assert str(e.value) == ("phnsw error -1: phnsw_search_labelset_ranged_auto: k must be 1..number_of_candidates (got %d, "
                                "number_of_candidates 16)" % k)
        with pytest.raises(ph.PhnswError) as e:
            hix.search_labelset_ranged_device(at, 4, 4, sp, k, 8, 8, 8, 8, qids=8, want_first=8, want_values=8, lo=8, hi=8)
        assert e.value.code == E_INVALID and "k must be 1..number_of_candidates" in str(e.value)
    other = ph.Hnsw.from_layers(hix.store, ring(np.arange(N)))  # a handle of another index
    for call in (lambda: other.search_labelset_ranged(queries=q, sp=sp, attr=at, want=sets, lo=0, hi=50, k=3),
                 lambda: other.search_labelset_ranged_device(at, 4, 4, sp, 3, 8, 8, 8, 8, qids=8, want_first=8, want_values=8, lo=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == E_INVALID and "are stale" in str(e.value) and "phnsw_search_labelset_ranged_auto" in str(e.value)
    for bad in (dict(qids=8, want_first=8, want_values=8, lo=8), dict(qids=8, want_first=8, want_values=8, hi=8), dict(qids=8, want_values=8, lo=8, hi=8),
                dict(qids=8, want_first=8, lo=8, hi=8), dict(queries=16, ldq=24, qids=8, want_first=8, want_values=8, lo=8, hi=8),
                dict(want_first=8, want_values=8, lo=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_labelset_ranged_device(at, 4, 4, sp, 3, 8, 8, 8, 8, **bad)
        assert e.value.code == E_INVALID and "phnsw_search_labelset_ranged_auto_device: invalid argument" in str(e.value)
    ids, d, ln = hix.search_labelset_ranged(queries=np.zeros((0, 24), dtype=np.float32), sp=sp, attr=at, want=[], lo=0, hi=5, k=3)
    assert ids.shape == (0, 3)  # nq == 0: a no-op
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses a Stored query id at or past n, naming the call and the query
        hix.search_labelset_ranged(qids=np.array([1, 2, N, 3], dtype=np.uint64), sp=sp, attr=at, want=sets, lo=0, hi=5, k=3)
    assert "phnsw_search_labelset_ranged_auto: query 2: stored query id %d out of range" % N in str(e.value)
