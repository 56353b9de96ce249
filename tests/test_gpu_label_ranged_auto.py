"""phnsw_search_label_ranged_auto[_device]: one call by a row label and a numeric range that picks the span scan or the
walk per query and rescans what the walk left short.  Every comparison is on ids, distance bits, lengths, routes and
statuses, no tolerance anywhere.

Yardsticks, named per assertion below:
  * ROWS    -- tests/filter_auto_reference.compose of the two established BITMAP calls (search_batch_filtered strict,
               search_exact_filtered) over tests/label_ranged_reference.masks_of(labels, keys, want, lo, hi): masks the
               code under test never saw; and the routed bitmap call search_filtered itself over those masks with the
               same scan_below.
  * ROUTES  -- filter_auto_reference.rule evaluated on LabeledAttribute.count(want, lo, hi).
  * COMPLETE-- filter_auto_reference.assert_complete: len == min(k, candidates - e), candidates only.

The world is that of tests/test_gpu_ranged_auto.py (N = 5000, 70 queries) and so is the key column: the rows FARTHEST
from one query take the first FAR ranks, the others follow in a random order, 50 rows carry no value; keys are
10 * rank.  The ranked column is split over two labels: the ranks below SPLIT = e + 275 carry LA = 9, the others
LB = 0x80000009 (e = the first count the second rule routes to the graph).  Under LA the counts sit on the rule's upper
edge (e - 1 rows: scan, e rows: graph) and the far rows are one span; under LB, which holds fewer than e rows, they sit
on its lower edge (BELOW and BELOW + 1) and every query is scanned; a range across the border holds rows of both."""
import functools

import numpy as np
import pytest

import parallel_hnsw_amd as ph

import filter_auto_reference as ar
import label_ranged_reference as lr
from test_gpu_exact_filter import ring
from test_gpu_filter_auto import BELOW, EMPTY, K, KINDS, N, NQ, SP, same, world
from test_gpu_i8q import env
from test_gpu_labeled_auto import FAR, far_query
from test_gpu_ranged_auto import NMISSING, ranked_column, span, values_of

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
LA, LB = 9, 0x80000009
E_INVALID = -1


def split_of(n_nodes=N, ef=SP[0], k=K):
    return ar.first_graph_count(ef, k, n_nodes) + 275


def labels_of(keys, split):
    """u32 labels [N]: LA for the ranks below `split` (and for the rows without a value, which no span holds), LB above"""
    return np.where((keys != NONE) & (keys // 10 >= split), np.uint32(LB), np.uint32(LA)).astype(np.uint32)


def labeled_attribute(hix, labels, keys):
    return ph.LabeledAttribute(hix, labels, values_of(np.where(keys == NONE, 0, keys)), missing=keys == NONE)


@functools.lru_cache(maxsize=None)
def far_columns(kind, dim):
    j, far = far_query(kind, dim)
    keys = ranked_column(far, 21)
    labels = labels_of(keys, split_of())
    keys.setflags(write=False), labels.setflags(write=False)
    return j, labels, keys, labeled_attribute(world(kind, dim)["hix"], labels, keys)


def edge_pairs(listed, ef=SP[0], k=K, n_nodes=N):
    """(want, lo, hi): under LA spans of 0, 1, k - 1, k, BELOW, BELOW + 1, e - 1 and e rows and the whole label without an
    upper end; under LB spans of 0, 1, k, BELOW and BELOW + 1 rows and the whole label; a range across the border under
    either label; a label nobody carries and NONE"""
    e, split = ar.first_graph_count(ef, k, n_nodes), split_of(n_nodes, ef, k)
    assert 200 + e <= split and split + 200 + BELOW + 1 <= listed < split + e
    out = [(LA,) + span(200, c) for c in (0, 1, k - 1, k, BELOW, BELOW + 1, e - 1, e)] + [(LA, 0, NONE)]
    out += [(LB,) + span(split + 200, c) for c in (0, 1, k, BELOW, BELOW + 1)] + [(LB, 0, NONE)]
    out += [(LA,) + span(split - 60, 200), (LB,) + span(split - 60, 200), (LA + 1, 0, NONE), (NONE, 0, NONE)]
    return out


def spread(pairs):
    return tuple(np.array([pairs[i % len(pairs)][j] for i in range(NQ)], dtype=np.uint32) for j in range(3))


def device_auto(hix, at, sp, k, want, lo, hi, queries=None, qids=None, exclude=None, scan_below=0, stream=0):
    """phnsw_search_label_ranged_auto_device with torch buffers -> ids u64, d, len u64, route, status; 64 guard words
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
    wd, lod, hid = (up(np.asarray(x, dtype=np.uint32), np.int32).data_ptr() for x in (want, lo, hi))
    G = 64
    ids = torch.full((nq * k + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * k + G,), -1.0, dtype=torch.float32, device=dev)
    ln, route, status = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    hix.search_label_ranged_device(at, nq, sp, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd,
                                   ldq=ld, qids=qi, exclude=ex, want=wd, lo=lod, hi=hid, scan_below=scan_below,
                                   out_route=route.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert (ids[nq * k:] == 7).all() and (d[nq * k:] == -1.0).all()
    for t in (ln, route, status):
        assert (t[nq:] == -1).all()
    i64 = ids[:nq * k].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, k)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return (i64, d[:nq * k].cpu().numpy().reshape(nq, k), ln[:nq].cpu().numpy().view(np.uint32).astype(np.uint64),
            route[:nq].cpu().numpy().view(np.uint32), status[:nq].cpu().numpy())


def check(w, cols, at, want, lo, hi, exclude=None, k=K, sp=SP, scan_below=BELOW, device=False, stored=(False, True), q=None,
          routes=True):
    """the host form (and the device form) on raw and stored queries against ROWS, ROUTES and COMPLETE; routes=False
    (the library's own scan_below): COMPLETE and the routed bitmap call's rows only.  Returns the host results."""
    hix = w["hix"]
    spp = ph.SearchParameters(*sp)
    masks = lr.masks_of(cols[0], cols[1], want, lo, hi)
    vlo, vhi = values_of(lo), values_of(hi)
    out = []
    for st in stored:
        kw = dict(qids=w["qids"]) if st else dict(queries=w["q"] if q is None else q)
        got = hix.search_label_ranged(sp=spp, attr=at, want=want, lo=vlo, hi=vhi, exclude=exclude, k=k, scan_below=scan_below,
                                      route=True, **kw)
        ar.assert_complete(got, N, k, masks, exclude, w["members"])  # COMPLETE
        same(got, hix.search_filtered(sp=spp, allow=masks, exclude=exclude, k=k, scan_below=scan_below, **kw))  # ROWS
        if routes:
            walk = hix.search_batch_filtered(sp=spp, allow=masks, strict=True, exclude=exclude, **kw)
            scan = hix.search_exact_filtered(allow=masks, exclude=exclude, k=k, **kw)
            ref = ar.compose(walk, scan, N, sp[0], k, w["n_nodes"], masks, exclude, w["members"], scan_below)
            print("routes", np.bincount(got[3], minlength=3).tolist(), "expected", np.bincount(ref[3], minlength=3).tolist())
            np.testing.assert_array_equal(got[3], ref[3])  # ROWS: which graph rows the strict bitmap call leaves short
            same(got, ref)                                  # ROWS
            counts = at.count(want, vlo, vhi)
            for i in range(NQ):                             # ROUTES
                r = ar.rule(counts[i], scan_below, sp[0], k, w["n_nodes"])
                assert got[3][i] == r or (got[3][i] == ar.GRAPH_THEN_SCAN and r == ar.GRAPH), (i, got[3][i], r)
        if device:
            dv = device_auto(hix, at, spp, k, want, lo, hi, exclude=exclude, scan_below=scan_below, **kw)
            assert not dv[4].any()
            same(dv, got)
            np.testing.assert_array_equal(dv[3], got[3])
        out.append(got)
    return out


# ---------------------------------------------------------------- 1: routes and rows on the rule's edges
@pytest.mark.parametrize("kind,dim", KINDS)
def test_routes_follow_the_rule_and_rows_are_the_established_calls(kind, dim):
    w = world(kind, dim)
    j, labels, keys, at = far_columns(kind, dim)
    listed, split = N - NMISSING, split_of()
    assert at.info() == (N, listed, 2, split)
    e = ar.first_graph_count(SP[0], K, N)
    want, lo, hi = spread(edge_pairs(listed))
    raw, st = check(w, (labels, keys), at, want, lo, hi, device=True)
    counts = at.count(want, values_of(lo), values_of(hi))
    seen = {}
    for got in (raw, st):
        for lbl, c, r in zip(want.tolist(), counts.tolist(), got[3].tolist()):
            seen.setdefault((lbl, c), set()).add(r)
    assert sorted(c for lbl, c in seen if lbl == LA) == sorted([0, 1, K - 1, K, BELOW, BELOW + 1, e - 1, e, split, 60])
    assert sorted(c for lbl, c in seen if lbl == LB) == sorted([0, 1, K, BELOW, BELOW + 1, listed - split, 140])
    for key, routes in seen.items():  # both edges of the rule: BELOW | BELOW + 1 scan by its two halves, e - 1 | e part
        assert (routes == {ar.SCAN}) == (key[1] < e), (key, routes)
    assert ar.SCAN not in seen[(LA, e)] and ar.SCAN not in seen[(LA, split)] and seen[(LA, e - 1)] == {ar.SCAN}
    # exclude INSIDE the span: each query's nearest candidate (EMPTY where there is none); every third query the entry
    # vector, every fifth a row without a value -- OUTSIDE every span
    ex = w["hix"].search_exact_label_ranged(queries=w["q"], attr=at, want=want, lo=values_of(lo), hi=values_of(hi), k=1)[0][:, 0].copy()
    inside = ex != EMPTY
    ex[2::3] = w["entry"]
    ex[4::5] = int(np.nonzero(keys == NONE)[0][0])
    got = check(w, (labels, keys), at, want, lo, hi, exclude=ex, device=True, stored=(False,))[0]
    assert not ((got[0] == ex[:, None]) & (ex[:, None] != EMPTY)).any()
    masks = lr.masks_of(labels, keys, want, lo, hi)
    e_q = np.array([ex[i] != EMPTY and masks[i, int(ex[i])] for i in range(NQ)])
    assert (e_q & inside).any() and (~e_q & (ex != EMPTY)).any()
    np.testing.assert_array_equal(got[2], np.minimum(K, masks.sum(1) - e_q))  # out_len == min(k, c - e)


def test_scan_below_values_and_wider_queues():
    w = world("f32", 24)
    j, labels, keys, at = far_columns("f32", 24)
    want, lo, hi = spread(edge_pairs(N - NMISSING))
    want[j], (lo[j], hi[j]) = LA, span(0, FAR)  # the far rows hold ranks 0 ..: the walk of their query over them is short
    seen = set()
    for below in (1, 2000, ar.ALWAYS_SCAN):
        got = check(w, (labels, keys), at, want, lo, hi, scan_below=below, stored=(False,))[0]
        seen |= set(got[3].tolist())
    assert seen == {ar.GRAPH, ar.SCAN, ar.GRAPH_THEN_SCAN}
    check(w, (labels, keys), at, want, lo, hi, scan_below=0, routes=False)  # the library's own threshold: complete rows


# ---------------------------------------------------------------- 2: the fallback
@pytest.mark.parametrize("kind,dim", KINDS)
def test_the_fallback_really_runs(kind, dim):
    """The FAR rows farthest from one query (far_query) hold the first FAR ranks, all under LA; that query, copied to
    five places of the batch, wants exactly them: the rule says graph, and a walk towards the query ends among rows it
    may not return.  The precondition -- the strict bitmap call returns fewer than K -- is asserted.  The other queries
    want BELOW rows of LB."""
    w = world(kind, dim)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    j, labels, keys, at = far_columns(kind, dim)
    assert ar.rule(FAR, BELOW, SP[0], K, N) == ar.GRAPH and FAR <= split_of()
    copies = [0, 7, 33, 64, 69]
    q = w["q"].copy()
    q[copies] = w["q"][j]
    want, lo, hi = spread([(LB,) + span(split_of() + 100, BELOW)])
    want[copies] = LA
    lo[copies], hi[copies] = span(0, FAR)
    assert at.count(want, values_of(lo), values_of(hi))[copies].tolist() == [FAR] * 5
    masks = lr.masks_of(labels, keys, want, lo, hi)
    strict = hix.search_batch_filtered(queries=q, sp=spp, allow=masks, strict=True)
    assert (strict[2] < K)[copies].all()  # the precondition, on the established call
    got = check(w, (labels, keys), at, want, lo, hi, device=True, stored=(False,), q=q)[0]
    np.testing.assert_array_equal(np.nonzero(got[3] == ar.GRAPH_THEN_SCAN)[0], copies)  # left short by the walk
    assert (np.delete(got[3], copies) == ar.SCAN).all()
    short = got[3] == ar.GRAPH_THEN_SCAN
    scan = hix.search_exact_label_ranged(queries=q, attr=at, want=want, lo=values_of(lo), hi=values_of(hi), k=K)
    same([x[short] for x in got[:3]], [x[short] for x in scan])  # those rows are the scan's
    assert (got[2] == K).all()


# ---------------------------------------------------------------- 3: the order of the batch, the scan's knob
def test_results_do_not_depend_on_the_order_of_the_batch_or_the_slices(monkeypatch):
    w = world("f32", 24)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    j, labels, keys, at = far_columns("f32", 24)
    want, lo, hi = spread([(LA,) + span(0, FAR), (LB,) + span(split_of() + 100, BELOW), (LA,) + span(FAR - 300, K - 1),
                           (LA,) + span(9, 0), (LB, 0, NONE), (NONE, 0, NONE)])
    want[j], (lo[j], hi[j]) = LA, span(0, FAR)
    vlo, vhi = values_of(lo), values_of(hi)
    ex = hix.search_exact_label_ranged(queries=w["q"], attr=at, want=want, lo=vlo, hi=vhi, k=1)[0][:, 0].copy()
    ex[j] = EMPTY  # (its nearest candidate stays: the walk is short without help)
    a = dict(sp=spp, attr=at, k=K, scan_below=BELOW, route=True)
    base = hix.search_label_ranged(queries=w["q"], want=want, lo=vlo, hi=vhi, exclude=ex, **a)
    assert len(set(base[3].tolist())) == 3  # all three routes are in play
    for perm in (np.arange(NQ)[::-1], np.random.default_rng(3).permutation(NQ)):
        got = hix.search_label_ranged(queries=w["q"][perm], want=want[perm], lo=vlo[perm], hi=vhi[perm], exclude=ex[perm], **a)
        same(got, [x[perm] for x in base])
        np.testing.assert_array_equal(got[3], base[3][perm])
    for slices in ("1", "3"):
        with env(monkeypatch, PHNSW_LABEL_RANGE_SLICES=slices):
            got = hix.search_label_ranged(queries=w["q"], want=want, lo=vlo, hi=vhi, exclude=ex, **a)
        same(got, base)
        np.testing.assert_array_equal(got[3], base[3])


# ---------------------------------------------------------------- 4: an index over part of its store
def test_an_index_over_every_second_vector():
    w = world("f32", 24, 2)
    assert w["n_nodes"] == N // 2
    keys = ranked_column([], 31, members=w["members"])
    split = split_of(w["n_nodes"])
    labels = labels_of(keys, split)  # the odd rows carry labels and values too: unlisted
    at = labeled_attribute(w["hix"], labels, keys)
    listed = N // 2 - NMISSING
    assert at.info() == (N, listed, 2, split) and listed < int((keys != NONE).sum())
    want, lo, hi = spread(edge_pairs(listed, n_nodes=w["n_nodes"]))
    raw, _ = check(w, (labels, keys), at, want, lo, hi, device=True)
    assert not (raw[0][raw[0] != EMPTY] % 2).any()
    # exclude: odd ids (they carry labels and values and are not listed: e_q = 0), the entry vector, the nearest candidate
    ex = w["hix"].search_exact_label_ranged(queries=w["q"], attr=at, want=want, lo=values_of(lo), hi=values_of(hi), k=1)[0][:, 0].copy()
    ex[0::3] = np.arange(NQ)[0::3] * 2 + 1
    ex[8::9] = w["entry"]
    check(w, (labels, keys), at, want, lo, hi, exclude=ex, device=True, stored=(False,))


# ---------------------------------------------------------------- 5: the device form on a stream of its own
def test_device_form_on_a_side_stream():
    import torch
    w = world("f32", 24)
    spp = ph.SearchParameters(*SP)
    j, labels, keys, at = far_columns("f32", 24)
    e = ar.first_graph_count(SP[0], K, N)
    want, lo, hi = spread([(LA,) + span(200, e), (LB,) + span(split_of() + 100, 300), (LA,) + span(9, 0), (NONE, NONE, NONE)])
    vlo, vhi = values_of(lo), values_of(hi)
    ex = w["hix"].search_exact_label_ranged(qids=w["qids"], attr=at, want=want, lo=vlo, hi=vhi, k=1)[0][:, 0].copy()
    host = w["hix"].search_label_ranged(qids=w["qids"], sp=spp, attr=at, want=want, lo=vlo, hi=vhi, exclude=ex, k=K,
                                        scan_below=BELOW, route=True)
    assert (host[3] != ar.SCAN).any() and (host[3] == ar.SCAN).any()
    stream = torch.cuda.Stream()
    dv = device_auto(w["hix"], at, spp, K, want, lo, hi, qids=w["qids"], exclude=ex, scan_below=BELOW, stream=stream.cuda_stream)
    assert set(dv[4].tolist()) == {0}
    same(dv, host)
    np.testing.assert_array_equal(dv[3], host[3])
    # a Stored id at or past n: scanned whatever its count, status 4, an empty row; its neighbours are untouched by it
    bad = w["qids"].copy()
    bad[[4, 69]] = [N, 0xFFFFFFF0]
    dv = device_auto(w["hix"], at, spp, K, want, lo, hi, qids=bad, exclude=ex, scan_below=BELOW, stream=stream.cuda_stream)
    ok = np.ones(NQ, dtype=bool)
    ok[[4, 69]] = False
    assert (dv[4][~ok] == 4).all() and not dv[4][ok].any() and not dv[2][~ok].any() and (dv[0][~ok] == EMPTY).all()
    assert (dv[3][~ok] == ar.SCAN).all()
    same([x[ok] for x in dv[:3]], [x[ok] for x in host[:3]])


# ---------------------------------------------------------------- 6: argument checks
def test_argument_checks():
    w = world("f32", 24)
    hix, q = w["hix"], w["q"]
    j, labels, keys, at = far_columns("f32", 24)
    sp = ph.SearchParameters(16, 16, 2)
    for k in (0, 17):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_label_ranged(queries=q, sp=sp, attr=at, want=LA, lo=0, hi=50, k=k)
        assert str(e.value) == ("phnsw error -1: phnsw_search_label_ranged_auto: k must be 1..number_of_candidates (got %d, "
                                "number_of_candidates 16)" % k)
        with pytest.raises(ph.PhnswError) as e:
            hix.search_label_ranged_device(at, 4, sp, k, 8, 8, 8, 8, qids=8, want=8, lo=8, hi=8)
        assert e.value.code == E_INVALID and "k must be 1..number_of_candidates" in str(e.value)
    other = ph.Hnsw.from_layers(hix.store, ring(np.arange(N)))  # a handle of another index
    for call in (lambda: other.search_label_ranged(queries=q, sp=sp, attr=at, want=LA, lo=0, hi=50, k=3),
                 lambda: other.search_label_ranged_device(at, 4, sp, 3, 8, 8, 8, 8, qids=8, want=8, lo=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == E_INVALID and "are stale" in str(e.value) and "phnsw_search_label_ranged_auto" in str(e.value)
    for bad in (dict(qids=8, want=8, lo=8), dict(qids=8, lo=8, hi=8), dict(queries=16, ldq=24, qids=8, want=8, lo=8, hi=8),
                dict(want=8, lo=8, hi=8)):  # no hi, no want, both kinds of query, neither
        with pytest.raises(ph.PhnswError) as e:
            hix.search_label_ranged_device(at, 4, sp, 3, 8, 8, 8, 8, **bad)
        assert e.value.code == E_INVALID and "phnsw_search_label_ranged_auto_device: invalid argument" in str(e.value)
    ids, d, ln = hix.search_label_ranged(queries=np.zeros((0, 24), dtype=np.float32), sp=sp, attr=at, want=LA, lo=0, hi=5, k=3)
    assert ids.shape == (0, 3)  # nq == 0: a no-op
