"""phnsw_search_filtered_auto[_device]: one filtered call that picks the exact scan or the graph walk per query and
rescans what the walk left short.  Every comparison is on ids, distance bits, lengths and routes, no tolerance anywhere.

Yardsticks, named per assertion below:
  * ROWS    -- the two established calls on the same inputs: search_exact_filtered for a scanned row (routes 1 and 2),
               search_batch_filtered(strict=True) over the whole queue with exclude[q] removed and cut to k for a graph
               row (route 0).  tests/filter_auto_reference.compose puts them together as phnsw.h words the contract
               (pinned on the CPU by tests/test_filter_auto_cpu.py); it also says which graph rows must read 2.
  * ROUTES  -- the rule evaluated in Python integers (filter_auto_reference.rule) from what filter_count reports.
  * COMPLETE-- candidates from tests/exact_filter_reference.candidates: len == min(k, candidates), candidates only.

The worlds are those of tests/test_gpu_exact_filter.py (N = 5000 rows: 157 bitmap words, a ragged last word) with a
built graph over them; 70 queries: more than one wave of ballot lanes, no multiple of 64."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import filter_auto_reference as ar
import filter_reference as fr
from test_gpu_exact_filter import COS, N, NW, ring, rows_of, stores
from test_gpu_i8 import adopt, bits
from test_gpu_i8q import env, lattice_rows

pytestmark = pytest.mark.gpu

NQ = 70
EMPTY = xr.EMPTY
KINDS = [("f32", 24), ("i8q", 24), ("pq", 24), ("f32", 768)]
SP, K, BELOW = (16, 16, 2), 10, 100  # ceil(K * N / 16) = 3125 candidates is where the second rule lets go
E_INVALID, E_UNSUPPORTED = -1, -7


@functools.lru_cache(maxsize=None)
def graph(lattice, dim, every=1):
    full = ph.VectorStore(rows_of(lattice, dim), metric=COS)
    return ph.Hnsw.generate(full, np.arange(0, N, every, dtype=np.uint64), ph.BuildParameters(seed=1))


@functools.lru_cache(maxsize=None)
def world(kind, dim, every=1):
    """store of `kind`, a built graph over every `every`-th row adopted onto it, 70 raw queries, 70 stored ones and each
    raw query's cosine to every row (numpy, for choosing far rows only); made once, changed by no test"""
    store = stores(kind, dim)[1]
    g = graph(kind == "i8q", dim, every)
    hix = g if kind == "f32" and every == 1 else adopt(store, g)
    q = lattice_rows(NQ, dim, 104729 + dim) if kind == "i8q" else oracle.synth_rows(2 ** 32, NQ, dim)[:, :dim].copy()
    qids = (np.arange(NQ, dtype=np.uint64) * 71 + 3) % N
    rows = rows_of(kind == "i8q", dim).astype(np.float64)
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    cos = (q.astype(np.float64) / np.linalg.norm(q, axis=1, keepdims=True)) @ unit.T
    members = None if every == 1 else np.arange(N) % every == 0
    return dict(hix=hix, q=q, qids=qids, cos=cos, members=members, n_nodes=len(range(0, N, every)), entry=g.entry_vector())


def same(a, b):
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(bits(a[1]), bits(b[1]))


def bitmaps(counts, seed, members=None):
    """bool [NQ, N]: query q allows counts[q % len] rows chosen at random among the index's vectors"""
    rng = np.random.default_rng(seed)
    pool = np.arange(N) if members is None else np.nonzero(members)[0]
    allow = np.zeros((NQ, N), dtype=bool)
    for i in range(NQ):
        allow[i, rng.permutation(pool)[:counts[i % len(counts)]]] = True
    return allow


def farthest(w, c):
    """bool [NQ, N]: query q allows the c rows with the smallest cosine to it"""
    allow = np.zeros((NQ, N), dtype=bool)
    for i in range(NQ):
        allow[i, np.argsort(-w["cos"][i], kind="stable")[N - c:]] = True
    return allow


def edge_counts(w, ef=SP[0], k=K):
    e = ar.first_graph_count(ef, k, w["n_nodes"])
    return [0, 1, k - 1, k, BELOW, BELOW + 1, e - 1, e, w["n_nodes"]]


def device_auto(hix, sp, k, queries=None, qids=None, allow=None, exclude=None, scan_below=0, stream=0):
    """phnsw_search_filtered_auto_device with torch buffers -> ids u64, d, len u64, route, status; 64 guard words
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
    words, stride = ph.hnsw.pack_allow(allow, hix.store.n, nq)
    wd = 0 if words is None else up(words, np.int32).data_ptr()
    G = 64
    ids = torch.full((nq * k + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * k + G,), -1.0, dtype=torch.float32, device=dev)
    ln, route, status = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    hix.search_filtered_device(nq, sp, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd, ldq=ld,
                               qids=qi, exclude=ex, allow=wd, allow_stride=stride, scan_below=scan_below,
                               out_route=route.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert (ids[nq * k:] == 7).all() and (d[nq * k:] == -1.0).all()
    for t in (ln, route, status):
        assert (t[nq:] == -1).all()
    i64 = ids[:nq * k].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, k)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return (i64, d[:nq * k].cpu().numpy().reshape(nq, k), ln[:nq].cpu().numpy().view(np.uint32).astype(np.uint64),
            route[:nq].cpu().numpy().view(np.uint32), status[:nq].cpu().numpy())


def check(w, allow=None, exclude=None, k=K, sp=SP, scan_below=BELOW, ref_allow=None, hix=None, device=False, stored=(False, True)):
    """the host form (and the device form) on raw and stored queries against ROWS, ROUTES and COMPLETE.  allow: what
    the call gets; ref_allow: the same as a bool mask where the call gets none (a default filter).  Returns the host
    results."""
    hix = hix or w["hix"]
    spp = ph.SearchParameters(*sp)
    ra = allow if ref_allow is None else ref_allow
    out = []
    for st in stored:
        kw = dict(qids=w["qids"]) if st else dict(queries=w["q"])
        got = hix.search_filtered(sp=spp, allow=allow, exclude=exclude, k=k, scan_below=scan_below, route=True, **kw)
        walk = hix.search_batch_filtered(sp=spp, allow=allow, strict=True, exclude=exclude, **kw)
        scan = hix.search_exact_filtered(allow=allow, exclude=exclude, k=k, **kw)
        want = ar.compose(walk, scan, N, sp[0], k, w["n_nodes"], ra, exclude, w["members"], scan_below)
        print("routes", np.bincount(got[3], minlength=3).tolist(), "expected", np.bincount(want[3], minlength=3).tolist())
        np.testing.assert_array_equal(got[3], want[3])  # ROWS: which graph rows the existing strict call leaves short
        same(got, want)                                  # ROWS
        counts = hix.filter_count(ra if allow is None and ref_allow is not None else allow)
        per_query = ra is not None and np.ndim(ra) == 2
        for i in range(NQ):                              # ROUTES
            r = ar.rule(counts[i] if per_query else counts, scan_below, sp[0], k, w["n_nodes"], per_query)
            assert got[3][i] == r or (got[3][i] == ar.GRAPH_THEN_SCAN and r == ar.GRAPH), (i, got[3][i], r)
        ar.assert_complete(got, N, k, ra, exclude, w["members"])  # COMPLETE
        if device:
            dv = device_auto(hix, spp, k, allow=allow, exclude=exclude, scan_below=scan_below, **kw)
            assert not dv[4].any()
            same(dv, got)
            np.testing.assert_array_equal(dv[3], got[3])
        out.append(got)
    return out


def best_ids(w, allow, stored):
    """each query's nearest candidate: an id that matters when it is excluded"""
    kw = dict(qids=w["qids"]) if stored else dict(queries=w["q"])
    return w["hix"].search_exact_filtered(allow=allow, k=1, **kw)[0][:, 0].copy()


# ---------------------------------------------------------------- 1: routes and rows
@pytest.mark.parametrize("kind,dim", KINDS)
def test_routes_follow_the_rule_and_rows_are_the_established_calls(kind, dim):
    w = world(kind, dim)
    allow = bitmaps(edge_counts(w), 17 + dim)
    raw, st = check(w, allow=allow, device=True)
    for got in (raw, st):
        assert (got[3][:6] == ar.SCAN).all() and (got[3][6] == ar.SCAN) and (got[3][7:9] != ar.SCAN).all()
        assert (got[3][8::9] == ar.GRAPH).all()  # every vector allowed: the walk fills its row
    # exclude: each query's nearest candidate (EMPTY where there is none, which excludes nothing); the queries that
    # allow every vector exclude the index's entry vector instead -- allowed, and the walk hands it back
    for stored in (False, True):
        ex = best_ids(w, allow, stored)
        ex[8::9] = w["entry"]
        got = check(w, allow=allow, exclude=ex, device=True, stored=(stored,))[0]
        assert not ((got[0] == ex[:, None]) & (ex[:, None] != EMPTY)).any()
        assert (got[3][8::9] == ar.GRAPH).all() and (got[2][8::9] == K).all()


@pytest.mark.parametrize("kind,dim", KINDS)
def test_shared_bitmaps_the_default_filter_and_no_filter(kind, dim):
    import torch
    w = world(kind, dim)
    hix = w["hix"]
    lo, hi = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    rng = np.random.default_rng(5)
    lo[rng.permutation(N)[:BELOW]] = True
    hi[rng.permutation(N)[:4000]] = True
    raw, _ = check(w, allow=lo, device=True)
    assert (raw[3] == ar.SCAN).all()
    raw, _ = check(w, allow=hi, device=True)
    assert (raw[3] != ar.SCAN).all() and (raw[3] == ar.GRAPH).sum() > NQ // 2
    lo[rng.permutation(N)[:1]] = True  # BELOW + 1 candidates (or BELOW): the first rule lets go, the second holds on
    assert (check(w, allow=lo)[0][3] == ar.SCAN).all()
    raw, _ = check(w, allow=None, device=True)  # no filter at all: every vector of the index
    assert (raw[3] == ar.GRAPH).all() and (raw[2] == K).all()
    assert (check(w, allow=None, scan_below=ar.ALWAYS_SCAN)[0][3] == ar.SCAN).all()
    assert (check(w, allow=None, scan_below=0)[0][3] == ar.SCAN).all()  # the default: 5000 <= 13 000
    words = torch.from_numpy(fr.pack(hi).view(np.int32)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    hix.set_filter(words.data_ptr())
    try:
        raw, _ = check(w, allow=None, ref_allow=hi, device=True)
        assert (raw[3] != ar.SCAN).all()
        assert (check(w, allow=lo)[0][3] == ar.SCAN).all()  # an explicit filter wins
    finally:
        hix.set_filter(0)


def test_wider_queues_and_other_k():
    w = world("f32", 24)
    for sp, k in (((200, 200, 2), 10), ((64, 32, 2), 64), ((1024, 300, 2), 1)):
        check(w, allow=bitmaps(edge_counts(w, sp[0], k), 23 + k), sp=sp, k=k, device=sp[0] == 200)
    words = np.full((NQ, NW + 3), 0xFFFFFFFF, dtype=np.uint32)  # a wide stride, garbage between and past the bitmaps
    allow = bitmaps(edge_counts(w), 29)
    words[:, :NW] = fr.pack(allow)
    words[:, NW - 1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    check(w, allow=words, ref_allow=allow, device=True)


# ---------------------------------------------------------------- 2: the fallback
@pytest.mark.parametrize("kind,dim", KINDS)
def test_the_fallback_really_runs(kind, dim):
    """Every query allows the ceil(K * N / 16) + 64 rows FARTHEST from it (numpy, on the store's rows): the rule says
    graph, and a walk towards the query ends among rows it may not return.  What the walk's upper layers pass on can
    still fill a row, so the precondition -- the existing strict call returns fewer than K -- is asserted for the batch
    (some query is short) and query by query decides which rows must read 2."""
    w = world(kind, dim)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    c = ar.first_graph_count(SP[0], K, N) + 64
    allow = farthest(w, c)
    assert (allow.sum(axis=1) == c).all() and ar.rule(c, BELOW, SP[0], K, N) == ar.GRAPH
    strict = hix.search_batch_filtered(queries=w["q"], sp=spp, allow=allow, strict=True)
    short = strict[2] < K
    print("strict graph rows shorter than k:", int(short.sum()), "of", NQ, "lengths", strict[2].tolist())
    assert short.any()  # the precondition, on the parent's code
    got = check(w, allow=allow, device=True, stored=(False,))[0]
    np.testing.assert_array_equal(got[3] == ar.GRAPH_THEN_SCAN, short)
    assert (got[3][~short] == ar.GRAPH).all()
    same([x[short] for x in got[:3]], [x[short] for x in hix.search_exact_filtered(queries=w["q"], allow=allow, k=K)])
    assert (got[2] == K).all()


# ---------------------------------------------------------------- 3: processing order, slices
@pytest.mark.parametrize("kind,dim", KINDS)
def test_results_do_not_depend_on_the_order_of_the_batch_or_the_slices(monkeypatch, kind, dim):
    w = world(kind, dim)
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    allow = bitmaps(edge_counts(w), 41 + dim)
    allow[60:] = farthest(w, ar.first_graph_count(SP[0], K, N) + 64)[60:]  # rows the walk leaves short
    ex = best_ids(w, allow, False)
    base = hix.search_filtered(queries=w["q"], sp=spp, allow=allow, exclude=ex, k=K, scan_below=BELOW, route=True)
    assert len(set(base[3].tolist())) == 3  # all three routes are in play
    for perm in (np.arange(NQ)[::-1], np.random.default_rng(3).permutation(NQ)):
        got = hix.search_filtered(queries=w["q"][perm], sp=spp, allow=allow[perm], exclude=ex[perm], k=K, scan_below=BELOW,
                                  route=True)
        same(got, [x[perm] for x in base])
        np.testing.assert_array_equal(got[3], base[3][perm])
    for slices in ("1", "3"):
        with env(monkeypatch, PHNSW_EXACT_SLICES=slices):
            got = hix.search_filtered(queries=w["q"], sp=spp, allow=allow, exclude=ex, k=K, scan_below=BELOW, route=True)
        same(got, base)
        np.testing.assert_array_equal(got[3], base[3])


# ---------------------------------------------------------------- 4: an index over part of its store
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("i8q", 24)])
def test_an_index_over_every_second_vector(kind, dim):
    w = world(kind, dim, 2)
    assert w["n_nodes"] == N // 2 and ar.first_graph_count(SP[0], K, w["n_nodes"]) == 1563
    allow = bitmaps(edge_counts(w), 53, members=w["members"])
    allow[:, 1::2] |= np.random.default_rng(7).random((NQ, N // 2)) < 0.5  # bits of vectors the index does not hold
    raw, _ = check(w, allow=allow, device=True)
    assert not (raw[0][raw[0] != EMPTY] % 2).any()
    # exclude: odd ids (no candidates: e_q = 0), the entry vector, the nearest candidate
    ex = best_ids(w, allow, False)
    ex[0::3] = np.arange(NQ)[0::3] * 2 + 1
    ex[8::9] = w["entry"]
    check(w, allow=allow, exclude=ex, device=True, stored=(False,))
    raw, _ = check(w, allow=None)
    assert (raw[3] == ar.GRAPH).all() and (raw[2] == K).all()


# ---------------------------------------------------------------- 5: the device form on a stream of its own
def test_device_form_on_a_side_stream():
    import torch
    w = world("f32", 24)
    spp = ph.SearchParameters(*SP)
    allow = bitmaps(edge_counts(w), 61)
    ex = best_ids(w, allow, True)
    host = w["hix"].search_filtered(qids=w["qids"], sp=spp, allow=allow, exclude=ex, k=K, scan_below=BELOW, route=True)
    stream = torch.cuda.Stream()
    dv = device_auto(w["hix"], spp, K, qids=w["qids"], allow=allow, exclude=ex, scan_below=BELOW, stream=stream.cuda_stream)
    assert set(dv[4].tolist()) == {0}
    same(dv, host)
    np.testing.assert_array_equal(dv[3], host[3])
    # a Stored id at or past n: scanned whatever its count, status 4, an empty row; its neighbours are untouched by it
    bad = w["qids"].copy()
    bad[[5, 69]] = [N, 0xFFFFFFF0]
    dv = device_auto(w["hix"], spp, K, qids=bad, allow=allow, exclude=ex, scan_below=BELOW, stream=stream.cuda_stream)
    ok = np.ones(NQ, dtype=bool)
    ok[[5, 69]] = False
    assert (dv[4][~ok] == 4).all() and not dv[4][ok].any() and not dv[2][~ok].any() and (dv[0][~ok] == EMPTY).all()
    assert (dv[3][~ok] == ar.SCAN).all()
    same([x[ok] for x in dv[:3]], [x[ok] for x in host[:3]])


# ---------------------------------------------------------------- 6: argument checks
def test_argument_checks():
    w = world("f32", 24)
    hix, q = w["hix"], w["q"]
    sp = ph.SearchParameters(16, 16, 2)
    for k in (0, 17):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_filtered(queries=q, sp=sp, k=k)
        assert e.value.code == E_INVALID
        assert str(e.value) == ("phnsw error -1: phnsw_search_filtered_auto: k must be 1..number_of_candidates (got %d, "
                                "number_of_candidates 16)" % k)
        with pytest.raises(ph.PhnswError) as e:
            hix.search_filtered_device(4, sp, k, 8, 8, 8, 8, qids=8)
        assert e.value.code == E_INVALID
    with pytest.raises(ph.PhnswError) as e:  # number_of_candidates past 1024
        hix.search_filtered(queries=q, sp=ph.SearchParameters(1025, 16, 2), k=1025)
    assert e.value.code == E_INVALID
    with pytest.raises(ph.PhnswError) as e:  # queries and qids
        hix.search_filtered(queries=q, qids=w["qids"], sp=sp, k=3)
    assert e.value.code == E_INVALID
    with pytest.raises(ph.PhnswError) as e:  # neither
        hix.search_filtered_device(4, sp, 3, 8, 8, 8, 8)
    assert e.value.code == E_INVALID
    with pytest.raises(ph.PhnswError) as e:  # a stride below ceil(n / 32) that is not 0
        hix.search_filtered_device(NQ, sp, 3, 8, 8, 8, 8, qids=8, allow=8, allow_stride=NW - 1)
    assert e.value.code == E_INVALID
    ids, d, ln = hix.search_filtered(queries=np.zeros((0, 24), dtype=np.float32), sp=sp, k=3)  # nq == 0: a no-op
    assert ids.shape == (0, 3)
    rows = oracle.synth_rows(0, 400, 32)[:, :32].copy()
    f2 = ph.VectorStore(rows, metric=ph.METRIC_L2)
    shared = ph.SharedPqStore(f2, 16, 100, seed=3, centroid_bp=ph.BuildParameters(seed=2),
                              quantized_search=ph.SearchParameters(32, 32, 2))
    six = ph.Hnsw.from_layers(shared, ring(np.arange(400)))
    with pytest.raises(ph.PhnswError) as e:
        six.search_filtered(queries=rows[:2], sp=sp, k=3)
    assert e.value.code == E_UNSUPPORTED
    assert str(e.value) == ("phnsw error -7: phnsw_search_filtered_auto: not supported over a shared-codebook PQ store; use "
                            "its reconstruction store")
