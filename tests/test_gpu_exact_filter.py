"""The exact top-k over an allow-list (phnsw_search_exact_filtered[_device], phnsw_filter_count_device): a scan of the
allowed rows instead of the graph search.  Every comparison is on ids, distance bits and lengths, no tolerance anywhere.

Yardstick: tests/exact_filter_reference.py (a stable sort on (D, id), pinned by tests/test_exact_filter_cpu.py) over a
distance matrix that the code under test did not make -- the oracle's ORC_SUM_BLOCKED64 distances over store.read() for
the row stores (lattice rows on i8q, where the oracle's f32 sums equal the integer arithmetic), and compare_vec
(phnsw_distance_batch, unchanged code) on the same store for PQ.

N = 5000 rows: 157 bitmap words, so three passes of 64 words with a ragged last one, n no multiple of 32, and -- with 16
queries -- three slices per query by default.  40 copies of one row are spread over the id range, so ties cross pass and
slice borders.  The scan never walks the graph, so the indexes are adopted one-layer rings; the two tests that need a
built graph build one over the 24-component rows."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import filter_reference as fr
from test_gpu_i8 import bits, oracle_over
from test_gpu_i8q import env, lattice_rows

pytestmark = pytest.mark.gpu

N, NW = 5000, 157
NQ, NS = 16, 8
COS = oracle.METRIC_COSINE_HALF
EMPTY = xr.EMPTY
DUPS = np.linspace(0, N - 1, 40).astype(np.int64)  # ids of the 40 copies of row 0: first and last id among them
PQ_M = {24: 12, 300: 60, 768: 64}                  # sub-spaces of the PQ worlds (tables of 12, 60 and 64 KiB)
KINDS = [(k, d) for k in ("f32", "f16", "i8", "i8q", "pq") for d in (24, 300, 768)] + [("f32", 1536)]
SMALL = [(k, 24) for k in ("f32", "f16", "i8", "i8q", "pq")]
assert (N + 31) // 32 == NW and N % 32 and NW % 64


def ring(nodes):
    """one layer over `nodes` (VectorIds, ascending): node i linked to its two neighbours on a ring"""
    n = len(nodes)
    nb = np.stack([(np.arange(n) + 1) % n, (np.arange(n) + n - 1) % n], axis=1).astype(np.uint64)
    return [(np.asarray(nodes, dtype=np.uint64), nb)]


@functools.lru_cache(maxsize=None)
def rows_of(lattice, dim):
    rows = lattice_rows(N, dim, 7919 + dim) if lattice else oracle.synth_rows(0, N, dim)[:, :dim].copy()
    rows[DUPS] = rows[0]
    return rows


@functools.lru_cache(maxsize=None)
def stores(kind, dim):
    full = ph.VectorStore(rows_of(kind == "i8q", dim), metric=COS)
    store = {"f32": lambda f: f, "f16": ph.F16Store.from_full, "i8": ph.I8Store.from_full, "i8q": ph.I8QStore.from_full,
             "pq": lambda f: ph.PqStore(f, PQ_M[dim])}[kind](full)
    return full, store


@functools.lru_cache(maxsize=None)
def world(kind, dim):
    """store of `kind`, an index over all of it, 16 raw and 8 stored queries and the yardstick's distance of each to
    every row; made once per (kind, dim), changed by no test"""
    store = stores(kind, dim)[1]
    q = lattice_rows(NQ, dim, 104729 + dim) if kind == "i8q" else oracle.synth_rows(2 ** 32, NQ, dim)[:, :dim].copy()
    q[0] = rows_of(kind == "i8q", dim)[0]  # the duplicated row itself: 40 candidates tie for the first place
    qids = np.array([int(DUPS[3]), 1, 77, 2047, 2048, 4095, 4096, N - 1], dtype=np.uint64)
    if kind == "pq":
        every = np.arange(N, dtype=np.uint64)
        Dq = np.stack([store.compare_vec(ph.Unstored(np.ascontiguousarray(v)), every) for v in q])
        Ds = np.stack([store.compare_vec(ph.Stored(int(v)), every) for v in qids])
    else:
        oix = oracle_over(store, COS)
        Dq = fr.distance_rows(oix, queries=q, mode=oracle.SUM_BLOCKED64)
        Ds = fr.distance_rows(oix, qids=qids, mode=oracle.SUM_BLOCKED64)
    return dict(store=store, hix=ph.Hnsw.from_layers(store, ring(np.arange(N))), q=q, qids=qids, Dq=Dq, Ds=Ds)


def mask(density, shape, seed):
    return np.random.default_rng(seed).random(shape) < density


def same(a, b):
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(bits(a[1]), bits(b[1]))


def device_exact(hix, k, queries=None, qids=None, allow=None, exclude=None, stream=0):
    """phnsw_search_exact_filtered_device with torch buffers -> ids u64, d, len u64, status"""
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
        ex = up(np.asarray(exclude, dtype=np.uint32), np.int32).data_ptr()
    words, stride = ph.hnsw.pack_allow(allow, hix.store.n, nq)
    wd = 0 if words is None else up(words, np.int32).data_ptr()
    ids = torch.full((nq, k), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev)
    ln = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    status = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    hix.search_exact_filtered_device(nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd, ldq=ld,
                                     qids=qi, exclude=ex, allow=wd, allow_stride=stride, stream=stream)
    torch.cuda.synchronize()
    i64 = ids.cpu().numpy().view(np.uint32).astype(np.uint64)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return i64, d.cpu().numpy(), ln.cpu().numpy().view(np.uint32).astype(np.uint64), status.cpu().numpy()


def check(w, allow=None, exclude=None, k=10, members=None, hix=None, ref_allow=None, device=True):
    """raw and stored queries, host and device form, against the restatement.  allow: what the call gets (a bool mask or
    packed words); ref_allow: the same as a bool mask when `allow` is packed.  Per-query arrays have NQ rows; the stored
    queries use the first NS.  Returns the host results (raw, stored)."""
    hix = hix or w["hix"]
    out = []
    for kw, D in ((dict(queries=w["q"]), w["Dq"]), (dict(qids=w["qids"]), w["Ds"])):
        nq = len(D)
        a, ra = (None if x is None else (x if np.ndim(x) == 1 else x[:nq]) for x in (allow, allow if ref_allow is None else ref_allow))
        e = None if exclude is None else exclude[:nq]
        ref = xr.exact_topk(D, ra, e, members, k)
        got = hix.search_exact_filtered(allow=a, exclude=e, k=k, **kw)
        same(got, ref)
        assert (got[0][np.arange(k)[None, :] >= got[2][:, None]] == EMPTY).all()
        if device:
            dv = device_exact(hix, k, allow=a, exclude=e, **kw)
            assert not dv[3].any()
            same(dv, ref)
        out.append(got)
    return out


# ---------------------------------------------------------------- 1: the bitmaps
@pytest.mark.parametrize("kind,dim", KINDS)
def test_bitmaps(kind, dim):
    w = world(kind, dim)
    for density in (0.5, 0.01):
        raw, _ = check(w, allow=mask(density, N, int(density * 1000) + dim))
        assert (raw[2] == 10).all()
    check(w, allow=np.ones(N, dtype=bool))
    check(w, allow=None)  # no filter and no default set: every vector of the index
    raw, st = check(w, allow=np.zeros(N, dtype=bool))
    assert not raw[2].any() and not st[2].any() and (bits(raw[1]) == bits(xr.FMAX)).all()
    for v in (0, 2047, 2048, N - 1):  # a single bit: first, either side of a pass border, last
        one = np.zeros(N, dtype=bool)
        one[v] = True
        raw, _ = check(w, allow=one, device=v == N - 1)
        assert (raw[2] == 1).all() and (raw[0][:, 0] == v).all()
    last = np.zeros(N, dtype=bool)
    last[(NW - 1) * 32:] = True  # bits of the last word only
    raw, _ = check(w, allow=last)
    assert (raw[2] == N - (NW - 1) * 32).all()


@pytest.mark.parametrize("kind,dim", KINDS)
def test_per_query_bitmaps_strides_and_garbage_past_n(kind, dim):
    w = world(kind, dim)
    per_q = mask(0.02, (NQ, N), 31 + dim)
    check(w, allow=per_q)
    words = fr.pack(per_q)
    assert words.shape == (NQ, NW)
    dirty = words.copy()
    dirty[:, -1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)  # bits at and past n in the packed words
    check(w, allow=dirty, ref_allow=per_q)
    wide = np.full((NQ, NW + 3), 0xFFFFFFFF, dtype=np.uint32)  # stride nw + 3, the words between the bitmaps all ones
    wide[:, :NW] = dirty
    check(w, allow=wide, ref_allow=per_q)
    shared = mask(0.3, N, 5)
    sw = fr.pack(shared)
    sw[-1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    check(w, allow=sw, ref_allow=shared)


# ---------------------------------------------------------------- 2: exclude, k, ties
@pytest.mark.parametrize("kind,dim", KINDS)
def test_exclude_and_k(kind, dim):
    w = world(kind, dim)
    allow = mask(0.1, N, 77 + dim)  # about 500 candidates: fewer than 1024
    assert 300 < allow.sum() < 1024
    first = check(w, allow=allow, k=1)
    ex = np.concatenate([first[0][0][:, 0], first[1][0][:, 0]])  # each query's best: an allowed id, and it matters
    for which, e in ((0, ex[:NQ]), (1, ex[NQ:])):
        kw = dict(queries=w["q"]) if which == 0 else dict(qids=w["qids"])
        D = w["Dq"] if which == 0 else w["Ds"]
        got = w["hix"].search_exact_filtered(allow=allow, exclude=e, k=10, **kw)
        same(got, xr.exact_topk(D, allow, e, None, 10))
        assert (got[0][:, 0] != e).all() and not (got[0] == e[:, None]).any()
        dv = device_exact(w["hix"], 10, allow=allow, exclude=e, **kw)
        assert not dv[3].any()
        same(dv, got)
    raw, st = check(w, allow=allow, k=1024)
    assert (raw[2] == allow.sum()).all() and (st[2] == allow.sum()).all()
    raw, _ = check(w, allow=mask(0.5, N, 3), k=1024)  # more candidates than k: the full list is merged into over and over
    assert (raw[2] == 1024).all()
    check(w, allow=None, k=64, exclude=np.full(NQ, EMPTY, dtype=np.uint64))  # PHNSW_EMPTY excludes nothing


@pytest.mark.parametrize("kind,dim", KINDS)
def test_duplicate_rows_come_out_in_id_order(kind, dim):
    w = world(kind, dim)

    def copies_are_one_run(got, copies):
        """the copies of one row share one distance: in a result they form one run, ascending by id"""
        for i in range(len(got[0])):
            at = np.nonzero(np.isin(got[0][i], copies.astype(np.uint64)))[0]
            assert len(at) == len(copies) and (np.diff(at) == 1).all()
            np.testing.assert_array_equal(got[0][i, at], copies.astype(np.uint64))
            assert len(set(bits(got[1][i, at]).tolist())) == 1

    some = mask(0.04, N, 17)
    some[DUPS] = True  # the 40 copies, spread over all three passes and slices, among about 200 other rows
    raw, st = check(w, allow=some, k=1024)
    copies_are_one_run(raw, DUPS)
    copies_are_one_run(st, DUPS)
    if kind != "i8q":  # normalised rows: nothing is nearer to a row than its copies (lattice rows differ in length)
        first = check(w, allow=None, k=64)
        for got in first:  # query 0 is the duplicated row, stored query 0 one of its copies
            np.testing.assert_array_equal(got[0][0, :40], DUPS.astype(np.uint64))
    half = np.zeros(N, dtype=bool)
    half[DUPS[::2]] = True
    half[DUPS[1] + 1:DUPS[1] + 300] = True
    raw, st = check(w, allow=half, k=1024)
    kept = DUPS[half[DUPS]]  # every second copy, and the one inside the allowed run
    assert len(kept) == 21
    copies_are_one_run(raw, kept)
    copies_are_one_run(st, kept)


# ---------------------------------------------------------------- 3: an index over part of its store
@pytest.mark.parametrize("kind,dim", SMALL + [("f32", 768)])
def test_vectors_outside_the_index_are_never_returned(kind, dim):
    w = world(kind, dim)
    allow = mask(0.5, N, 11)
    even = np.arange(N) % 2 == 0
    hix = ph.Hnsw.from_layers(w["store"], ring(np.arange(0, N, 2)))  # every second vector: VectorId != NodeId
    raw, _ = check(w, allow=allow, members=even, hix=hix, k=100)
    assert not (raw[0][raw[0] != EMPTY] % 2).any()
    check(w, allow=None, members=even, hix=hix, k=1024)
    assert hix.filter_count(allow) == np.count_nonzero(allow & even) and hix.filter_count(None) == N // 2
    head = np.arange(N) < N - 100
    hix = ph.Hnsw.from_layers(w["store"], ring(np.arange(N - 100)))  # the first N - 100: identity, shorter than the store
    raw, _ = check(w, allow=np.ones(N, dtype=bool), members=head, hix=hix, k=1024, exclude=np.full(NQ, N - 50, dtype=np.uint64))
    assert (raw[0][raw[0] != EMPTY] < N - 100).all()
    assert hix.filter_count(np.ones(N, dtype=bool)) == N - 100


def test_an_index_built_over_every_second_vector():
    w = world("f32", 24)
    g = ph.Hnsw.generate(stores("f32", 24)[0], np.arange(0, N, 2, dtype=np.uint64), ph.BuildParameters(seed=1))
    allow = mask(0.05, N, 13)
    raw, _ = check(w, allow=allow, members=np.arange(N) % 2 == 0, hix=g, k=50)
    assert (raw[2] == 50).all() and not (raw[0] % 2).any()


# ---------------------------------------------------------------- 4: the default filter
def test_the_default_filter_serves_calls_that_pass_none():
    import torch
    w = world("f32", 300)
    hix = w["hix"]
    allow = mask(0.03, N, 99)
    words = torch.from_numpy(fr.pack(allow).view(np.int32)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    hix.set_filter(words.data_ptr())
    try:
        check(w, allow=None, ref_allow=allow)
        assert hix.filter_count(None) == np.count_nonzero(allow)
        other = mask(0.5, N, 100)
        check(w, allow=other)  # an explicit filter wins
    finally:
        hix.set_filter(0)
    check(w, allow=None)


# ---------------------------------------------------------------- 5: the slice count changes nothing
@pytest.mark.parametrize("kind,dim", KINDS)
def test_results_do_not_depend_on_the_slices(monkeypatch, kind, dim):
    w = world(kind, dim)
    shared, per_q = mask(0.2, N, 1), mask(0.01, (NQ, N), 2)
    ex = np.array([np.nonzero(per_q[i])[0][i % 3] for i in range(NQ)], dtype=np.uint64)
    base = [check(w, allow=shared, k=1024), check(w, allow=per_q, exclude=ex, k=10), check(w, allow=None, k=64)]
    for slices in ("1", "2", "3", "1000"):  # 1000: clamped to the three passes there are
        with env(monkeypatch, PHNSW_EXACT_SLICES=slices):
            now = [check(w, allow=shared, k=1024), check(w, allow=per_q, exclude=ex, k=10), check(w, allow=None, k=64)]
        for a, b in zip(base, now):
            same(a[0], b[0])
            same(a[1], b[1])


# ---------------------------------------------------------------- 6: the count
@pytest.mark.parametrize("kind,dim", SMALL)
def test_filter_count(kind, dim):
    hix = world(kind, dim)["hix"]
    for density in (0.5, 0.01, 0.0, 1.0):
        a = mask(density, N, 5 + int(density * 100))
        assert hix.filter_count(a) == np.count_nonzero(a)
    per_q = mask(0.1, (NQ, N), 8)
    np.testing.assert_array_equal(hix.filter_count(per_q), np.count_nonzero(per_q, axis=1))
    wide = np.full((NQ, NW + 3), 0xFFFFFFFF, dtype=np.uint32)  # garbage past n and between the bitmaps is not counted
    wide[:, :NW] = fr.pack(per_q)
    wide[:, NW - 1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    np.testing.assert_array_equal(hix.filter_count(wide), np.count_nonzero(per_q, axis=1))
    assert hix.filter_count(None) == N


# ---------------------------------------------------------------- 7: argument checks
def test_argument_checks():
    w = world("f32", 24)
    hix, q = w["hix"], w["q"]
    for k in (0, 1025):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_filtered(queries=q, k=k)
        assert e.value.code == -1  # PHNSW_E_INVALID
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_filtered: k must be 1..1024 (got %d)" % k
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_filtered_device(4, k, 8, 8, 8, 8, qids=8)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_filtered_device: k must be 1..1024 (got %d)" % k
    with pytest.raises(ph.PhnswError) as e:  # a stride below ceil(n / 32) that is not 0
        hix.search_exact_filtered_device(NQ, 3, 8, 8, 8, 8, qids=8, allow=8, allow_stride=NW - 1)
    assert e.value.code == -1
    with pytest.raises(ph.PhnswError) as e:  # queries and qids
        hix.search_exact_filtered_device(NQ, 3, 8, 8, 8, 8, queries=16, ldq=24, qids=8)
    assert e.value.code == -1
    ids, d, ln = hix.search_exact_filtered(queries=np.zeros((0, 24), dtype=np.float32), k=3)  # nq == 0: a no-op
    assert ids.shape == (0, 3)
    # a shared-codebook PQ store: unsupported, as for the distance batch
    rows = oracle.synth_rows(0, 400, 32)[:, :32].copy()
    f2 = ph.VectorStore(rows, metric=ph.METRIC_L2)
    shared = ph.SharedPqStore(f2, 16, 100, seed=3, centroid_bp=ph.BuildParameters(seed=2),
                              quantized_search=ph.SearchParameters(32, 32, 2))
    six = ph.Hnsw.from_layers(shared, ring(np.arange(400)))
    with pytest.raises(ph.PhnswError) as e:
        six.search_exact_filtered(queries=rows[:2], k=3)
    assert e.value.code == -7  # PHNSW_E_UNSUPPORTED
    assert str(e.value) == ("phnsw error -7: phnsw_search_exact_filtered: not supported over a shared-codebook PQ store; "
                            "use its reconstruction store")


# ---------------------------------------------------------------- 8: recall 1 where the graph search runs dry
def test_recall_one_at_a_selective_filter():
    w = world("f32", 24)
    g = ph.Hnsw.generate(stores("f32", 24)[0], np.arange(N, dtype=np.uint64), ph.BuildParameters(seed=1))
    allow = mask(0.01, N, 2024)
    exact = check(w, allow=allow, k=10, hix=g)[0]
    assert (exact[2] == 10).all()  # the full k, whatever the density
    every = g.search_exact_filtered(queries=w["q"], allow=allow, k=1024)  # all candidates with their distances
    graph = g.search_batch_filtered(queries=w["q"], sp=ph.SearchParameters(300, 300, 2), allow=allow, strict=True)
    print("graph search, ef 300, density 0.01: results per query", graph[2].tolist())
    for i in range(NQ):
        cand = {int(v): b for v, b in zip(every[0][i, :int(every[2][i])], bits(every[1][i]))}
        assert len(cand) == np.count_nonzero(allow)
        for v, b in zip(graph[0][i, :int(graph[2][i])], bits(graph[1][i])):
            assert int(v) in cand and cand[int(v)] == b
