"""The exact top-k for ONE allow-list shared by the batch, computed as a distance table
(phnsw_search_exact_shared[_device], filter_dense.hip).  Every comparison is on ids, distance bits, lengths and status,
no tolerance anywhere.

Two yardsticks, both for every case: tests/exact_filter_reference.py over the oracle's ORC_SUM_BLOCKED64 distances of
store.read() (lattice rows on i8q), which the code under test did not make, and the existing scan,
search_exact_filtered with one shared bitmap, whose rows the new call promises bit for bit.

The stores are those of tests/test_gpu_exact_filter.py (N = 5000, n no multiple of 32, 40 copies of one row spread over
the id range, one-layer ring indexes) at the dimensions where the table takes another path: 24 (ragged: the vector-unit
tile pass; the int8 GEMM with K zero-padded on i8q), 256 / 768 / 1536 (the matrix cores at NV = 1 / 3 / 6).  Query
counts 16 (below 32: the vector-unit pass even at 256), 40 (32 + 8: a partial position tile) and 65 (one block tile
plus one row); query 0 is the duplicated row, stored query 0 one of its copies, so 40 candidates tie and ids decide."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import filter_reference as fr
from test_gpu_exact_filter import COS, DUPS, EMPTY, N, NW, mask, ring, rows_of, same, stores
from test_gpu_i8 import bits, oracle_over
from test_gpu_i8q import env, lattice_rows

pytestmark = pytest.mark.gpu

NQX = 65
COUNTS = (16, 40, 65)
KINDS = [(k, d) for k in ("f32", "f16", "i8", "i8q") for d in (24, 256)] + [("f32", 768), ("i8q", 768), ("f32", 1536)]


@functools.lru_cache(maxsize=None)
def sworld(kind, dim, metric=COS):
    """store of `kind`, a ring index over all of it, 65 raw and 65 stored queries and the yardstick's distance of each
    to every row; made once per (kind, dim, metric), changed by no test"""
    if metric == COS:
        store = stores(kind, dim)[1]
    else:
        assert kind == "f32"
        store = ph.VectorStore(rows_of(False, dim), metric=metric)
    q = lattice_rows(NQX, dim, 15485863 + dim) if kind == "i8q" else oracle.synth_rows(2 ** 33, NQX, dim)[:, :dim].copy()
    q[0] = rows_of(kind == "i8q", dim)[0]
    qids = np.concatenate([[int(DUPS[3])], np.linspace(1, N - 1, NQX - 1).astype(np.int64)]).astype(np.uint64)
    oix = oracle_over(store, metric)
    Dq = fr.distance_rows(oix, queries=q, mode=oracle.SUM_BLOCKED64)
    Ds = fr.distance_rows(oix, qids=qids, mode=oracle.SUM_BLOCKED64)
    return dict(store=store, hix=ph.Hnsw.from_layers(store, ring(np.arange(N))), q=q, qids=qids, Dq=Dq, Ds=Ds)


def exactly(count, seed, with_dups=True):
    """a mask with exactly `count` candidates, copies of the duplicated row first (as many as fit)"""
    m = np.zeros(N, dtype=bool)
    take = DUPS[:min(count, 8)] if with_dups else DUPS[:0]
    m[take] = True
    perm = np.random.default_rng(seed).permutation(N)
    rest = perm[~np.isin(perm, take)][:count - len(take)]
    m[rest] = True
    assert m.sum() == count
    return m


def device_shared(hix, k, queries=None, qids=None, allow=None, exclude=None, stream=None, sync=True):
    """phnsw_search_exact_shared_device with torch buffers -> ids u64, d, len u64, status (or the tensors, sync=False)"""
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
    assert stride == 0
    wd = 0 if words is None else up(words, np.int32).data_ptr()
    ids = torch.full((nq, k), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev)
    ln = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    status = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    hix.search_exact_shared_device(nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd, ldq=ld,
                                   qids=qi, exclude=ex, allow=wd, stream=0 if stream is None else stream.cuda_stream)
    out = (ids, d, ln, status, keep)
    return fetch(out) if sync else out


def fetch(out):
    import torch
    torch.cuda.synchronize()
    ids, d, ln, status, _ = out
    i64 = ids.cpu().numpy().view(np.uint32).astype(np.uint64)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return i64, d.cpu().numpy(), ln.cpu().numpy().view(np.uint32).astype(np.uint64), status.cpu().numpy()


def check(w, nq=16, allow=None, exclude=None, k=10, members=None, hix=None, ref_allow=None, device=True, forms=(0, 1)):
    """raw (0) and stored (1) queries, host and device form, against both yardsticks.  allow: what the call gets (a bool
    mask or packed words); ref_allow: the same as a bool mask when `allow` is packed or None with a default filter.
    Per-query arrays have NQX rows.  Returns the host results by form."""
    hix = hix or w["hix"]
    out = {}
    for form in forms:
        kw, D = (dict(queries=w["q"][:nq]), w["Dq"][:nq]) if form == 0 else (dict(qids=w["qids"][:nq]), w["Ds"][:nq])
        e = None if exclude is None else exclude[:nq]
        ref = xr.exact_topk(D, allow if ref_allow is None else ref_allow, e, members, k)
        got = hix.search_exact_shared(allow=allow, exclude=e, k=k, **kw)
        same(got, ref)
        same(got, hix.search_exact_filtered(allow=allow, exclude=e, k=k, **kw))
        assert (got[0][np.arange(k)[None, :] >= got[2][:, None]] == EMPTY).all()
        assert (bits(got[1])[np.arange(k)[None, :] >= got[2][:, None]] == bits(xr.FMAX)).all()
        if device:
            dv = device_shared(hix, k, allow=allow, exclude=e, **kw)
            assert not dv[3].any()
            same(dv, ref)
        out[form] = got
    return out


# ---------------------------------------------------------------- 1: kinds x dimensions x query counts
@pytest.mark.parametrize("kind,dim", KINDS)
def test_kinds_dimensions_and_query_counts(kind, dim):
    w = sworld(kind, dim)
    allow = mask(0.3, N, 41 + dim)  # about 1500 candidates
    allow[DUPS] = True
    for nq in COUNTS:
        got = check(w, nq=nq, allow=allow, k=64, device=nq == 40)
        if kind != "i8q":  # normalised rows: nothing is nearer to a row than its copies (lattice rows differ in length)
            for form in (0, 1):  # query 0 is the duplicated row, stored query 0 one of its copies
                np.testing.assert_array_equal(got[form][0][0, :40], DUPS.astype(np.uint64))
    some = mask(0.04, N, 17)
    some[DUPS] = True  # the 40 copies among about 200 other rows, every candidate returned: the copies tie, ids decide
    got = check(w, nq=40, allow=some, k=1024, device=False)
    for form in (0, 1):
        for i in range(40):
            at = np.nonzero(np.isin(got[form][0][i], DUPS.astype(np.uint64)))[0]
            assert len(at) == 40 and (np.diff(at) == 1).all()
            np.testing.assert_array_equal(got[form][0][i, at], DUPS.astype(np.uint64))
            assert len(set(bits(got[form][1][i, at]).tolist())) == 1


@pytest.mark.parametrize("metric", [oracle.METRIC_L2, oracle.METRIC_ONE_MINUS_DOT])
def test_the_other_metrics_on_the_vector_unit_pass(metric):
    w = sworld("f32", 24, metric)
    allow = mask(0.3, N, 7)
    allow[DUPS] = True
    for nq in (16, 65):
        check(w, nq=nq, allow=allow, k=64)


# ---------------------------------------------------------------- 2: candidate counts at tile and chunk edges
@pytest.mark.parametrize("kind,dim,nq", [("f32", 24, 16), ("f32", 256, 40), ("i8q", 256, 40), ("f16", 256, 65)])
def test_candidate_counts_at_the_tile_edges(kind, dim, nq):
    w = sworld(kind, dim)
    for count in (0, 1, 63, 64, 65):
        got = check(w, nq=nq, allow=exactly(count, 100 + count), k=100, device=count in (0, 65))
        for form in (0, 1):
            assert (got[form][2] == count).all()
    got = check(w, nq=nq, allow=np.ones(N, dtype=bool), k=10)  # all rows
    assert (got[0][2] == 10).all()


def test_the_node_chunk_edge_and_equal_rows_across_chunkings(monkeypatch):
    w = sworld("f32", 256)
    dense = mask(0.3, N, 5)
    dense[DUPS] = True  # ties that cross chunk borders: the copies are spread over the id range
    cases = [(exactly(192, 1), 1024), (exactly(193, 2), 1024), (dense, 1024), (dense, 10)]
    base = [check(w, nq=40, allow=a, k=k) for a, k in cases]
    for nodes in ("64", "192", "100"):  # 100: not a multiple of 64, rounded up to 128
        with env(monkeypatch, PHNSW_DENSE_NODES=nodes):
            now = [check(w, nq=40, allow=a, k=k, device=nodes == "192") for a, k in cases]
        for a, b in zip(base, now):
            same(a[0], b[0])
            same(a[1], b[1])
    assert (base[0][0][2] == 192).all() and (base[1][1][2] == 193).all()


@pytest.mark.parametrize("kind,dim", [("f32", 256), ("i8q", 24), ("i8", 24)])
def test_position_chunks(monkeypatch, kind, dim):
    w = sworld(kind, dim)
    allow = mask(0.3, N, 9)
    allow[DUPS] = True
    base = check(w, nq=65, allow=allow, k=100)
    stride = (min(int(allow.sum()), 8192) + 63) // 64 * 64
    # 65 queries in three position chunks: 32 + 32 + 1 (matrix cores, then the vector units) and 22 + 22 + 21
    for positions in (32, 22):
        with env(monkeypatch, PHNSW_DENSE_TABLE_BYTES=str(stride * 4 * positions)):
            now = check(w, nq=65, allow=allow, k=100)
        for form in (0, 1):
            same(base[form], now[form])
    with env(monkeypatch, PHNSW_DENSE_TABLE_BYTES="1", PHNSW_DENSE_NODES="192"):  # one position per table, eight node chunks
        now = check(w, nq=16, allow=allow, k=100, device=False)
    for form in (0, 1):
        same(tuple(x[:16] for x in base[form]), now[form])


def test_the_default_filter_and_no_filter():
    import torch
    w = sworld("f32", 256)
    hix = w["hix"]
    allow = mask(0.03, N, 99)
    words = torch.from_numpy(fr.pack(allow).view(np.int32)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    check(w, nq=40, allow=None, k=10)  # no filter and no default set: every vector of the index
    hix.set_filter(words.data_ptr())
    try:
        check(w, nq=40, allow=None, ref_allow=allow)
        check(w, nq=40, allow=mask(0.5, N, 100))  # an explicit filter wins
    finally:
        hix.set_filter(0)
    check(w, nq=40, allow=None, k=10)
    dirty = fr.pack(allow)
    dirty[-1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)  # bits at and past n in the packed words
    assert dirty.shape == (NW,)
    check(w, nq=40, allow=dirty, ref_allow=allow)


# ---------------------------------------------------------------- 3: k, exclude
@pytest.mark.parametrize("kind,dim,nq", [("f32", 256, 40), ("i8q", 24, 16), ("f32", 768, 65)])
def test_k_values(kind, dim, nq):
    w = sworld(kind, dim)
    some = mask(0.1, N, 77)  # about 500 candidates: fewer than 1024
    assert 300 < some.sum() < 1024
    for k in (1, 10, 100, 1024):
        got = check(w, nq=nq, allow=some, k=k, device=k in (1, 1024))
        assert (got[0][2] == min(k, some.sum())).all() and (got[1][2] == min(k, some.sum())).all()
    got = check(w, nq=nq, allow=mask(0.5, N, 3), k=1024, device=False)  # more candidates than k
    assert (got[0][2] == 1024).all()


@pytest.mark.parametrize("kind,dim,nq", [("f32", 256, 40), ("f16", 24, 16)])
def test_exclude(kind, dim, nq):
    w = sworld(kind, dim)
    allow = mask(0.1, N, 78)
    first = check(w, nq=nq, allow=allow, k=1, device=False)
    inside, outside = np.nonzero(allow)[0], np.nonzero(~allow)[0]
    for form in (0, 1):
        best = first[form][0][:, 0]  # each query's best hit: an allowed id, and it matters
        ex = np.full(NQX, EMPTY, dtype=np.uint64)
        ex[:nq] = best
        got = check(w, nq=nq, allow=allow, exclude=ex, k=10, forms=(form,))[form]
        assert (got[0][:, 0] != best).all() and not (got[0] == best[:, None]).any()
    mixed = np.full(NQX, EMPTY, dtype=np.uint64)  # a candidate, a non-candidate, PHNSW_EMPTY, an id past n, in turn
    mixed[0::4], mixed[1::4], mixed[3::4] = inside[5], outside[5], N + 7
    got = check(w, nq=nq, allow=allow, exclude=mixed, k=1024)
    for form in (0, 1):
        np.testing.assert_array_equal(got[form][2], allow.sum() - (np.arange(nq) % 4 == 0))


# ---------------------------------------------------------------- 4: an index over part of its store
@pytest.mark.parametrize("kind,dim,nq", [("f32", 24, 16), ("f32", 256, 40), ("i8q", 256, 40)])
def test_vectors_outside_the_index_are_never_candidates(kind, dim, nq):
    w = sworld(kind, dim)
    allow = mask(0.5, N, 11)
    even = np.arange(N) % 2 == 0
    hix = ph.Hnsw.from_layers(w["store"], ring(np.arange(0, N, 2)))  # every second vector: vec2node is not the identity
    got = check(w, nq=nq, allow=allow, members=even, hix=hix, k=100, exclude=np.full(NQX, EMPTY, dtype=np.uint64))
    assert not (got[0][0][got[0][0] != EMPTY] % 2).any()
    got = check(w, nq=nq, allow=None, members=even, hix=hix, k=1024, device=False)
    assert (got[0][2] == 1024).all()
    head = np.arange(N) < N - 100
    hix = ph.Hnsw.from_layers(w["store"], ring(np.arange(N - 100)))  # the first N - 100: identity, shorter than the store
    got = check(w, nq=nq, allow=np.ones(N, dtype=bool), members=head, hix=hix, k=1024, device=False)
    assert (got[0][0][got[0][0] != EMPTY] < N - 100).all()


# ---------------------------------------------------------------- 5: the device form
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("f32", 24), ("i8q", 256)])
def test_a_stored_query_id_past_n_is_reported_and_harms_nobody(kind, dim):
    w = sworld(kind, dim)
    allow = mask(0.3, N, 21)
    qids = w["qids"][:40].copy()
    bad = [3, 17, 39]
    qids[bad] = [N, N + 12345, 0xFFFFFFFE]
    dv = device_shared(w["hix"], 10, qids=qids, allow=allow)
    ref = xr.exact_topk(w["Ds"][:40], allow, None, None, 10)
    good = np.setdiff1d(np.arange(40), bad)
    same(tuple(x[good] for x in dv[:3]), tuple(x[good] for x in ref))
    assert (dv[3][bad] == 4).all() and not dv[3][good].any()
    assert (dv[0][bad] == EMPTY).all() and (bits(dv[1][bad]) == bits(xr.FMAX)).all() and not dv[2][bad].any()
    # the scan reports the same for the same arguments
    from test_gpu_exact_filter import device_exact
    sc = device_exact(w["hix"], 10, qids=qids, allow=allow)
    same(dv, sc)
    np.testing.assert_array_equal(dv[3], sc[3])
    none = device_shared(w["hix"], 10, qids=qids, allow=np.zeros(N, dtype=bool))  # no candidate at all: the same report
    assert (none[3][bad] == 4).all() and not none[3][good].any() and not none[2].any()


def test_a_refused_query_carried_through_three_node_chunks(monkeypatch):
    """The refusal word of the select is the status itself.  130 candidates in node chunks of 64 are three chunks, so
    the refused query's key list is stored empty, reloaded twice and written by a chunk that is not the first."""
    w = sworld("f32", 256)
    allow = exactly(130, 77)
    qids = w["qids"][:5].copy()
    qids[2] = N + 7
    with env(monkeypatch, PHNSW_DENSE_NODES="64"):
        dv = device_shared(w["hix"], 10, qids=qids, allow=allow)
    ref = xr.exact_topk(w["Ds"][:5], allow, None, None, 10)
    good = [0, 1, 3, 4]
    same(tuple(x[good] for x in dv[:3]), tuple(x[good] for x in ref))
    assert not dv[3][good].any() and (ref[2][good] == 10).all()
    assert dv[3][2] == 4 and dv[2][2] == 0
    assert (dv[0][2] == EMPTY).all() and (bits(dv[1][2]) == bits(xr.FMAX)).all()


def test_two_calls_in_flight_on_two_streams():
    import torch
    w = sworld("f32", 256)
    a, b = mask(0.3, N, 31), mask(0.2, N, 32)
    one = device_shared(w["hix"], 100, queries=w["q"], allow=a)
    two = device_shared(w["hix"], 100, qids=w["qids"], allow=b)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        o1 = device_shared(w["hix"], 100, queries=w["q"], allow=a, stream=s1, sync=False)
        o2 = device_shared(w["hix"], 100, qids=w["qids"], allow=b, stream=s2, sync=False)
        r1, r2 = fetch(o1), fetch(o2)
        same(r1, one)
        same(r2, two)
        assert not r1[3].any() and not r2[3].any()
    same(one, xr.exact_topk(w["Dq"], a, None, None, 100))
    same(two, xr.exact_topk(w["Ds"], b, None, None, 100))


# ---------------------------------------------------------------- 6: the kept node operand
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("i8q", 256), ("i8q", 24)])
def test_two_bitmaps_of_equal_count_do_not_share_a_packed_operand(kind, dim):
    """consecutive calls with two bitmaps of EQUAL candidate count: the id list sits at the same address with the same
    length, so a node operand kept under (address, length) would serve the first call's rows to the second"""
    w = sworld(kind, dim)
    a, b = exactly(700, 1, with_dups=False), exactly(700, 2, with_dups=True)
    assert (a != b).any()
    for allow in (a, b, a, b):
        got = w["hix"].search_exact_shared(queries=w["q"][:40], allow=allow, k=10)
        same(got, xr.exact_topk(w["Dq"][:40], allow, None, None, 10))
        dv = device_shared(w["hix"], 10, queries=w["q"][:40], allow=allow)
        same(dv, got)


def test_the_vector_unit_pass_gives_the_same_bits(monkeypatch):
    w = sworld("f32", 256)
    allow = mask(0.3, N, 51)
    base = check(w, nq=65, allow=allow, k=100)
    with env(monkeypatch, PHNSW_TINY_VALU="1"):
        now = check(w, nq=65, allow=allow, k=100)
    for form in (0, 1):
        same(base[form], now[form])


# ---------------------------------------------------------------- 7: refusals
def test_refusals():
    w = sworld("f32", 24)
    hix, q = w["hix"], w["q"][:4]
    assert hix.exact_shared_supported(10) == 0 and hix.exact_shared_supported(1024) == 0
    for k in (0, 1025):
        assert hix.exact_shared_supported(k) == -1
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_shared(queries=q, k=k)
        assert e.value.code == -1  # PHNSW_E_INVALID
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_shared: k must be 1..1024 (got %d)" % k
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_shared_device(4, k, 8, 8, 8, 8, qids=8)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_shared_device: k must be 1..1024 (got %d)" % k
    with pytest.raises(ph.PhnswError) as e:  # queries and qids
        hix.search_exact_shared_device(4, 3, 8, 8, 8, 8, queries=16, ldq=24, qids=8)
    assert e.value.code == -1 and "phnsw_search_exact_shared_device" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # neither
        hix.search_exact_shared_device(4, 3, 8, 8, 8, 8)
    assert e.value.code == -1 and "phnsw_search_exact_shared_device" in str(e.value)
    with pytest.raises(ValueError):
        hix.search_exact_shared(queries=q, qids=w["qids"][:4])
    with pytest.raises(ValueError):
        hix.search_exact_shared()
    with pytest.raises(ValueError):  # a 2-D mask: per-query bitmaps are the scan's
        hix.search_exact_shared(queries=q, allow=np.ones((4, N), dtype=bool))
    with pytest.raises(ph.PhnswError) as e:  # a stored query id at or past n: the host form refuses it as the scan's does
        hix.search_exact_shared(qids=np.array([1, N], dtype=np.uint64), k=3)
    with pytest.raises(ph.PhnswError) as e2:
        hix.search_exact_filtered(qids=np.array([1, N], dtype=np.uint64), k=3)
    assert e.value.code == e2.value.code == -1 and str(e.value) == str(e2.value)
    ids, d, ln = hix.search_exact_shared(queries=np.zeros((0, 24), dtype=np.float32), k=3)  # nq == 0: a no-op
    assert ids.shape == (0, 3)
    # PQ stores of either form: unsupported, the message names the call and points to the scan
    rows = oracle.synth_rows(0, 400, 32)[:, :32].copy()
    f2 = ph.VectorStore(rows, metric=ph.METRIC_L2)
    shared = ph.SharedPqStore(f2, 16, 100, seed=3, centroid_bp=ph.BuildParameters(seed=2),
                              quantized_search=ph.SearchParameters(32, 32, 2))
    for store in (ph.PqStore(f2, 16), shared):
        pix = ph.Hnsw.from_layers(store, ring(np.arange(400)))
        assert pix.exact_shared_supported(3) == -7
        with pytest.raises(ph.PhnswError) as e:
            pix.search_exact_shared(queries=rows[:2], k=3)
        assert e.value.code == -7  # PHNSW_E_UNSUPPORTED
        assert "phnsw_search_exact_shared:" in str(e.value) and "phnsw_search_exact_filtered" in str(e.value)
        with pytest.raises(ph.PhnswError) as e:
            pix.search_exact_shared_device(2, 3, 8, 8, 8, 8, qids=8)
        assert e.value.code == -7 and "phnsw_search_exact_shared_device:" in str(e.value)
