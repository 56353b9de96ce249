"""The bits row store (phnsw_store_create_bits): one sign bit per component, a distance from the popcount of row XOR
query (tests/bits_reference.py restates it in numpy).  On ALL data that distance equals the f32 arithmetic of the
unchanged oracle over the +1 / -1 rows store.read() returns with the query where(q < 0, -1, +1) -- tests/test_bits_cpu.py
proves that on the CPU -- so every search here must equal the oracle in ids, distance BITS, lengths and both counters.
No tolerance anywhere and no recall threshold: the re-rank test asserts a theorem about the walk's own rows.

Wall time of the file on an MI355X: 3.1 s for its 70 cases."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import bits_reference as br
from bits_reference import bit_edge_rows
from test_gpu_i8 import adopt, assert_same, bits, edge_rows, oracle_over

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -7
COS, DOT, L2 = oracle.METRIC_COSINE_HALF, oracle.METRIC_ONE_MINUS_DOT, oracle.METRIC_L2
METRICS = [COS, DOT, L2]


# ---------------------------------------------------------------- 1: the store
@pytest.mark.parametrize("dim", [768, 100, 6])
def test_words_and_read_equal_the_numpy_restatement(dim):
    rows = np.concatenate([edge_rows(dim), bit_edge_rows(dim)])
    full = ph.VectorStore(rows)
    st = ph.BitStore.from_full(full)
    assert (st.n, st.dim, st.ld, st.metric, st.rows_dev) == (full.n, full.dim, full.ld, full.metric, None)
    want = br.pack(rows)
    got = st.words()
    assert got.shape == (len(rows), (dim + 31) // 32)
    np.testing.assert_array_equal(got, want)
    e = len(edge_rows(dim))
    assert not got[e].any() and not got[e + 1].any() and not got[e + 2].any()  # zeros, -0.0, positive subnormals
    np.testing.assert_array_equal(got[e + 3], got[e + 4])                      # negative subnormals: every bit
    assert int(br.hamming(got[e + 3], np.zeros_like(got[e + 3]))) == dim      # ... and no padding bit
    held = st.read()
    np.testing.assert_array_equal(bits(held), bits(br.unpack(want, dim)))
    np.testing.assert_array_equal(bits(held), bits(np.where(rows < 0, -1.0, 1.0)))
    np.testing.assert_array_equal(bits(st.read(first=17, count=40)), bits(held[17:57]))


@pytest.mark.parametrize("bad", [np.inf, -np.inf])
def test_store_rejects_infinities(bad):
    rows = np.ones((64, 20), dtype=np.float32)
    rows[33, 19] = bad
    with pytest.raises(ph.PhnswError) as e:
        ph.BitStore.from_full(ph.VectorStore(rows))
    assert e.value.code == E_INVALID


def test_store_rejects_nan():
    # an f32 store refuses NaN itself, so the NaN reaches create_bits through a device-resident store
    torch = pytest.importorskip("torch")
    t = torch.ones((64, 24), dtype=torch.float32, device="cuda")
    full = ph.VectorStore.from_device(t.data_ptr(), 64, 24, 24, keepalive=t)
    t[5, 7] = float("nan")
    torch.cuda.synchronize()
    with pytest.raises(ph.PhnswError) as e:
        ph.BitStore.from_full(full)
    assert e.value.code == E_INVALID


def test_store_rejects_a_source_that_is_not_f32_and_accepts_l2():
    full = ph.VectorStore(np.ones((64, 20), dtype=np.float32))
    for src in (ph.I8Store.from_full(full), ph.F16Store.from_full(full), ph.BitStore.from_full(full)):
        with pytest.raises(ph.PhnswError) as e:
            ph.BitStore.from_full(src)
        assert e.value.code == E_INVALID
    l2 = ph.BitStore.from_full(ph.VectorStore(np.ones((64, 20), dtype=np.float32), metric=L2))
    assert l2.metric == L2


# ---------------------------------------------------------------- 2: distance batches
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [6, 100, 256, 768, 1536])
def test_distance_batch_bit_exact(dim, metric):
    n = 300
    rng = np.random.default_rng(7 * dim + metric)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows[:7] = bit_edge_rows(dim)[:7]
    st = ph.BitStore.from_full(ph.VectorStore(rows, metric=metric))
    w = br.pack(rows)
    np.testing.assert_array_equal(st.words(), w)
    q = rng.standard_normal(dim).astype(np.float32)
    q[0] = -0.0
    perm = rng.permutation(n).astype(np.uint64)
    for m in (1, 63, 64, 65, 300):
        ids = perm[:m].copy()
        ids[-1] = n - 1               # the last row and (past one entry; alone below) the first are always in the list
        if m > 1:
            ids[0] = 0
        got = st.compare_vec(ph.Unstored(q), ids)
        np.testing.assert_array_equal(bits(got), bits(br.distances(w[ids.astype(np.int64)], br.pack(q)[0], dim, metric)))
        got_s = st.compare_vec(ph.Stored(11), ids)  # a stored query is its row as it is
        np.testing.assert_array_equal(bits(got_s), bits(br.distances(w[ids.astype(np.int64)], w[11], dim, metric)))
    got0 = st.compare_vec(ph.Unstored(q), np.array([0], dtype=np.uint64))
    np.testing.assert_array_equal(bits(got0), bits(br.distances(w[:1], br.pack(q)[0], dim, metric)))


# ---------------------------------------------------------------- 3: searches against the oracle
WORLDS = [(4000, 768, COS), (2000, 100, COS), (2000, 1536, COS), (2000, 100, DOT), (2000, 100, L2)]
EFS = [16, 100, 256, 512, 1024]  # queues of 128, 128, 256, 512 and 1024 slots


@functools.lru_cache(maxsize=None)
def world(n, dim, metric):
    """f32 store, the graph built over it, the bits store, the adopted index, the oracle over the +-1 rows with the same
    graph, 70 raw queries and their +-1 form, 70 stored queries; made once per shape, never changed"""
    norm = metric != L2
    full = ph.VectorStore.synthetic(n, dim, seed=42, normalize=norm, metric=metric)
    g = ph.Hnsw.generate(full, np.arange(n, dtype=np.uint64), ph.BuildParameters(seed=1))
    st = ph.BitStore.from_full(full)
    q = oracle.synth_rows(2 ** 32, 70, dim, normalize=norm)[:, :dim].copy()
    q[0, : min(dim, 5)] = [-0.0, 0.0, -1e-42, 1e-42, -1.0][: min(dim, 5)]
    qids = np.arange(3, n, n // 70, dtype=np.uint64)[:70]
    return full, g, st, adopt(st, g), oracle_over(st, metric, g), q, br.signed_query(q), qids


@functools.lru_cache(maxsize=None)
def truth(n, dim, metric, ef, pd=2):
    """the oracle's answer for the world's raw and stored queries: computed once, shared by the tests of that shape"""
    oix, sq, qids = world(n, dim, metric)[4], world(n, dim, metric)[6], world(n, dim, metric)[7]
    return oix.search(queries=sq, sp=(ef, ef, pd), stats=True), oix.search(qids=qids, sp=(ef, ef, pd), stats=True)


@pytest.mark.parametrize("ef", EFS)
@pytest.mark.parametrize("n,dim,metric", WORLDS)
def test_search_equals_the_oracle_over_the_sign_rows(n, dim, metric, ef):
    full, g, st, hix, oix, q, sq, qids = world(n, dim, metric)
    want_raw, want_stored = truth(n, dim, metric, ef)
    sp = ph.SearchParameters(ef, ef, 2)
    assert hix.dense_top_layers(ef)[0] == 0
    got = hix.search_batch(queries=q, sp=sp, stats=True)
    assert_same(got, want_raw)
    d = hix.dispatches()
    assert d[1]["n_table"] == 0 and d[1]["n_dist"] == int(want_raw[3][:, 0].sum())
    assert_same(hix.search_batch(qids=qids, sp=sp, stats=True), want_stored)
    # the distances are the restatement's, in sign-vector units
    w = st.words()
    for i in (0, 1, 69):
        m = int(got[2][i])
        np.testing.assert_array_equal(bits(got[1][i, :m]), bits(br.distances(w[got[0][i, :m].astype(np.int64)], br.pack(q[i])[0], dim, metric)))


@pytest.mark.parametrize("ef", [100, 1024])
@pytest.mark.parametrize("n,dim,metric", WORLDS)
def test_device_form_agrees_with_the_host_form_byte_for_byte(n, dim, metric, ef):
    torch = pytest.importorskip("torch")
    full, g, st, hix, oix, q, sq, qids = world(n, dim, metric)
    sp = ph.SearchParameters(ef, ef, 2)
    nq = len(q)
    qp = np.zeros((nq, st.ld), dtype=np.float32)
    qp[:, :dim] = q
    dq = torch.from_numpy(qp).cuda()
    ids = torch.empty((nq, ef), dtype=torch.int32, device="cuda")
    d = torch.empty((nq, ef), dtype=torch.float32, device="cuda")
    ln = torch.empty(nq, dtype=torch.int32, device="cuda")
    stats = torch.empty((nq, 2), dtype=torch.int32, device="cuda")
    status = torch.empty(nq, dtype=torch.int32, device="cuda")
    hix.search_batch_device(nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=dq.data_ptr(),
                            ldq=qp.shape[1], out_stats=stats.data_ptr())
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    hi, hd, hl, hs = hix.search_batch(queries=q, sp=sp, stats=True)
    di = ids.cpu().numpy().view(np.uint32).astype(np.uint64)
    np.testing.assert_array_equal(ln.cpu().numpy().astype(np.uint64), hl)
    np.testing.assert_array_equal(stats.cpu().numpy().view(np.uint32).astype(np.uint64), hs)
    for i in range(nq):
        m = int(hl[i])
        np.testing.assert_array_equal(di[i, :m], hi[i, :m])
        np.testing.assert_array_equal(d.cpu().numpy()[i, :m].view(np.uint32), bits(hd[i, :m]))


@pytest.mark.parametrize("n,dim,metric", WORLDS[:3])
def test_visited_in_the_bitmap_agrees_with_the_default(monkeypatch, n, dim, metric):
    full, g, st, hix, oix, q, sq, qids = world(n, dim, metric)
    monkeypatch.setenv("PHNSW_VISITED", "global")
    for ef in (100, 256):
        assert_same(hix.search_batch(queries=q, sp=ph.SearchParameters(ef, ef, 2), stats=True), truth(n, dim, metric, ef)[0])


@pytest.mark.parametrize("n,dim,metric", WORLDS[:3])
def test_a_spill_list_of_64_entries_takes_the_overflow_and_rerun_path(monkeypatch, n, dim, metric):
    """a workspace keeps the largest spill list it ever had, so the forced calls get an index of their own"""
    torch = pytest.importorskip("torch")
    full, g, st, hix, oix, q, sq, qids = world(n, dim, metric)
    ef, pd = 16, 8
    want = oix.search(queries=sq, sp=(ef, ef, pd), stats=True)
    sp = ph.SearchParameters(ef, ef, pd)
    assert_same(hix.search_batch(queries=q, sp=sp, stats=True), want)
    monkeypatch.setenv("PHNSW_OVF_CAP", "64")
    fresh = adopt(st, g)
    nq = len(q)
    qp = np.zeros((nq, st.ld), dtype=np.float32)
    qp[:, :dim] = q
    dq = torch.from_numpy(qp).cuda()
    ids = torch.empty((nq, ef), dtype=torch.int32, device="cuda")
    d = torch.empty((nq, ef), dtype=torch.float32, device="cuda")
    ln = torch.empty(nq, dtype=torch.int32, device="cuda")
    status = torch.empty(nq, dtype=torch.int32, device="cuda")
    fresh.search_batch_device(nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=dq.data_ptr(),
                              ldq=qp.shape[1])
    torch.cuda.synchronize()
    s = status.cpu().numpy()
    assert (s == 5).any() and set(s.tolist()) <= {0, 5}  # the overflow really happens: the device form re-runs nothing
    assert_same(adopt(st, g).search_batch(queries=q, sp=sp, stats=True), want)  # the host form re-runs them


# ---------------------------------------------------------------- 4: re-rank
@pytest.mark.parametrize("k", [1, 10, 256])
@pytest.mark.parametrize("n,dim,metric", [(4000, 768, COS), (2000, 100, L2)])
def test_rerank_equals_the_restatement_on_the_walks_own_rows(n, dim, metric, k):
    """The re-ranked row is, bit for bit, the k smallest by (f32 distance, id) of the walk's own candidates.  Hence the
    theorem: every member of the brute-force top-k that is among the walk's candidates is in the re-ranked row (ties at
    the k-th distance resolved by id, as the truth resolves them)."""
    full, g, st, hix, oix, q, sq, qids = world(n, dim, metric)
    ef = 256
    sp = ph.SearchParameters(ef, ef, 2)
    wi, wd, wl = hix.search_batch(queries=q, sp=sp)
    gi, gd, gl = hix.search_batch_reranked(full, q, sp, k)
    fd = np.full(wi.shape, np.finfo(np.float32).max, dtype=np.float32)
    for i in range(len(q)):
        m = int(wl[i])
        fd[i, :m] = full.compare_vec(ph.Unstored(q[i]), wi[i, :m])
    ri, rd, rl = br.rerank(wi, wl, fd, k)
    np.testing.assert_array_equal(gl, rl)
    for i in range(len(q)):
        m = int(rl[i])
        np.testing.assert_array_equal(gi[i, :m], ri[i, :m])
        np.testing.assert_array_equal(bits(gd[i, :m]), bits(rd[i, :m]))
    # the theorem, against a truth made here: all n distances of the f32 store, sorted by (distance, id)
    allids = np.arange(n, dtype=np.uint64)
    for i in (0, 17, 69):
        d_all = full.compare_vec(ph.Unstored(q[i]), allids) + np.float32(0.0)
        top = np.lexsort((allids, d_all))[:k]
        cand = set(wi[i, :int(wl[i])].tolist())
        assert {int(t) for t in top if int(t) in cand} <= set(gi[i, :int(gl[i])].tolist())


def test_rerank_argument_checks_and_kinds():
    full, g, st, hix, oix, q, sq, qids = world(2000, 100, COS)
    other = ph.VectorStore.synthetic(1999, 100)
    for bad_full, k in ((other, 5), (st, 5), (full, 0), (full, 65)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_batch_reranked(bad_full, q, ph.SearchParameters(64, 64, 2), k)
        assert e.value.code == E_INVALID
    L = ph.lib()
    sp = ph.SearchParameters(64, 64, 2)
    from parallel_hnsw_amd.hnsw import _p
    q4 = np.ascontiguousarray(q[:4])
    ids, d, ln = np.zeros((4, 5), dtype=np.uint64), np.zeros((4, 5), dtype=np.float32), np.zeros(4, dtype=np.uint64)
    # the entry points are per store kind
    assert L.phnsw_i8q_search_batch(hix._h, full._h, _p(q4), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert L.phnsw_bits_search_batch(g._h, full._h, _p(q4), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert b"phnsw_bits_search_batch" in L.phnsw_last_error() and b"bits store" in L.phnsw_last_error()
    assert L.phnsw_bits_search_batch(hix._h, full._h, _p(q4), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == 0
