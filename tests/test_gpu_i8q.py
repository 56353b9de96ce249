"""The i8q row store (phnsw_store_create_i8q): the rows of an i8 store, searched with an int8 query and integer dot
products.  tests/i8q_reference.py restates the distance in numpy.  Two yardsticks, no tolerance anywhere:
  * on general data every distance must equal the numpy restatement bit for bit (distance batches, and every (id, d) a
    search returns), and a search must not depend on how it was run (dense tables or per hop, locality order, where
    the visited set lives);
  * on `lattice` data (codes times a power of two) the i8q distance equals the f32 arithmetic of the unchanged oracle
    over the dequantised rows (tests/test_i8q_cpu.py proves that on the CPU), so there a search must equal the oracle's
    -- ids, distance bits, lengths, counters."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from parallel_hnsw_amd._lib import lib
from parallel_hnsw_amd.hnsw import _p

import i8q_reference
from i8_reference import dequantize, quantize
from test_gpu_i8 import adopt, assert_same, bits, edge_rows, oracle_over

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -7
METRICS = [oracle.METRIC_COSINE_HALF, oracle.METRIC_ONE_MINUS_DOT]
COS = oracle.METRIC_COSINE_HALF


def lattice_rows(n, dim, seed, k_range=12):
    rows, c, k = i8q_reference.lattice(n, dim, np.random.default_rng(seed), k_range)
    # what makes the oracle's f32 sums exact on these rows, asserted on the inputs themselves
    assert int(np.abs(c.astype(np.int64)).sum(axis=1).max()) * 127 < 2 ** 24
    return rows


@functools.lru_cache(maxsize=None)
def lattice_pair(n, dim, k_range=12, metric=COS):
    """f32 store of lattice rows, the graph phnsw_build makes over it, the i8q store, the adopted index and the oracle
    over store.read(); made once per shape, changed by no test"""
    full = ph.VectorStore(lattice_rows(n, dim, 7919 * n + dim + k_range, k_range), metric=metric)
    g = ph.Hnsw.generate(full, np.arange(n, dtype=np.uint64), ph.BuildParameters(seed=1))
    st = ph.I8QStore.from_full(full)
    return full, g, st, adopt(st, g), oracle_over(st, metric, g)


@functools.lru_cache(maxsize=None)
def general_pair(n, dim):
    """the same over oracle.synth_rows rows; no oracle: general data is checked against the numpy restatement"""
    full = ph.VectorStore.synthetic(n, dim, seed=42)
    g = ph.Hnsw.generate(full, np.arange(n, dtype=np.uint64), ph.BuildParameters(seed=1))
    st = ph.I8QStore.from_full(full)
    return full, g, st, adopt(st, g)


def lattice_queries(nq, dim, k_range=12):
    return lattice_rows(nq, dim, 104729 + dim + k_range, k_range)


class env:
    def __init__(self, monkeypatch, **kv):
        self.mp, self.kv = monkeypatch, kv

    def __enter__(self):
        self.ctx = self.mp.context()
        m = self.ctx.__enter__()
        for k, v in self.kv.items():
            m.setenv(k, v)

    def __exit__(self, *a):
        return self.ctx.__exit__(*a)


def same_bytes(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


# ---------------------------------------------------------------- 1: the store
@pytest.mark.parametrize("dim", [768, 100, 6])
def test_rows_are_an_i8_stores_rows(dim):
    rows = edge_rows(dim)  # a zero row, a huge component, a subnormal row, half-to-even ties
    full = ph.VectorStore(rows)
    i8, st = ph.I8Store.from_full(full), ph.I8QStore.from_full(full)
    assert (st.n, st.dim, st.metric, st.rows_dev) == (full.n, full.dim, full.metric, None)
    np.testing.assert_array_equal(st.codes(), i8.codes())
    np.testing.assert_array_equal(bits(st.scales()), bits(i8.scales()))
    np.testing.assert_array_equal(bits(st.read()), bits(i8.read()))
    codes, scales = quantize(rows)
    np.testing.assert_array_equal(st.codes(), codes)
    np.testing.assert_array_equal(bits(st.scales()), bits(scales))
    np.testing.assert_array_equal(bits(st.read(first=17, count=40)), bits(dequantize(codes, scales)[17:57]))


@pytest.mark.parametrize("bad", [np.inf, -np.inf])
def test_store_rejects_infinities(bad):
    rows = np.ones((64, 20), dtype=np.float32)
    rows[33, 19] = bad
    with pytest.raises(ph.PhnswError) as e:
        ph.I8QStore.from_full(ph.VectorStore(rows))
    assert e.value.code == E_INVALID


def test_store_rejects_nan():
    torch = pytest.importorskip("torch")
    t = torch.ones((64, 24), dtype=torch.float32, device="cuda")
    full = ph.VectorStore.from_device(t.data_ptr(), 64, 24, 24, keepalive=t)
    t[5, 7] = float("nan")
    torch.cuda.synchronize()
    with pytest.raises(ph.PhnswError) as e:
        ph.I8QStore.from_full(full)
    assert e.value.code == E_INVALID


def test_store_rejects_a_source_that_is_not_f32():
    full = ph.VectorStore(np.ones((64, 20), dtype=np.float32))
    for src in (ph.I8Store.from_full(full), ph.F16Store.from_full(full), ph.I8QStore.from_full(full)):
        with pytest.raises(ph.PhnswError) as e:
            ph.I8QStore.from_full(src)
        assert e.value.code == E_INVALID


def test_store_refuses_the_euclidean_metric():
    full = ph.VectorStore(np.ones((64, 20), dtype=np.float32), metric=oracle.METRIC_L2)
    with pytest.raises(ph.PhnswError) as e:
        ph.I8QStore.from_full(full)
    assert e.value.code == E_UNSUPPORTED and "phnsw_store_create_i8q" in str(e.value)
    ph.I8Store.from_full(full)  # the i8 store still takes it


# ---------------------------------------------------------------- 2: distance batches on general data
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [6, 100, 256, 768, 1536])
def test_distance_batch_equals_the_numpy_restatement(dim, metric):
    n = 300
    rows = oracle.synth_rows(0, n, dim)[:, :dim].copy()
    rows[3, : min(dim, 4)] *= 1.0e-6  # components far below the row's step: codes 0
    rows[5] = 0.0                     # scale 0
    st = ph.I8QStore.from_full(ph.VectorStore(rows, metric=metric))
    codes, scales = st.codes(), st.scales()
    assert scales[5] == 0
    ids = np.arange(n, dtype=np.uint64)
    q = oracle.synth_rows(2 ** 32, 1, dim)[0, :dim].copy()
    last = q.copy()
    last[dim - 1] = 3.0  # the maxabs sits in the last component (at dim 6 and 100: in the row's ragged last chunks)
    for query in (q, np.zeros(dim, dtype=np.float32), last):
        got = st.compare_vec(ph.Unstored(query), ids)
        np.testing.assert_array_equal(bits(got), bits(i8q_reference.distance(query, codes, scales, metric)))
    got_s = st.compare_vec(ph.Stored(3), ids)  # a stored query: its codes and scale as they are, not requantised
    np.testing.assert_array_equal(bits(got_s), bits(i8q_reference.distance_codes(codes[3], scales[3], codes, scales, metric)))
    got_z = st.compare_vec(ph.Stored(5), ids)
    np.testing.assert_array_equal(bits(got_z), bits(i8q_reference.distance_codes(codes[5], scales[5], codes, scales, metric)))


# ---------------------------------------------------------------- 3: search parity on lattice data
# NV = 1 / 3 / 6, queues of every size class, the <4, DistI8Q<3, 8>> kernel, probe depths 2 and 8
@pytest.mark.parametrize("n,dim,ef,upper,pd", [
    (2000, 128, 64, 64, 2),
    (2000, 128, 128, 16, 2),
    (3000, 768, 128, 128, 2),
    (3000, 768, 256, 256, 2),
    (3000, 100, 32, 32, 8),
    (2000, 32, 40, 40, 8),
    (2000, 1536, 32, 32, 2),
])
def test_search_parity(n, dim, ef, upper, pd):
    full, g, st, hix, oix = lattice_pair(n, dim)
    q = lattice_queries(129, dim)
    assert_same(hix.search_batch(queries=q, sp=ph.SearchParameters(ef, upper, pd), stats=True),
                oix.search(queries=q, sp=(ef, upper, pd), stats=True))
    assert hix.layer_count() == g.layer_count()


def test_search_parity_with_many_exact_ties():
    # every scale is 1: distances are small integers over 2, equal ones abound and the id decides
    full, g, st, hix, oix = lattice_pair(2000, 32, 0)
    q = lattice_queries(129, 32, 0)
    cpu = oix.search(queries=q, sp=(64, 64, 2), stats=True)
    d = cpu[1][:, :64]
    assert (d[:, 1:] == d[:, :-1]).sum() >= 10  # ties really occur inside the result rows (41 among the exact top 64s)
    assert_same(hix.search_batch(queries=q, sp=ph.SearchParameters(64, 64, 2), stats=True), cpu)


def test_search_parity_one_minus_dot():
    full, g, st, hix, oix = lattice_pair(2000, 32, 12, oracle.METRIC_ONE_MINUS_DOT)
    q = lattice_queries(100, 32)
    assert_same(hix.search_batch(queries=q, sp=ph.SearchParameters(64, 64, 2), stats=True),
                oix.search(queries=q, sp=(64, 64, 2), stats=True))


def test_search_parity_stored_exclude_upto_topk():
    full, g, st, hix, oix = lattice_pair(2000, 128)
    qids = np.arange(0, 2000, 7, dtype=np.uint64)
    sp = ph.SearchParameters(256, 256, 2)
    assert_same(hix.search_batch(qids=qids, sp=sp, exclude=qids, stats=True),
                oix.search(qids=qids, sp=(256, 256, 2), exclude=qids, stats=True))
    assert_same(hix.search_batch(qids=qids, sp=sp, stats=True), oix.search(qids=qids, sp=(256, 256, 2), stats=True))
    q = lattice_queries(100, 128)
    ex = np.arange(100, dtype=np.uint64)
    assert_same(hix.search_batch(queries=q, sp=sp, exclude=ex), oix.search(queries=q, sp=(256, 256, 2), exclude=ex))
    upto = hix.layer_count() - 1
    short = oracle_over(st, COS)
    for l in g.layers[:upto]:
        short.push_layer(l.nodes, l.neighbors, l.neighborhood_size)
    assert_same(hix.search_batch(queries=q, sp=sp, upto=upto, stats=True), short.search(queries=q, sp=(256, 256, 2), stats=True))
    ci, cd, cl = oix.search(queries=q, sp=(256, 256, 2))
    gi, gd, gl = hix.search_batch(queries=q, sp=sp, k=10)
    np.testing.assert_array_equal(gi, ci[:, :10])
    np.testing.assert_array_equal(bits(gd), bits(cd[:, :10]))
    np.testing.assert_array_equal(gl, np.minimum(cl, 10))


def test_search_device_form_with_exclude_and_stats():
    torch = pytest.importorskip("torch")
    full, g, st, hix, oix = lattice_pair(3000, 100)
    nq, ef = 200, 64
    q, _, ld = oracle.pad_rows(lattice_queries(nq, 100))
    assert ld >= st.ld and ld % 4 == 0
    dq = torch.from_numpy(q).cuda()
    ex = torch.arange(nq, dtype=torch.int32, device="cuda")
    ids = torch.empty((nq, ef), dtype=torch.int32, device="cuda")
    d = torch.empty((nq, ef), dtype=torch.float32, device="cuda")
    ln = torch.empty(nq, dtype=torch.int32, device="cuda")
    stt = torch.empty((nq, 2), dtype=torch.int32, device="cuda")
    status = torch.empty(nq, dtype=torch.int32, device="cuda")
    hix.search_batch_device(nq, ph.SearchParameters(ef, ef, 2), ids.data_ptr(), d.data_ptr(), ln.data_ptr(),
                            status.data_ptr(), queries=dq.data_ptr(), ldq=ld, exclude=ex.data_ptr(), out_stats=stt.data_ptr())
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    ci, cd, cl, cs = oix.search(queries=q[:, :100], sp=(ef, ef, 2), exclude=np.arange(nq, dtype=np.uint64), stats=True)
    gi = ids.cpu().numpy().view(np.uint32).astype(np.uint64)
    gi[gi == 0xFFFFFFFF] = oracle.EMPTY
    np.testing.assert_array_equal(ln.cpu().numpy().astype(np.uint64), cl)
    np.testing.assert_array_equal(gi, ci)
    np.testing.assert_array_equal(bits(d.cpu().numpy()), bits(cd))
    np.testing.assert_array_equal(stt.cpu().numpy().astype(np.uint64), cs)


# ---------------------------------------------------------------- 4: the int8 table == the per-hop path
def table_evals(hix):
    cap = 8
    cnt, tab = C.c_uint32(), np.zeros(cap, dtype=np.uint64)
    ph._lib.check(lib().phnsw_last_search_table_evals(hix._h, cap, C.byref(cnt), _p(tab)))
    return int(tab[:cnt.value].sum())


@pytest.mark.parametrize("data", ["lattice", "general"])
def test_table_equals_per_hop(data, monkeypatch):
    if data == "lattice":
        full, g, st, hix, oix = lattice_pair(3000, 768)
        q = lattice_queries(300, 768)
    else:
        full, g, st, hix = general_pair(3000, 768)
        q = oracle.synth_rows(2 ** 32, 300, 768)[:, :768]
    ef = 128
    sp = ph.SearchParameters(ef, ef, 2)
    assert hix.dense_top_layers(ef)[0] > 0
    qids = np.arange(0, 3000, 13, dtype=np.uint64)
    runs = {}
    for name, kw in (("raw", dict(queries=q)), ("five", dict(queries=q[:5])), ("stored", dict(qids=qids))):
        with env(monkeypatch, PHNSW_TINY_VALU="1"):  # means nothing to this kind: the int8 kernel all the same
            got = hix.search_batch(sp=sp, stats=True, **kw)
        assert table_evals(hix) > 0      # evaluations really came from the table
        assert len(hix.dispatches()) >= 2  # the table pass and the search
        with env(monkeypatch, PHNSW_NO_TINY="1"):
            hop = hix.search_batch(sp=sp, stats=True, **kw)
            assert table_evals(hix) == 0
        same_bytes(got, hop)
        runs[name] = got
    if data == "lattice":
        assert_same(runs["raw"], oix.search(queries=q, sp=(ef, ef, 2), stats=True))
        assert_same(runs["stored"], oix.search(qids=qids, sp=(ef, ef, 2), stats=True))


def test_table_equals_per_hop_ragged_dimension(monkeypatch):
    # 100 dimensions: K padded from 100 to 128 code bytes, partial tiles on both sides (261 queries, a few hundred nodes)
    full, g, st, hix = general_pair(2000, 100)
    q = oracle.synth_rows(2 ** 32, 261, 100)[:, :100]
    sp = ph.SearchParameters(64, 64, 2)
    assert hix.dense_top_layers(64)[0] > 0
    got = hix.search_batch(queries=q, sp=sp, stats=True)
    assert table_evals(hix) > 0
    with env(monkeypatch, PHNSW_NO_TINY="1"):
        same_bytes(got, hix.search_batch(queries=q, sp=sp, stats=True))


# ---------------------------------------------------------------- 5: general data, whatever the traversal
@pytest.mark.parametrize("n,dim,ef", [(3000, 768, 128), (2000, 100, 64)])
def test_general_data_distances_order_and_independence_of_the_schedule(n, dim, ef, monkeypatch):
    full, g, st, hix = general_pair(n, dim)
    codes, scales = st.codes(), st.scales()
    q = oracle.synth_rows(2 ** 32, 200, dim)[:, :dim]
    sp = ph.SearchParameters(ef, ef, 2)
    got = hix.search_batch(queries=q, sp=sp, stats=True)
    gi, gd, gl = got[:3]
    for i in range(len(q)):
        L = int(gl[i])
        assert L > 0
        ids = gi[i, :L].astype(np.int64)
        assert len(set(ids.tolist())) == L
        want = i8q_reference.distance(q[i], codes[ids], scales[ids], COS)
        np.testing.assert_array_equal(bits(gd[i, :L]), bits(want))
        key = list(zip((gd[i, :L] + np.float32(0.0)).tolist(), ids.tolist()))
        assert key == sorted(key)
    same_bytes(got, hix.search_batch(queries=q, sp=sp, stats=True))  # a second run
    with env(monkeypatch, PHNSW_NO_LOCALITY="1"):
        same_bytes(got, hix.search_batch(queries=q, sp=sp, stats=True))
    with env(monkeypatch, PHNSW_VISITED="global"):
        same_bytes(got, hix.search_batch(queries=q, sp=sp, stats=True))


# ---------------------------------------------------------------- 6: split descent
LN, LDIM, LNQ = 150_000, 32, 40_000  # the bottom layer's int8 rows (48 bytes each) exceed one XCD's L2: a launch of its own


def test_large_batch_split_descent(monkeypatch):
    monkeypatch.setenv("PHNSW_HOST_CHUNKS", "4000000000,1024,4096")  # the list runs whole (see test_gpu_i8)
    full = ph.VectorStore(lattice_rows(LN, LDIM, 5))
    g = ph.Hnsw.generate(full, np.arange(LN, dtype=np.uint64), ph.BuildParameters(max_link_rounds=1))
    st = ph.I8QStore.from_full(full)
    hix = adopt(st, g)
    q = lattice_rows(LNQ, LDIM, 6)
    sp = ph.SearchParameters(32, 20, 2)
    f = lib().phnsw_debug_two_launch_count
    f.restype = C.c_uint64
    before = f()
    gpu = hix.search_batch(queries=q, sp=sp, stats=True)
    assert f() > before
    oix = oracle_over(st, COS, g)
    m = 2000
    assert_same([x[:m] for x in gpu], oix.search(queries=q[:m], sp=(32, 20, 2), stats=True))
    tail = slice(LNQ - 500, LNQ)
    assert_same([x[tail] for x in gpu], oix.search(queries=q[tail], sp=(32, 20, 2), stats=True))


# ---------------------------------------------------------------- 7: re-rank
@pytest.mark.parametrize("n,dim,ef,k", [(2000, 100, 64, 10), (3000, 768, 128, 128)])
def test_rerank_both_forms_agree_and_distances_are_the_f32_stores(n, dim, ef, k):
    torch = pytest.importorskip("torch")
    full, g, st, hix = general_pair(n, dim)
    nq = 120
    qp = oracle.synth_rows(2 ** 32, nq, dim)
    q = np.ascontiguousarray(qp[:, :dim])
    sp = ph.SearchParameters(ef, ef, 2)
    gi, gd, gl = hix.search_batch_reranked(full, q, sp, k)
    pi, pd, pl = hix.search_batch(queries=q, sp=sp)
    for i in range(nq):
        L = int(gl[i])
        assert L == min(int(pl[i]), k)
        assert set(gi[i, :L].tolist()) <= set(pi[i, :int(pl[i])].tolist())
        np.testing.assert_array_equal(bits(gd[i, :L]), bits(full.compare_vec(ph.Unstored(q[i]), gi[i, :L])))
        key = list(zip((gd[i, :L] + np.float32(0.0)).tolist(), gi[i, :L].tolist()))
        assert key == sorted(key)
        if k >= int(pl[i]):
            assert set(gi[i, :L].tolist()) == set(pi[i, :L].tolist())
    dq = torch.from_numpy(qp).cuda()
    ids = torch.empty((nq, ef), dtype=torch.int32, device="cuda")
    d = torch.empty((nq, ef), dtype=torch.float32, device="cuda")
    ln = torch.empty(nq, dtype=torch.int32, device="cuda")
    status = torch.empty(nq, dtype=torch.int32, device="cuda")
    hix.search_batch_reranked_device(full, nq, sp, k, dq.data_ptr(), qp.shape[1], ids.data_ptr(), d.data_ptr(), ln.data_ptr(),
                                     status.data_ptr())
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    di = ids.cpu().numpy().view(np.uint32).astype(np.uint64)
    np.testing.assert_array_equal(ln.cpu().numpy().astype(np.uint64), gl)
    for i in range(nq):
        L = int(gl[i])
        np.testing.assert_array_equal(di[i, :L], gi[i, :L])
        np.testing.assert_array_equal(bits(d.cpu().numpy()[i, :L]), bits(gd[i, :L]))
        assert (di[i, L:] == 0xFFFFFFFF).all()


def test_rerank_argument_checks():
    full, g, st, hix = general_pair(2000, 32)
    q = oracle.synth_rows(2 ** 32, 4, 32)[:, :32]
    other = ph.VectorStore.synthetic(1999, 32)
    for bad_full, k in ((other, 5), (st, 5), (full, 0), (full, 65)):  # mismatched full, not an f32 store, k = 0, k > ef
        with pytest.raises(ph.PhnswError) as e:
            hix.search_batch_reranked(bad_full, q, ph.SearchParameters(64, 64, 2), k)
        assert e.value.code == E_INVALID
    L = lib()
    sp = ph.SearchParameters(64, 64, 2)
    ids, d, ln = np.zeros((4, 5), dtype=np.uint64), np.zeros((4, 5), dtype=np.float32), np.zeros(4, dtype=np.uint64)
    assert L.phnsw_i8q_search_batch(hix._h, full._h, None, 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert L.phnsw_i8q_search_batch(hix._h, full._h, _p(q), 4, C.byref(sp), 5, None, _p(d), _p(ln)) == E_INVALID
    assert L.phnsw_i8q_search_batch(hix._h, None, _p(q), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert L.phnsw_i8q_search_batch(None, full._h, _p(q), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert L.phnsw_i8q_search_batch_device(hix._h, full._h, None, 32, 4, C.byref(sp), 5, None, None, None, None, None,
                                           None) == E_INVALID
    # the entry points are per store kind: the i8 call refuses an i8q index, and the other way round
    assert L.phnsw_i8_search_batch(hix._h, full._h, _p(q), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert b"phnsw_i8_search_batch" in L.phnsw_last_error()
    assert L.phnsw_f16_search_batch(hix._h, full._h, _p(q), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    i8ix = adopt(ph.I8Store.from_full(full), g)
    assert L.phnsw_i8q_search_batch(i8ix._h, full._h, _p(q), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert L.phnsw_i8q_search_batch(g._h, full._h, _p(q), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert b"phnsw_i8q_search_batch" in L.phnsw_last_error() and b"i8q store" in L.phnsw_last_error()
    assert L.phnsw_i8_search_batch(i8ix._h, full._h, _p(q), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == 0


# ---------------------------------------------------------------- 8: the unsupported surface
def test_everything_else_is_unsupported_by_name():
    full, g, st, hix = general_pair(2000, 32)
    L = lib()
    bp, sp, op = ph.BuildParameters(), ph.SearchParameters(), ph.BuildParameters().optimization
    vids = np.arange(2000, dtype=np.uint64)
    q = oracle.synth_rows(2 ** 32, 4, 32)[:, :32].copy()
    out_h, out_u64, out_f, out_i = C.c_void_p(), C.c_uint64(), C.c_float(), C.c_int()
    big_u64 = np.zeros(2000 * 64, dtype=np.uint64)
    big_f = np.zeros(2000 * 64, dtype=np.float32)
    path = b"/tmp/phnsw_i8q_unsupported"
    calls = {
        "phnsw_build": lambda: L.phnsw_build(st._h, _p(vids), 2000, C.byref(bp), None, None, C.byref(out_h)),
        "phnsw_build_sharded": lambda: L.phnsw_build_sharded(st._h, _p(vids), 2000, C.byref(bp), None, ph._lib.PROGRESS_CB(),
                                                             None, C.byref(out_h), None),
        "phnsw_index_create": lambda: L.phnsw_index_create(st._h, C.byref(bp), C.byref(out_h)),
        "phnsw_generate_layer": lambda: L.phnsw_generate_layer(hix._h, _p(vids), 10, 24, C.byref(bp)),
        "phnsw_link_layer": lambda: L.phnsw_link_layer(hix._h, 0, C.byref(sp), 24, C.byref(out_u64)),
        "phnsw_improve_index": lambda: L.phnsw_improve_index(hix._h, C.byref(bp), float("nan"), None, None, C.byref(out_f)),
        "phnsw_improve_neighbors_upto": lambda: L.phnsw_improve_neighbors_upto(hix._h, 1, C.byref(bp), float("nan"), C.byref(out_f)),
        "phnsw_improve_index_sharded": lambda: L.phnsw_improve_index_sharded(hix._h, C.byref(bp), float("nan"), None,
                                                                             C.byref(out_f), None),
        "phnsw_extend_layer": lambda: L.phnsw_extend_layer(hix._h, 0, _p(vids), 1),
        "phnsw_promote_at_layer": lambda: L.phnsw_promote_at_layer(hix._h, 0, C.byref(bp), C.byref(out_i)),
        "phnsw_discover_unreachable": lambda: L.phnsw_discover_unreachable(hix._h, 0, C.byref(sp), _p(big_u64), C.byref(out_u64)),
        "phnsw_stochastic_recall_at": lambda: L.phnsw_stochastic_recall_at(hix._h, 0, C.byref(op), C.byref(out_f)),
        "phnsw_knn": lambda: L.phnsw_knn(hix._h, 3, 2, _p(big_u64), _p(big_f), _p(big_u64)),
        "phnsw_threshold_nn": lambda: L.phnsw_threshold_nn(hix._h, 0.1, 2, 8, 64, _p(big_u64), _p(big_f), _p(big_u64)),
        "phnsw_search_instrumented": lambda: L.phnsw_search_instrumented(hix._h, _p(q), None, 4, C.byref(sp), _p(big_u64),
                                                                         _p(big_f), _p(big_u64), _p(big_u64)),
        "phnsw_store_append": lambda: L.phnsw_store_append(st._h, _p(q), 4, C.byref(out_u64)),
        "phnsw_store_create_pq": lambda: L.phnsw_store_create_pq(st._h, 8, 16, 0, C.byref(out_h)),
        "phnsw_store_create_pq_kmeans": lambda: L.phnsw_store_create_pq_kmeans(st._h, 8, 16, 0, 2, 0, C.byref(out_h)),
        "phnsw_store_create_pq_shared": lambda: L.phnsw_store_create_pq_shared(st._h, 4, 64, 0, C.byref(bp), C.byref(sp), 2,
                                                                               C.byref(out_h)),
        "phnsw_bruteforce_topk": lambda: L.phnsw_bruteforce_topk(st._h, _p(q), 4, 5, _p(big_u64), _p(big_f)),
        "phnsw_index_serialize": lambda: L.phnsw_index_serialize(hix._h, path),
        "phnsw_index_deserialize": lambda: L.phnsw_index_deserialize(st._h, path, C.byref(out_h)),
    }
    for name, call in calls.items():
        rc = call()
        msg = (L.phnsw_last_error() or b"").decode()
        assert rc == E_UNSUPPORTED, (name, rc, msg)
        assert "i8q store" in msg and name.replace("_kmeans", "") in msg, (name, msg)
        assert not out_h.value
    # and the index still searches afterwards
    got = hix.search_batch(queries=q, sp=ph.SearchParameters(32, 32, 2))
    codes, scales = st.codes(), st.scales()
    for i in range(4):
        ids = got[0][i, :int(got[2][i])].astype(np.int64)
        np.testing.assert_array_equal(bits(got[1][i, :len(ids)]), bits(i8q_reference.distance(q[i], codes[ids], scales[ids], COS)))


# ---------------------------------------------------------------- 9: two batches in flight
def test_two_batches_on_two_streams_equal_the_batches_alone():
    torch = pytest.importorskip("torch")
    full, g, st, hix, oix = lattice_pair(3000, 768)
    nq, ef = 3000, 128  # with dense top layers: the second batch's table is made beside the first batch's search
    sp = ph.SearchParameters(ef, ef, 2)
    qs = [torch.from_numpy(lattice_rows(nq, 768, 31 + b)).cuda() for b in range(2)]

    def outputs():
        return (torch.empty((nq, ef), dtype=torch.int32, device="cuda"), torch.empty((nq, ef), dtype=torch.float32, device="cuda"),
                torch.empty(nq, dtype=torch.int32, device="cuda"), torch.empty((nq, 2), dtype=torch.int32, device="cuda"),
                torch.empty(nq, dtype=torch.int32, device="cuda"))

    def launch(b, o, stream):
        hix.search_batch_device(nq, sp, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[4].data_ptr(),
                                queries=qs[b].data_ptr(), ldq=qs[b].shape[1], out_stats=o[3].data_ptr(), stream=stream)

    alone = []
    for b in range(2):
        o = outputs()
        launch(b, o, 0)
        torch.cuda.synchronize()
        alone.append([t.cpu().numpy() for t in o])
    s0 = torch.cuda.Stream()
    s1 = torch.cuda.Stream()
    both = [outputs(), outputs()]
    for rep in range(2):
        launch(0, both[0], s0.cuda_stream)
        launch(1, both[1], s1.cuda_stream)
    torch.cuda.synchronize()
    for b in range(2):
        for got, want in zip(both[b], alone[b]):
            np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert not alone[b][4].any()
    m = 100
    ci, cd, cl, cs = oix.search(queries=qs[0].cpu().numpy()[:m], sp=(ef, ef, 2), stats=True)
    np.testing.assert_array_equal(alone[0][0][:m].view(np.uint32).astype(np.uint64), ci)
    np.testing.assert_array_equal(alone[0][1][:m].view(np.uint32), bits(cd))
    np.testing.assert_array_equal(alone[0][3][:m].astype(np.uint64), cs)


# ---------------------------------------------------------------- 10: nothing else moved
def test_f32_f16_and_i8_searches_still_equal_the_oracle():
    full, g, st, hix = general_pair(2000, 32)
    q = oracle.synth_rows(2 ** 32, 129, 32)[:, :32]
    sp = ph.SearchParameters(40, 40, 8)
    assert_same(g.search_batch(queries=q, sp=sp, stats=True), oracle_over(full, COS, g).search(queries=q, sp=(40, 40, 8), stats=True))
    for kind in (ph.F16Store, ph.I8Store):
        low = kind.from_full(full)
        assert_same(adopt(low, g).search_batch(queries=q, sp=sp, stats=True),
                    oracle_over(low, COS, g).search(queries=q, sp=(40, 40, 8), stats=True))
