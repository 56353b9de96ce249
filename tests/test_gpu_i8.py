"""The i8 row store (phnsw_store_create_i8): rows are scalar-quantised per row (tests/i8_reference.py restates the
quantiser in numpy), a distance dequantises them -- scale * (float)code, one f32 multiply -- and runs the f32 chain, so
every result must equal -- ids, distance BITS, lengths, counters -- the unchanged oracle over the dequantised rows
(what store_read() returns) in the kernel's summation order (SUM_BLOCKED64).  No tolerance anywhere: the recall test
at the end compares the GPU pipeline with the same pipeline run through the oracle and prints the gap to f32."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from parallel_hnsw_amd._lib import lib
from parallel_hnsw_amd.hnsw import _p

from i8_reference import dequantize, quantize

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -7
METRICS = [oracle.METRIC_COSINE_HALF, oracle.METRIC_ONE_MINUS_DOT, oracle.METRIC_L2]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle_over(store, metric, graph=None):
    """the oracle over the rows the device really holds (store_read of the i8 / f16 store), optionally with `graph`'s layers"""
    ix = oracle.Index(store.read(), metric=metric, sum_mode=oracle.SUM_BLOCKED64)
    if graph is not None:
        for l in graph.layers:
            ix.push_layer(l.nodes, l.neighbors, l.neighborhood_size)
    return ix


def adopt(store, graph):
    return ph.Hnsw.from_layers(store, [(l.nodes, l.neighbors) for l in graph.layers], graph.build_parameters)


@functools.lru_cache(maxsize=None)
def build_pair(n, dim, metric=oracle.METRIC_COSINE_HALF, normalize=True):
    """f32 store, graph built over it by phnsw_build, the i8 store, the adopted index, the oracle over the dequantised
    rows; made once per shape and shared by the tests (none of them changes any of it)"""
    full = ph.VectorStore.synthetic(n, dim, seed=42, normalize=normalize, metric=metric)
    g = ph.Hnsw.generate(full, np.arange(n, dtype=np.uint64), ph.BuildParameters(seed=1))
    i8 = ph.I8Store.from_full(full)
    return full, g, i8, adopt(i8, g), oracle_over(i8, metric, g)


def assert_same(gpu, cpu):
    np.testing.assert_array_equal(gpu[2], cpu[2])
    np.testing.assert_array_equal(gpu[0], cpu[0])
    np.testing.assert_array_equal(bits(gpu[1]), bits(cpu[1]))
    if len(cpu) > 3:
        np.testing.assert_array_equal(gpu[3], cpu[3])  # distance evaluations and hops per query


# ---------------------------------------------------------------- 1: quantisation
def edge_rows(dim):
    rng = np.random.default_rng(dim)
    rows = rng.standard_normal((300, dim)).astype(np.float32)
    rows[0] = 0.0                                              # a zero row: scale 0, codes 0
    rows[1, 0] = 3.0e38                                        # one huge component: every other code is 0
    sub = rng.integers(-70000, 70001, size=dim).astype(np.int32)
    sub[dim - 1] = 70000
    rows[2] = (sub.astype(np.float64) * 2.0 ** -149).astype(np.float32)  # f32 subnormals, exactly
    rows[3] = np.where(np.arange(dim) % 2 == 0, 1.0, -1.0).astype(np.float32) * rng.uniform(0.1, 2.0, dim).astype(np.float32)
    rows[4, :3] = [0.5, 1.5, 2.5][:min(dim, 3)]                # with maxabs 127 below: ties, round half to even
    rows[4, 3:] = 0.0
    rows[4, dim - 1] = 127.0
    return rows


@pytest.mark.parametrize("dim", [768, 100, 6])
def test_codes_scales_and_read_equal_the_numpy_quantiser(dim):
    rows = edge_rows(dim)
    assert np.abs(rows[2]).max() < np.finfo(np.float32).tiny and rows[2].any()
    full = ph.VectorStore(rows)
    i8 = ph.I8Store.from_full(full)
    assert (i8.n, i8.dim, i8.metric, i8.rows_dev) == (full.n, full.dim, full.metric, None)
    codes, scales = quantize(rows)
    np.testing.assert_array_equal(i8.codes(), codes)
    np.testing.assert_array_equal(bits(i8.scales()), bits(scales))
    assert scales[0] == 0 and not codes[0].any() and codes[1, 0] == 127 and not codes[1, 1:].any()
    np.testing.assert_array_equal(codes[4, :3], [0, 2, 2])
    held = i8.read()
    np.testing.assert_array_equal(bits(held), bits(i8.scales()[:, None] * i8.codes().astype(np.float32)))
    np.testing.assert_array_equal(bits(held), bits(dequantize(codes, scales)))
    np.testing.assert_array_equal(bits(i8.read(first=17, count=40)), bits(held[17:57]))


@pytest.mark.parametrize("bad", [np.inf, -np.inf])
def test_store_rejects_infinities(bad):
    rows = np.ones((64, 20), dtype=np.float32)
    rows[33, 19] = bad
    with pytest.raises(ph.PhnswError) as e:
        ph.I8Store.from_full(ph.VectorStore(rows))
    assert e.value.code == E_INVALID


def test_store_rejects_nan():
    # an f32 store refuses NaN itself (PHNSW_E_NAN), so the NaN reaches create_i8 through a device-resident store
    torch = pytest.importorskip("torch")
    t = torch.ones((64, 24), dtype=torch.float32, device="cuda")
    full = ph.VectorStore.from_device(t.data_ptr(), 64, 24, 24, keepalive=t)
    t[5, 7] = float("nan")
    torch.cuda.synchronize()
    with pytest.raises(ph.PhnswError) as e:
        ph.I8Store.from_full(full)
    assert e.value.code == E_INVALID


def test_store_rejects_a_source_that_is_not_f32():
    full = ph.VectorStore(np.ones((64, 20), dtype=np.float32))
    for src in (ph.I8Store.from_full(full), ph.F16Store.from_full(full)):
        with pytest.raises(ph.PhnswError) as e:
            ph.I8Store.from_full(src)
        assert e.value.code == E_INVALID


# ---------------------------------------------------------------- 2: distance batches
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [6, 100, 256, 768, 1536])
def test_distance_batch_bit_exact(dim, metric):
    n = 300
    norm = metric != oracle.METRIC_L2
    rows = oracle.synth_rows(0, n, dim, normalize=norm)[:, :dim].copy()
    rows[3, : min(dim, 4)] *= 1.0e-6  # components far below the row's step: codes 0
    rows[5] = 0.0                     # scale 0
    i8 = ph.I8Store.from_full(ph.VectorStore(rows, metric=metric))
    held = i8.read()
    ix = oracle.Index(held, metric=metric)
    ids = np.arange(n, dtype=np.uint64)
    q = oracle.synth_rows(2 ** 32, 1, dim, normalize=norm)[0, :dim]
    got = i8.compare_vec(ph.Unstored(q), ids)
    want = np.array([ix.distance(q, held[i], oracle.SUM_BLOCKED64) for i in range(n)], dtype=np.float32)
    np.testing.assert_array_equal(bits(got), bits(want))
    got_s = i8.compare_vec(ph.Stored(3), ids)  # a stored query is its dequantised row
    want_s = np.array([ix.distance(held[3], held[i], oracle.SUM_BLOCKED64) for i in range(n)], dtype=np.float32)
    np.testing.assert_array_equal(bits(got_s), bits(want_s))


# ---------------------------------------------------------------- 3: search parity
# NV = 1 / 3 / 6, queues of every size class up to ef 256 (the headline kernel's), probe depths 2 and 8
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
    full, g, i8, hix, oix = build_pair(n, dim)
    q = oracle.synth_rows(2 ** 32, 129, dim)[:, :dim]
    sp = ph.SearchParameters(ef, upper, pd)
    assert_same(hix.search_batch(queries=q, sp=sp, stats=True), oix.search(queries=q, sp=(ef, upper, pd), stats=True))
    # the layer accessors of the adopted index
    assert hix.layer_count() == g.layer_count()
    for a, b in zip(hix.layers, g.layers):
        np.testing.assert_array_equal(a.nodes, b.nodes)
        np.testing.assert_array_equal(a.neighbors, b.neighbors)


def test_search_parity_dense_tables_serve_the_top_layers():
    full, g, i8, hix, oix = build_pair(3000, 768)
    ef = 128
    assert hix.dense_top_layers(ef)[0] > 0
    q = oracle.synth_rows(2 ** 32, 300, 768)[:, :768]
    gpu = hix.search_batch(queries=q, sp=ph.SearchParameters(ef, ef, 2), stats=True)
    assert_same(gpu, oix.search(queries=q, sp=(ef, ef, 2), stats=True))
    cap = 8
    cnt, tab = C.c_uint32(), np.zeros(cap, dtype=np.uint64)
    ph._lib.check(lib().phnsw_last_search_table_evals(hix._h, cap, C.byref(cnt), _p(tab)))
    assert tab[:cnt.value].sum() > 0  # evaluations really came from the table
    assert len(hix.dispatches()) >= 2  # the table pass and the search
    # stored queries through the table's pack step too
    qids = np.arange(0, 3000, 13, dtype=np.uint64)
    assert_same(hix.search_batch(qids=qids, sp=ph.SearchParameters(ef, ef, 2), stats=True),
                oix.search(qids=qids, sp=(ef, ef, 2), stats=True))


def test_search_parity_stored_exclude_upto_topk():
    full, g, i8, hix, oix = build_pair(2000, 128)
    qids = np.arange(0, 2000, 7, dtype=np.uint64)
    sp = ph.SearchParameters(256, 256, 2)
    assert_same(hix.search_batch(qids=qids, sp=sp, exclude=qids, stats=True),
                oix.search(qids=qids, sp=(256, 256, 2), exclude=qids, stats=True))
    assert_same(hix.search_batch(qids=qids, sp=sp, stats=True), oix.search(qids=qids, sp=(256, 256, 2), stats=True))
    q = oracle.synth_rows(2 ** 32, 100, 128)[:, :128]
    ex = np.arange(100, dtype=np.uint64)
    assert_same(hix.search_batch(queries=q, sp=sp, exclude=ex), oix.search(queries=q, sp=(256, 256, 2), exclude=ex))
    # upto: the first layers only (the oracle over the same leading layers)
    upto = hix.layer_count() - 1
    short = oracle_over(i8, oracle.METRIC_COSINE_HALF)
    for l in g.layers[:upto]:
        short.push_layer(l.nodes, l.neighbors, l.neighborhood_size)
    assert_same(hix.search_batch(queries=q, sp=sp, upto=upto, stats=True), short.search(queries=q, sp=(256, 256, 2), stats=True))
    # top-k form
    ci, cd, cl = oix.search(queries=q, sp=(256, 256, 2))
    gi, gd, gl = hix.search_batch(queries=q, sp=sp, k=10)
    np.testing.assert_array_equal(gi, ci[:, :10])
    np.testing.assert_array_equal(bits(gd), bits(cd[:, :10]))
    np.testing.assert_array_equal(gl, np.minimum(cl, 10))


def test_search_parity_l2_metric():
    full, g, i8, hix, oix = build_pair(3000, 32, oracle.METRIC_L2, False)
    q = oracle.synth_rows(2 ** 32, 100, 32, normalize=False)[:, :32]
    assert_same(hix.search_batch(queries=q, sp=ph.SearchParameters(64, 64, 2), stats=True),
                oix.search(queries=q, sp=(64, 64, 2), stats=True))


def test_search_device_form_with_exclude_upto_stats():
    torch = pytest.importorskip("torch")
    full, g, i8, hix, oix = build_pair(3000, 100)
    nq, ef = 200, 64
    q = oracle.synth_rows(2 ** 32, nq, 100)  # padded to ld
    ld = q.shape[1]
    assert ld >= i8.ld and ld % 4 == 0
    dq = torch.from_numpy(q).cuda()
    ex = torch.arange(nq, dtype=torch.int32, device="cuda")
    ids = torch.empty((nq, ef), dtype=torch.int32, device="cuda")
    d = torch.empty((nq, ef), dtype=torch.float32, device="cuda")
    ln = torch.empty(nq, dtype=torch.int32, device="cuda")
    st = torch.empty((nq, 2), dtype=torch.int32, device="cuda")
    status = torch.empty(nq, dtype=torch.int32, device="cuda")
    upto = hix.layer_count() - 1
    for u in (0, upto):
        hix.search_batch_device(nq, ph.SearchParameters(ef, ef, 2), ids.data_ptr(), d.data_ptr(), ln.data_ptr(),
                                status.data_ptr(), queries=dq.data_ptr(), ldq=ld, exclude=ex.data_ptr(),
                                out_stats=st.data_ptr(), upto=u)
        torch.cuda.synchronize()
        assert not status.cpu().numpy().any()
        ref = oix
        if u:
            ref = oracle_over(i8, oracle.METRIC_COSINE_HALF)
            for l in g.layers[:u]:
                ref.push_layer(l.nodes, l.neighbors, l.neighborhood_size)
        ci, cd, cl, cs = ref.search(queries=q[:, :100], sp=(ef, ef, 2), exclude=np.arange(nq, dtype=np.uint64), stats=True)
        gi = ids.cpu().numpy().view(np.uint32).astype(np.uint64)
        gi[gi == 0xFFFFFFFF] = oracle.EMPTY
        np.testing.assert_array_equal(ln.cpu().numpy().astype(np.uint64), cl)
        np.testing.assert_array_equal(gi, ci)
        np.testing.assert_array_equal(bits(d.cpu().numpy()), bits(cd))
        np.testing.assert_array_equal(st.cpu().numpy().astype(np.uint64), cs)


LN, LDIM, LNQ = 150_000, 32, 40_000  # the bottom layer's int8 rows (48 bytes each) exceed one XCD's L2: a launch of its own


def test_large_batch_split_descent_and_locality_order(monkeypatch):
    # the host-pointer entry points cut a long list into pipelined chunks (hostpath.hip); this test is about how ONE
    # launch of 40 000 queries descends, so the list runs whole
    monkeypatch.setenv("PHNSW_HOST_CHUNKS", "4000000000,1024,4096")
    full = ph.VectorStore.clustered(LN, LDIM, seed=42, n_clusters=300)
    g = ph.Hnsw.generate(full, np.arange(LN, dtype=np.uint64), ph.BuildParameters(max_link_rounds=1))
    i8 = ph.I8Store.from_full(full)
    hix = adopt(i8, g)
    q = ph.VectorStore.clustered(LNQ, LDIM, seed=42, first=2 ** 33, n_clusters=300).read()
    sp = ph.SearchParameters(32, 20, 2)
    f = lib().phnsw_debug_two_launch_count
    f.restype = C.c_uint64
    before = f()
    gpu = hix.search_batch(queries=q, sp=sp, stats=True)
    assert f() > before  # the split descent (cell-ordered launch for the large layer) really ran
    kinds = hix.dispatches()
    assert len(kinds) >= 3, kinds  # table pass, the search of the layers above, the search of the large layer
    m = 2000
    oix = oracle_over(i8, oracle.METRIC_COSINE_HALF, g)
    assert_same([x[:m] for x in gpu], oix.search(queries=q[:m], sp=(32, 20, 2), stats=True))
    tail = slice(LNQ - 500, LNQ)
    assert_same([x[tail] for x in gpu], oix.search(queries=q[tail], sp=(32, 20, 2), stats=True))


# ---------------------------------------------------------------- 4: re-rank
def reranked_by_oracle(oix, oracle_full, held_full, q, sp, k):
    """oracle i8 search -> distances from the f32 oracle store -> sort (d, id) -> first k"""
    ci, cd, cl = oix.search(queries=q, sp=sp)
    ids = np.full((len(q), k), oracle.EMPTY, dtype=np.uint64)
    d = np.full((len(q), k), oracle.FMAX, dtype=np.float32)
    ln = np.zeros(len(q), dtype=np.uint64)
    for i in range(len(q)):
        c = ci[i, :int(cl[i])]
        dd = np.array([oracle_full.distance(q[i], held_full[int(v)], oracle.SUM_BLOCKED64) for v in c], dtype=np.float32)
        order = np.lexsort((c, dd + np.float32(0.0)))[:k]
        ids[i, :len(order)], d[i, :len(order)], ln[i] = c[order], dd[order], len(order)
    return ids, d, ln


@pytest.mark.parametrize("n,dim,ef,k", [(3000, 100, 64, 10), (3000, 768, 128, 128), (2000, 32, 40, 1)])
def test_rerank_matches_the_oracle_and_both_forms_agree(n, dim, ef, k):
    torch = pytest.importorskip("torch")
    full, g, i8, hix, oix = build_pair(n, dim)
    held_full = full.read()
    ofull = oracle.Index(held_full, metric=oracle.METRIC_COSINE_HALF)
    nq = 120
    qp = oracle.synth_rows(2 ** 32, nq, dim)
    q = np.ascontiguousarray(qp[:, :dim])
    sp = ph.SearchParameters(ef, ef, 2)
    gi, gd, gl = hix.search_batch_reranked(full, q, sp, k)
    wi, wd, wl = reranked_by_oracle(oix, ofull, held_full, q, (ef, ef, 2), k)
    np.testing.assert_array_equal(gl, wl)
    for i in range(nq):
        np.testing.assert_array_equal(gi[i, :int(wl[i])], wi[i, :int(wl[i])])
        np.testing.assert_array_equal(bits(gd[i, :int(wl[i])]), bits(wd[i, :int(wl[i])]))
    # the distances are those of distance_batch on the f32 store
    np.testing.assert_array_equal(bits(gd[0, :int(gl[0])]), bits(full.compare_vec(ph.Unstored(q[0]), gi[0, :int(gl[0])])))
    # device form
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
    full, g, i8, hix, oix = build_pair(2000, 32)
    q = oracle.synth_rows(2 ** 32, 4, 32)[:, :32]
    other = ph.VectorStore.synthetic(1999, 32)
    for bad_full, k in ((other, 5), (i8, 5), (full, 0), (full, 65)):  # mismatched full, not an f32 store, k = 0, k > ef
        with pytest.raises(ph.PhnswError) as e:
            hix.search_batch_reranked(bad_full, q, ph.SearchParameters(64, 64, 2), k)
        assert e.value.code == E_INVALID
    L = lib()
    sp = ph.SearchParameters(64, 64, 2)
    ids, d, ln = np.zeros((4, 5), dtype=np.uint64), np.zeros((4, 5), dtype=np.float32), np.zeros(4, dtype=np.uint64)
    assert L.phnsw_i8_search_batch(hix._h, full._h, None, 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert L.phnsw_i8_search_batch(hix._h, full._h, _p(q), 4, C.byref(sp), 5, None, _p(d), _p(ln)) == E_INVALID
    assert L.phnsw_i8_search_batch(hix._h, None, _p(q), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert L.phnsw_i8_search_batch(None, full._h, _p(q), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert L.phnsw_i8_search_batch_device(hix._h, full._h, None, 32, 4, C.byref(sp), 5, None, None, None, None, None,
                                          None) == E_INVALID
    # the entry points are per store type: an f32 index and an f16 index are not i8 indexes, and the other way round
    assert L.phnsw_i8_search_batch(g._h, full._h, _p(q), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert L.phnsw_f16_search_batch(hix._h, full._h, _p(q), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    f16ix = adopt(ph.F16Store.from_full(full), g)
    assert L.phnsw_i8_search_batch(f16ix._h, full._h, _p(q), 4, C.byref(sp), 5, _p(ids), _p(d), _p(ln)) == E_INVALID
    assert b"phnsw_i8_search_batch" in L.phnsw_last_error()


# ---------------------------------------------------------------- 5: the unsupported surface
def test_everything_else_is_unsupported_by_name():
    full, g, i8, hix, oix = build_pair(2000, 32)
    L = lib()
    bp, sp, op = ph.BuildParameters(), ph.SearchParameters(), ph.BuildParameters().optimization
    vids = np.arange(2000, dtype=np.uint64)
    q = oracle.synth_rows(2 ** 32, 4, 32)[:, :32].copy()
    out_h, out_u64, out_f, out_i = C.c_void_p(), C.c_uint64(), C.c_float(), C.c_int()
    big_u64 = np.zeros(2000 * 64, dtype=np.uint64)
    big_f = np.zeros(2000 * 64, dtype=np.float32)
    path = b"/tmp/phnsw_i8_unsupported"
    calls = {
        "phnsw_build": lambda: L.phnsw_build(i8._h, _p(vids), 2000, C.byref(bp), None, None, C.byref(out_h)),
        "phnsw_build_sharded": lambda: L.phnsw_build_sharded(i8._h, _p(vids), 2000, C.byref(bp), None, ph._lib.PROGRESS_CB(),
                                                             None, C.byref(out_h), None),
        "phnsw_index_create": lambda: L.phnsw_index_create(i8._h, C.byref(bp), C.byref(out_h)),
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
        "phnsw_store_append": lambda: L.phnsw_store_append(i8._h, _p(q), 4, C.byref(out_u64)),
        "phnsw_store_create_pq": lambda: L.phnsw_store_create_pq(i8._h, 8, 16, 0, C.byref(out_h)),
        "phnsw_store_create_pq_kmeans": lambda: L.phnsw_store_create_pq_kmeans(i8._h, 8, 16, 0, 2, 0, C.byref(out_h)),
        "phnsw_store_create_pq_shared": lambda: L.phnsw_store_create_pq_shared(i8._h, 4, 64, 0, C.byref(bp), C.byref(sp), 2,
                                                                               C.byref(out_h)),
        "phnsw_bruteforce_topk": lambda: L.phnsw_bruteforce_topk(i8._h, _p(q), 4, 5, _p(big_u64), _p(big_f)),
        "phnsw_index_serialize": lambda: L.phnsw_index_serialize(hix._h, path),
        "phnsw_index_deserialize": lambda: L.phnsw_index_deserialize(i8._h, path, C.byref(out_h)),
    }
    for name, call in calls.items():
        rc = call()
        msg = (L.phnsw_last_error() or b"").decode()
        assert rc == E_UNSUPPORTED, (name, rc, msg)
        assert "i8" in msg and name.replace("_kmeans", "") in msg, (name, msg)  # (pq_kmeans is create_pq with iterations)
        assert not out_h.value
    # and the index still searches afterwards
    assert_same(hix.search_batch(queries=q, sp=ph.SearchParameters(32, 32, 2), stats=True),
                oix.search(queries=q, sp=(32, 32, 2), stats=True))


# ---------------------------------------------------------------- 6: two batches in flight
def test_two_batches_on_two_streams_equal_the_batches_alone():
    torch = pytest.importorskip("torch")
    full, g, i8, hix, oix = build_pair(3000, 768)
    nq, ef = 3000, 128  # with dense top layers: the second batch's table is made beside the first batch's search
    sp = ph.SearchParameters(ef, ef, 2)
    qs = [torch.from_numpy(oracle.synth_rows(2 ** 32 + 10 ** 6 * b, nq, 768)).cuda() for b in range(2)]

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
    # ... and the batches alone are the oracle's
    m = 100
    ci, cd, cl, cs = oix.search(queries=qs[0].cpu().numpy()[:m, :768], sp=(ef, ef, 2), stats=True)
    np.testing.assert_array_equal(alone[0][0][:m].view(np.uint32).astype(np.uint64), ci)
    np.testing.assert_array_equal(alone[0][1][:m].view(np.uint32), bits(cd))
    np.testing.assert_array_equal(alone[0][3][:m].astype(np.uint64), cs)


# ---------------------------------------------------------------- 7: recall
def test_recall_of_the_gpu_pipeline_is_the_oracle_pipelines():
    """6 000 x 768 clustered set (the bench's data family), graph built on the f32 store, ef 64: recall@10 of
    search_batch_reranked over the i8 index against bruteforce_topk on the f32 store equals the recall of the same
    pipeline computed through the oracle (search over the dequantised rows, f32 re-rank, (distance, id) sort, cut).
    The gap to the f32 index's own recall is a property of the data: printed (profiles/i8/README.md), not asserted."""
    n, dim, nq, ef = 6000, 768, 200, 64
    full = ph.VectorStore.clustered(n, dim, seed=42, n_clusters=50, noise=1.0)
    g = ph.Hnsw.generate(full, np.arange(n, dtype=np.uint64), ph.BuildParameters(seed=1))
    i8 = ph.I8Store.from_full(full)
    hix = adopt(i8, g)
    q = ph.VectorStore.clustered(nq, dim, seed=42, first=2 ** 33, n_clusters=50, noise=1.0).read()
    gt, _ = full.bruteforce_topk(q, 10)
    sp = ph.SearchParameters(ef, ef, 2)

    def recall(ids):
        return float(np.mean([len(set(ids[i, :10].tolist()) & set(gt[i].tolist())) / 10.0 for i in range(nq)]))

    held_full = full.read()
    ofull = oracle.Index(held_full, metric=oracle.METRIC_COSINE_HALF)
    wi, wd, wl = reranked_by_oracle(oracle_over(i8, oracle.METRIC_COSINE_HALF, g), ofull, held_full, q, (ef, ef, 2), 10)
    gi, gd, gl = hix.search_batch_reranked(full, q, sp, 10)
    r32 = recall(g.search_batch(queries=q, sp=sp, k=10)[0])
    r8 = recall(gi)
    r8_plain = recall(hix.search_batch(queries=q, sp=sp, k=10)[0])
    print("recall@10 at ef %d: f32 %.4f, i8 %.4f, i8 + re-rank %.4f (oracle pipeline %.4f), gap to f32 %+.4f"
          % (ef, r32, r8_plain, r8, recall(wi), r8 - r32))
    np.testing.assert_array_equal(gl, wl)
    np.testing.assert_array_equal(gi, wi)
    assert r8 == recall(wi)


# ---------------------------------------------------------------- 8: the policy seam changed nothing for f32 and f16
def test_f32_and_f16_searches_still_equal_the_oracle():
    full, g, i8, hix, oix = build_pair(2000, 32)
    q = oracle.synth_rows(2 ** 32, 129, 32)[:, :32]
    sp = ph.SearchParameters(40, 40, 8)
    assert_same(g.search_batch(queries=q, sp=sp, stats=True),
                oracle_over(full, oracle.METRIC_COSINE_HALF, g).search(queries=q, sp=(40, 40, 8), stats=True))
    f16 = ph.F16Store.from_full(full)
    assert_same(adopt(f16, g).search_batch(queries=q, sp=sp, stats=True),
                oracle_over(f16, oracle.METRIC_COSINE_HALF, g).search(queries=q, sp=(40, 40, 8), stats=True))
