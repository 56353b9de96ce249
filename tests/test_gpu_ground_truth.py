"""Run time on an MI355X: 6 s (19 cases, the slowest 0.8 s); run it under `timeout -k 10 60`.

The ground truth and the re-rank tail at the sizes only the benchmark reaches.

recall@10 of every measured cell is counted against phnsw_bruteforce_topk_device, which at 10 000 queries x 1M rows scores
the base rows a chunk at a time and merges each chunk's candidates into the keys the chunks before it left; the re-rank,
trim and take kernels launch at most 4096 blocks and stride beyond.  Here these paths run at small shapes:

  B  many chunks forced by PHNSW_BF_CHUNK_ROWS (a last partial chunk, ties that only the id decides across chunks, the
     nearest rows placed in the last chunk, duplicates on both sides of a chunk boundary), and the same inputs with the
     knob unset: not a bit may differ
  C  the chunking the formula itself chooses (40 960 queries: three chunks, and more than 4096 blocks), and the 2^20 cap
  D  the device entry point the way the benchmark calls it: a wider ldq, u32 ids, a stream of the caller's
  E  more than 4096 queries through ph_take_kernel, ph_pq_rerank_kernel and ph_rerank_trim_kernel

Every expected value is the CPU oracle's (SUM_SEQFMA for the GEMM's k-ordered fma chain, SUM_BLOCKED64 for the search
kernels) or value_families.topk64 (exact f64, rounded once); every constructed input asserts on the REFERENCE that it
is the case it claims to be, before the GPU is asked."""
import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
import value_families as vf
from value_families import bits

pytestmark = pytest.mark.gpu

HOST_LISTS_WHOLE = "4000000000,1024,4096"
KNOB = "PHNSW_BF_CHUNK_ROWS"
E_INVALID = -1
BF_TN = 128
BLOCK_CAP = 4096   # blocks of ph_topk_chunk_kernel / ph_pq_rerank_kernel; the trim and take kernels: 4096 x 256 threads
KS = (1, 10, 16)
NQ = 70


def formula_chunk(n, nq):
    """rows per chunk of phnsw_bruteforce_topk_device with the knob unset"""
    return min(max(BF_TN, min(n, (640 << 20) // nq // BF_TN * BF_TN)), 1 << 20)


def reference(rows, q, metric, k, exact):
    """(ids, d) of the oracle in the GEMM's summation order; on an exact (lattice) input topk64 must agree with it"""
    dim = q.shape[1]
    ci, cd = oracle.Index(rows, dim=dim, metric=metric).bruteforce(q, k, sum_mode=oracle.SUM_SEQFMA)
    if exact:
        ti, td = vf.topk64(rows, q, metric, k)
        np.testing.assert_array_equal(ci, ti, err_msg="the two references disagree (ids)")
        np.testing.assert_array_equal(bits(cd), bits(td), err_msg="the two references disagree (distance bits)")
    return ci, cd


def assert_topk(got, want, msg):
    np.testing.assert_array_equal(got[0], want[0], err_msg=msg + " (ids)")
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]), err_msg=msg + " (distance bits)")


# ---------------------------------------------------------------- B: many chunks through the knob
# family, n, dim, chunk rows: 6 chunks (last of 60 rows), 4 (232), 3 (77), 8 (104)
CHUNKED = [(f, n, dim, c) for (n, dim, c) in ((700, 100, 128), (1000, 260, 256), (333, 768, 128))
           for f in ("lattice", "scaled", "cancelling")] + [("lattice1", 1000, 3, 128)]
LAST_ROWS = {(700, 128): 60, (1000, 256): 232, (333, 128): 77, (1000, 128): 104}
NEAR_Q, DUP_Q = range(0, 8), range(8, 16)   # the queries of the two constructions on `scaled`


def scaled_across_chunks(n, dim, chunk):
    """vf.scaled with (a) the two nearest rows of each of the first 8 queries copied into the last, partial chunk and
    (b) the nearest row of each of the next 8 queries copied over a row of another full chunk"""
    rows, q = vf.scaled(n, dim, nq=NQ)
    top2, _ = reference(rows, q, 0, 2, False)
    src = rows.copy()
    used = set(int(v) for v in top2[NEAR_Q.start:NEAR_Q.stop].reshape(-1))
    dst = n - 1
    for i in NEAR_Q:
        for r in top2[i]:
            while dst in used:
                dst -= 1
            rows[dst] = src[int(r)]
            used.add(dst)
    assert dst >= n - n % chunk, "the copies left the last chunk"
    near, _ = reference(rows, q, 0, 1, False)
    full_chunks = n // chunk
    assert full_chunks >= 2
    used |= set(int(near[i, 0]) for i in DUP_Q)
    src = rows.copy()
    for i in DUP_Q:
        r = int(near[i, 0])
        dst = ((r // chunk + 1) % full_chunks) * chunk + 5
        while dst in used:
            dst += 1
        assert dst // chunk != r // chunk and dst < full_chunks * chunk
        rows[dst] = src[r]
        used.add(dst)
    return rows, q


def chunked_input(family, n, dim, chunk):
    if family == "scaled":
        return scaled_across_chunks(n, dim, chunk)
    return vf.make(family, n, dim, nq=NQ)


def check_constructed(family, n, chunk, k, want):
    """the conditions on the reference that make a case bite"""
    wi, wd = want
    last_first = n - n % chunk
    if family == "lattice1" and k == 16:
        one_value = (bits(wd) == bits(wd)[:, :1]).all(axis=1)
        assert 2 * one_value.sum() >= len(wd), "all ties: %d of %d lists hold one distance" % (one_value.sum(), len(wd))
        # ... and then the list is the 16 smallest ids of the tie group: nothing of a later chunk may win
        assert (np.diff(wi[one_value].astype(np.int64), axis=1) > 0).all()
    if family == "scaled" and k > 1:
        for i in NEAR_Q:
            assert (wi[i] >= last_first).any() and (wi[i] < last_first).any(), \
                "query %d: the expected list lies on one side of the last chunk: %s" % (i, wi[i])
        for i in DUP_Q:
            a, b = int(wi[i, 0]), int(wi[i, 1])
            assert a < b and a // chunk != b // chunk and bits(wd)[i, 0] == bits(wd)[i, 1], \
                "query %d: no duplicate pair across a chunk boundary at the head of the list: %s" % (i, wi[i, :2])


@pytest.mark.parametrize("family,n,dim,chunk", CHUNKED)
def test_bruteforce_across_chunks(family, n, dim, chunk, monkeypatch):
    assert n % chunk == LAST_ROWS[(n, chunk)] and formula_chunk(n, NQ) == n   # many chunks, a partial last one; one without
    rows, q = chunked_input(family, n, dim, chunk)
    for metric in (0, 1):
        store = ph.VectorStore(rows[:, :dim], metric=metric)
        for k in KS:
            msg = "%s n %d dim %d metric %d k %d" % (family, n, dim, metric, k)
            want = reference(rows, q, metric, k, family.startswith("lattice"))
            check_constructed(family, n, chunk, k, want)
            chunks = (n + chunk - 1) // chunk
            if k == 16 and family != "lattice1":
                assert len(np.unique(want[0] // chunk)) == chunks, msg + ": a chunk holds no expected id"
            with monkeypatch.context() as mp:
                mp.setenv(KNOB, str(chunk - 1 if chunk == 256 else chunk))   # 255 is rounded up to 256
                forced = store.bruteforce_topk(q, k)
            assert_topk(forced, want, msg + " in chunks of %d rows" % chunk)
            whole = store.bruteforce_topk(q, k)
            assert_topk(whole, forced, msg + ": one chunk against %d" % chunks)


# ---------------------------------------------------------------- C: the formula's own chunking, and the 2^20 cap
def sample_of(nq):
    """both ends, both sides of the block cap, every 97th"""
    return np.unique(np.concatenate([np.arange(64), np.arange(BLOCK_CAP - 32, BLOCK_CAP + 64), np.arange(nq - 64, nq),
                                     np.arange(0, nq, 97)]))


def test_bruteforce_at_the_formulas_chunking():
    nq, n, dim, k = 40960, 40000, 8, 10
    chunk = formula_chunk(n, nq)
    chunks = (n + chunk - 1) // chunk
    if chunks == 1:
        pytest.skip("the chunk formula scores %d rows x %d queries in one chunk: this case needs new sizes" % (n, nq))
    assert (chunk, chunks, n - (chunks - 1) * chunk) == (16384, 3, 7232)
    rows = oracle.synth_rows(0, n, dim)
    q = oracle.synth_rows(2 ** 32, nq, dim)[:, :dim]
    pick = sample_of(nq)
    assert pick[0] == 0 and pick[-1] == nq - 1 and {BLOCK_CAP - 1, BLOCK_CAP}.issubset(pick.tolist())
    want = reference(rows, q[pick], 0, k, False)
    per_chunk = np.bincount((want[0] // chunk).reshape(-1).astype(np.int64), minlength=chunks)
    assert (per_chunk > len(pick)).all(), "expected ids per chunk: %s" % per_chunk
    gi, gd = ph.VectorStore(rows[:, :dim], metric=0).bruteforce_topk(q, k)
    for name, sel in (("the first 64", pick < 64), ("both sides of the 4096-block cap", (pick >= 4064) & (pick < 4160)),
                      ("the last 64", pick >= nq - 64), ("the whole sample", pick >= 0)):
        assert_topk((gi[pick[sel]], gd[pick[sel]]), (want[0][sel], want[1][sel]), "formula chunking, " + name)
    # no query outside the sample may be a row nobody wrote
    assert (gi < n).all() and np.isfinite(gd).all() and (np.diff(gd, axis=1) >= 0).all()


@pytest.mark.parametrize("family", ["lattice", "scaled"])
def test_bruteforce_past_the_chunk_cap(family):
    cap, dim, nq, k = 1 << 20, 4, 8, 16
    n = cap + 200
    assert formula_chunk(n, nq) == cap   # two chunks, the second of 200 rows
    rows, q = vf.make(family, n, dim, nq=nq)
    near, _ = reference(rows, q, 0, k, False)
    assert (near < cap).all()   # with the plain generator nothing of the second chunk is ever expected
    rows[n - nq * k:] = rows[near.reshape(-1).astype(np.int64)]
    for metric in (0, 1):
        want = reference(rows, q, metric, k, family == "lattice")
        for i in range(nq):
            assert (want[0][i] < cap).any() and (want[0][i] >= cap).any(), \
                "query %d: the expected list lies on one side of 2^20: %s" % (i, want[0][i])
        got = ph.VectorStore(rows[:, :dim], metric=metric).bruteforce_topk(q, k)
        assert_topk(got, want, "%s n 2^20 + 200 metric %d" % (family, metric))


# ---------------------------------------------------------------- D: the device entry point as the benchmark calls it
@pytest.mark.parametrize("n,dim", [(700, 100), (333, 768)])
def test_bruteforce_device_entry(n, dim, monkeypatch):
    torch = pytest.importorskip("torch")
    chunk = 128
    monkeypatch.setenv(KNOB, str(chunk))
    for family in ("scaled", "lattice"):
        rows, q = chunked_input(family, n, dim, chunk)
        for metric in (0, 1):
            store = ph.VectorStore(rows[:, :dim], metric=metric)
            ld, ldq = store.ld, store.ld + 4
            qt = torch.zeros((NQ, ldq), dtype=torch.float32, device="cuda")
            qt[:, :dim] = torch.from_numpy(q).cuda()
            qt[:, ld:] = 1e30   # K = ld: columns past it are not the query's
            stream = torch.cuda.Stream()
            assert stream.cuda_stream != 0
            for k in KS:
                msg = "%s n %d dim %d metric %d k %d device entry" % (family, n, dim, metric, k)
                want = reference(rows, q, metric, k, family == "lattice")
                ids = torch.full((NQ, k), -7, dtype=torch.int32, device="cuda")
                d = torch.full((NQ, k), float("nan"), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()   # the inputs were written on the default stream
                ms = store.bruteforce_topk_device(qt.data_ptr(), ldq, NQ, k, ids.data_ptr(), d.data_ptr(), stream.cuda_stream)
                assert ms > 0.0, msg + ": phnsw_bruteforce_last_gemm_ms"
                got = ids.cpu().numpy().view(np.uint32).astype(np.uint64), d.cpu().numpy()
                assert_topk(got, want, msg)
                assert_topk(got, store.bruteforce_topk(q, k), msg + " against the host entry")
    # the argument checks the device form adds (on the last store and queries of the loop)
    ids = torch.empty((NQ, 17), dtype=torch.int32, device="cuda")
    d = torch.empty((NQ, 17), dtype=torch.float32, device="cuda")
    few = ph.VectorStore(rows[:10, :dim], metric=0)
    for st, bad_ldq, k in ((store, ld - 4, 10), (store, ld + 2, 10), (store, ldq, 17), (few, ldq, 16)):
        with pytest.raises(ph.PhnswError) as e:
            st.bruteforce_topk_device(qt.data_ptr(), bad_ldq, NQ, k, ids.data_ptr(), d.data_ptr(), stream.cuda_stream)
        assert e.value.code == E_INVALID, (bad_ldq, k)
    few.bruteforce_topk_device(qt.data_ptr(), ldq, NQ, 10, ids.data_ptr(), d.data_ptr(), stream.cuda_stream)   # k = n is served


# ---------------------------------------------------------------- E: more than 4096 queries through take, re-rank, trim
def windows(nq):
    assert nq > BLOCK_CAP + 64 + 64
    return (("queries 0..63", slice(0, 64)), ("queries 4064..4159, both sides of the 4096-block cap", slice(4064, 4160)),
            ("the last 64 queries", slice(nq - 64, nq)), ("the whole batch", slice(0, nq)))


def assert_lists(got, want, msg):
    """(ids, d, len[, counters]) equal: lengths, then every live entry's id and distance bits"""
    nq = len(want[2])
    width = np.arange(want[0].shape[1])[None, :]
    for name, w in windows(nq):
        m = "%s: %s" % (msg, name)
        np.testing.assert_array_equal(got[2][w], want[2][w], err_msg=m + " (lengths)")
        live = width < want[2][w].astype(np.int64)[:, None]
        np.testing.assert_array_equal(np.where(live, got[0][w], 0), np.where(live, want[0][w], 0), err_msg=m + " (ids)")
        np.testing.assert_array_equal(np.where(live, bits(got[1][w]), 0), np.where(live, bits(want[1][w]), 0),
                                      err_msg=m + " (distance bits)")
        if len(want) > 3:
            np.testing.assert_array_equal(got[3][w], want[3][w], err_msg=m + " (distance evaluations, hops)")


def test_take_past_its_block_cap(monkeypatch):
    """phnsw_search_batch of 4300 queries at ef = k = 256: ph_take_kernel copies 1.1 M > 4096 x 256 entries"""
    monkeypatch.setenv("PHNSW_HOST_CHUNKS", HOST_LISTS_WHOLE)
    n, dim, nq, ef = 3000, 32, 4300, 256
    assert nq * ef > BLOCK_CAP * 256
    rows = oracle.synth_rows(0, n, dim)
    oix = oracle.Index.generate(rows, np.arange(n), oracle.default_build_params(seed=0), dim=dim, sum_mode=oracle.SUM_BLOCKED64)
    store = ph.VectorStore(rows[:, :dim])
    gix = ph.Hnsw.from_layers(store, [oix.layer(l) for l in range(oix.layer_count)])
    q = oracle.synth_rows(2 ** 32, nq, dim)[:, :dim]
    cpu = oix.search(queries=q, sp=(ef, ef, 2), stats=True)
    assert cpu[2].max() == ef
    gpu = gix.search_batch(queries=q, sp=ph.SearchParameters(ef, ef, 2), stats=True)
    assert_lists(gpu, cpu, "f32 search of %d queries at ef %d" % (nq, ef))
    np.testing.assert_array_equal(gpu[0], cpu[0])   # the padding too
    np.testing.assert_array_equal(bits(gpu[1]), bits(cpu[1]))


@pytest.fixture(scope="module")
def f16_pair():
    """test_gpu_f16.build_pair(3000, 32), 4300 queries and every f32 distance of the re-rank, computed once"""
    from test_gpu_f16 import build_pair
    n, dim, nq = 3000, 32, 4300
    full, g, f16, hix, oix = build_pair(n, dim)
    held_full = full.read()
    qp = oracle.synth_rows(2 ** 32, nq, dim)
    q = np.ascontiguousarray(qp[:, :dim])
    dist = vf.oracle_matrix(held_full, q, oracle.METRIC_COSINE_HALF, oracle.SUM_BLOCKED64)
    ofull = oracle.Index(held_full, metric=oracle.METRIC_COSINE_HALF)
    one = np.array([ofull.distance(q[4100], held_full[v], oracle.SUM_BLOCKED64) for v in range(0, n, 7)], dtype=np.float32)
    np.testing.assert_array_equal(bits(dist[4100, ::7]), bits(one))   # the matrix holds what reranked_by_oracle asks per id
    dist.setflags(write=False)
    return full, hix, oix, qp, q, dist


def reranked_by_matrix(oix, dist, q, sp, k):
    """test_gpu_f16.reranked_by_oracle with its f32 distances read from one matrix: the oracle's search over the halves ->
    distances from the f32 rows -> sort (d, id) -> first k"""
    ci, cd, cl = oix.search(queries=q, sp=sp)
    ids = np.full((len(q), k), oracle.EMPTY, dtype=np.uint64)
    d = np.full((len(q), k), oracle.FMAX, dtype=np.float32)
    ln = np.zeros(len(q), dtype=np.uint64)
    for i in range(len(q)):
        c = ci[i, :int(cl[i])]
        dd = dist[i, c.astype(np.int64)]
        order = np.lexsort((c, dd + np.float32(0.0)))[:k]
        ids[i, :len(order)], d[i, :len(order)], ln[i] = c[order], dd[order], len(order)
    return ids, d, ln


@pytest.mark.parametrize("ef,k", [(256, 10), (40, 40)])
def test_rerank_and_trim_past_their_block_caps(f16_pair, ef, k, monkeypatch):
    """4300 queries through ph_pq_rerank_kernel (4096 blocks); at ef 256, k 10 ph_rerank_trim_kernel strides as well
    (1.1 M entries > 4096 x 256 threads); at ef = k = 40 there is no trim"""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("PHNSW_HOST_CHUNKS", HOST_LISTS_WHOLE)
    full, hix, oix, qp, q, dist = f16_pair
    nq = len(q)
    assert nq > BLOCK_CAP and (k == ef or nq * ef > BLOCK_CAP * 256)
    sp = ph.SearchParameters(ef, ef, 2)
    want = reranked_by_matrix(oix, dist, q, (ef, ef, 2), k)
    assert want[2].max() == k
    host = hix.search_batch_reranked(full, q, sp, k)
    msg = "f16 search + re-rank of %d queries, ef %d k %d" % (nq, ef, k)
    assert_lists(host, want, msg)
    # device form: rows keep the search's stride, the first len entries are live, the rest empty
    dq = torch.from_numpy(qp).cuda()
    ids = torch.full((nq, ef), 7, dtype=torch.int32, device="cuda")
    d = torch.zeros((nq, ef), dtype=torch.float32, device="cuda")
    ln = torch.empty(nq, dtype=torch.int32, device="cuda")
    status = torch.empty(nq, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    hix.search_batch_reranked_device(full, nq, sp, k, dq.data_ptr(), qp.shape[1], ids.data_ptr(), d.data_ptr(), ln.data_ptr(),
                                     status.data_ptr())
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    di = ids.cpu().numpy().view(np.uint32).astype(np.uint64)
    dd = d.cpu().numpy()
    dl = ln.cpu().numpy().astype(np.uint64)
    assert_lists((di[:, :k], dd[:, :k], dl), host, msg + ", device form against the host form")
    dead = np.arange(ef)[None, :] >= dl.astype(np.int64)[:, None]
    for name, w in windows(nq):
        assert (di[w][dead[w]] == 0xFFFFFFFF).all() and (bits(dd[w])[dead[w]] == bits(oracle.FMAX)).all(), \
            "%s: %s: entries past len are not empty" % (msg, name)


def test_pq_rerank_past_its_block_cap(monkeypatch):
    """8300 queries: past the 4096 blocks of the re-rank and the 8192 of the query-encode kernel"""
    from test_gpu_pq import make
    monkeypatch.setenv("PHNSW_HOST_CHUNKS", HOST_LISTS_WHOLE)
    n, dim, m, ksub, nq = 2500, 64, 16, 256, 8300
    rows, full, pq, ocodes, ocb = make(n, dim, m, ksub, seed=1, clustered=True)
    g = ph.Hnsw.generate(pq, np.arange(n), ph.BuildParameters(seed=2, promote=0))
    oix = oracle.Index(rows, dim=dim, sum_mode=oracle.SUM_BLOCKED64)
    oix.set_pq(ocodes, ocb)
    for l in g.layers:
        oix.push_layer(l.nodes, l.neighbors, l.neighborhood_size)
    ofull = oracle.Index(rows, dim=dim, sum_mode=oracle.SUM_BLOCKED64)
    ofull.set_sum_mode(oracle.SUM_BLOCKED64)
    qh = ph.QuantizedHnsw.__new__(ph.QuantizedHnsw)
    qh.full, qh.store, qh.hnsw = full, pq, g
    q = oracle.synth_clustered_rows(2 ** 32, nq, dim, n_clusters=20)[:, :dim]
    assert nq > 8192
    sp = (64, 64, 2)
    for quant in (False, True):
        want = oix.pq_search(ofull, q, sp, quantize_query=quant)
        assert want[2].max() == sp[0]
        got = qh.search_batch(q, ph.SearchParameters(*sp), quantize_query=quant)
        assert_lists(got, want, "PQ search + re-rank of %d queries, quantize_query %s" % (nq, quant))
