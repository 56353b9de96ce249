"""Run time on an MI355X: 16 s (147 cases, first clean run); run it under `timeout -k 10 48`, three times that.

Distance parity on value edges (tests/value_families.py): negative and huge distances, subnormal products, exact ties,
cancelling sums and L2 sums that overflow, through every place the library does distance arithmetic: distance_batch,
the search kernels under every switch, the build, the brute-force GEMM, the f16 store and the PQ lookup tables.  Every
expected value comes from the CPU oracle (test_value_families_cpu.py proves its premises) or from the float64 reference
(ref64 / ref32 / topk64); nothing compares the library with itself alone."""
import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
import value_families as vf
from value_families import bits, graph_over, oracle_matrix

pytestmark = pytest.mark.gpu

METRICS = [0, 1, 2]
DIMS = [3, 100, 256, 260, 768, 1536]
FAMILIES = ["lattice", "scaled", "cancelling", "tiny", "wide"]
FAMILY_METRIC = [(f, m) for f in FAMILIES for m in METRICS] + [("l2_overflow", 2)]
HOST_LISTS_WHOLE = "4000000000,1024,4096"   # the knob tests/conftest.py sets for the modules about one launch


def assert_same(gpu, cpu, msg):
    np.testing.assert_array_equal(gpu[2], cpu[2], err_msg=msg + " (lengths)")
    np.testing.assert_array_equal(gpu[0], cpu[0], err_msg=msg + " (ids)")
    np.testing.assert_array_equal(bits(gpu[1]), bits(cpu[1]), err_msg=msg + " (distance bits)")
    if len(cpu) > 3 and len(gpu) > 3:
        np.testing.assert_array_equal(gpu[3], cpu[3], err_msg=msg + " (distance evaluations, hops)")


# ---------------------------------------------------------------- a: phnsw_distance_batch
def check_distances(store, rows, q, metric, msg, lattice):
    n, dim = rows.shape[0], q.shape[1]
    ids = np.arange(n, dtype=np.uint64)
    stored = [0, 2, n - 1]
    allq = np.concatenate([q, rows[stored, :dim]])
    got = np.stack([store.compare_vec(ph.Unstored(x), ids) for x in q] + [store.compare_vec(ph.Stored(s), ids) for s in stored])
    want = oracle_matrix(rows, allq, metric, oracle.SUM_BLOCKED64)
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=msg + ": the oracle in SUM_BLOCKED64")
    r32 = vf.ref32(rows, allq, metric)
    fin = np.isfinite(r32)
    np.testing.assert_array_equal(np.isinf(got) & (got > 0), ~fin, err_msg=msg + ": +inf where the sum passes f32::MAX")
    err = np.abs(got[fin].astype(np.float64) - vf.ref64(rows, allq, metric)[fin])
    bnd = vf.bound(rows, allq, metric)[fin]
    w = np.argmax(err - bnd)
    assert (err <= bnd).all(), "%s: |gpu - ref64| = %g > bound %g" % (msg, err[w], bnd[w])
    if lattice:
        np.testing.assert_array_equal(bits(got), bits(r32), err_msg=msg + ": the correctly rounded f64 result")


@pytest.mark.parametrize("family,metric", FAMILY_METRIC)
def test_distance_batch(family, metric):
    for dim in DIMS + [1, 6]:
        rows, q = vf.make(family, 200, dim, nq=6)
        store = ph.VectorStore(rows[:, :dim], metric=metric)
        check_distances(store, rows, q, metric, "%s dim %d metric %d distance_batch" % (family, dim, metric), family == "lattice")
    if family == "lattice":
        rows, q = vf.make("lattice1", 200, 6, nq=6)
        check_distances(ph.VectorStore(rows[:, :6], metric=metric), rows, q, metric, "lattice1 dim 6 metric %d" % metric, True)


# ---------------------------------------------------------------- b: search
def search_pair(family, metric, dim, n=None, nq=48):
    """rows, queries, the oracle index (graph by Index.generate in SUM_BLOCKED64) and the GPU index adopted from it.
    l2_overflow: the reference cannot build over rows at +inf from everything (a search that starts there finds its
    candidates empty and panics, lib.rs:181), so the graph of the ordinary rows is adopted over the overflowing ones, and
    only queries at a finite distance from the entry vector are in the contract."""
    n = n or (500 if family == "l2_overflow" else 800)
    if family == "l2_overflow":
        base, _ = vf.scaled(n, dim, nq=nq)
        rows, q, big_rows, big_q = vf.l2_overflow(n, dim, nq=nq)
        g = graph_over(base, dim, metric)
        oix = oracle.Index(rows, dim=dim, metric=metric, sum_mode=oracle.SUM_BLOCKED64)
        for l in range(g.layer_count):
            nodes, nb = g.layer(l)
            oix.push_layer(nodes, nb, nb.shape[1])
        entry = int(g.layer(0)[0][0])
        assert entry not in big_rows
        q = q[np.setdiff1d(np.arange(nq), big_q)]
        qids = np.setdiff1d(np.arange(0, n, 9), big_rows).astype(np.uint64)
    else:
        rows, q = vf.make(family, n, dim, nq=nq)
        oix = graph_over(rows, dim, metric)
        qids = np.arange(0, n, 9, dtype=np.uint64)
    store = ph.VectorStore(rows[:, :dim], metric=metric)
    gix = ph.Hnsw.from_layers(store, [oix.layer(l) for l in range(oix.layer_count)])
    return rows, q, qids, oix, store, gix


SEARCH_CASES = [(f, m, d) for (f, m) in FAMILY_METRIC for d in DIMS]


@pytest.mark.parametrize("family,metric,dim", SEARCH_CASES)
def test_search(family, metric, dim, monkeypatch):
    monkeypatch.setenv("PHNSW_HOST_CHUNKS", HOST_LISTS_WHOLE)
    rows, q, qids, oix, store, gix = search_pair(family, metric, dim)
    tag = "%s dim %d metric %d search" % (family, dim, metric)
    seen_neg = seen_inf_eval = False
    # l2_overflow: ef 6 is below the count of rows at +inf and probe_depth 9 pops +inf keys from the spill list; ef 600
    # is above n, so the queue is never full and what was evaluated but is not in the result was dropped, not pushed out
    for ef, pd in ((1, 2), (6, 9), (64, 2), (300, 2)) + (((600, 2),) if family == "l2_overflow" else ()):
        sp, spo = ph.SearchParameters(ef, ef, pd), (ef, ef, pd)
        cpu = oix.search(queries=q, sp=spo, stats=True)
        msg = "%s ef %d pd %d" % (tag, ef, pd)
        assert_same(gix.search_batch(queries=q, sp=sp, stats=True), cpu, msg + " Unstored")
        cpu_s = oix.search(qids=qids, sp=spo, exclude=qids, stats=True)
        assert_same(gix.search_batch(qids=qids, sp=sp, exclude=qids, stats=True), cpu_s, msg + " Stored + exclude")
        seen_neg |= bool((cpu[1] < 0).any())
        seen_inf_eval |= ef == 600 and bool((cpu[3][:, 0] > cpu[2]).any())
        if ef in (6, 64):
            for switch in ("PHNSW_NO_TINY", "PHNSW_TINY_VALU", "PHNSW_NO_LAT"):
                with monkeypatch.context() as mp:
                    mp.setenv(switch, "1")
                    assert_same(gix.search_batch(queries=q, sp=sp, stats=True), cpu, "%s %s=1" % (msg, switch))
                    assert_same(gix.search_batch(qids=qids, sp=sp, exclude=qids, stats=True), cpu_s, "%s Stored %s=1" % (msg, switch))
        assert np.isfinite(cpu[1]).all() and cpu[2].min() >= 1, msg
    if dim in (256, 768, 1536) and metric != 2:
        # The dense top layers are used on their own accord (no switch turns them on), and for these row lengths with a
        # dot metric their table is built by the K = 1 MFMA kernel: every search above without a switch took that path.
        # PHNSW_TINY_VALU=1 is its off switch (the packed-fma table kernel), PHNSW_NO_TINY=1 the per-hop path: the same
        # oracle bits were required with it on and off.  The report below is asked for ef 64, one of the two ef values the
        # switches were run at: which table kernel a launch takes depends on the store (metric, row length) and on there
        # being dense layers for that ef, which is what this call reports (ph_tiny_matrix_cores, tiny.hip).
        t, _, mfma = gix.dense_top_layers(64)
        assert t > 0 and mfma, tag + ": the dense top layers' table comes from the matrix cores"
        with monkeypatch.context() as mp:
            mp.setenv("PHNSW_TINY_VALU", "1")
            assert not gix.dense_top_layers(64)[2], tag
    if family in ("scaled", "wide") and metric != 2:
        assert seen_neg, tag + ": negative distances in the checked results"
    if family == "l2_overflow":
        # +inf is evaluated (more evaluations than results with the queue never full) and, as in the reference, never a
        # queue entry (priority_queue.rs:102-107): every result is finite, the padding is f32::MAX / EMPTY
        assert seen_inf_eval, tag


def test_search_topk_cut_on_l2_overflow(monkeypatch):
    """search_batch_topk with k < ef: out_len counts the finite entries only (a candidate at +inf is never a queue entry,
    priority_queue.rs:102-107), min(len, k) of them; what lies behind is f32::MAX / EMPTY through the cut"""
    monkeypatch.setenv("PHNSW_HOST_CHUNKS", HOST_LISTS_WHOLE)
    for dim in (100, 768):
        rows, q, qids, oix, store, gix = search_pair("l2_overflow", 2, dim)
        ci, cd, cl = oix.search(queries=q, sp=(600, 600, 2))
        assert (cl < 600).all()  # ef above n: every list ends before ef; what is behind it is padding, not +inf
        for k in (1, 10, 64):
            gi, gd, gl = gix.search_batch(queries=q, sp=ph.SearchParameters(600, 600, 2), k=k)
            msg = "l2_overflow dim %d metric 2 search_batch_topk k %d" % (dim, k)
            np.testing.assert_array_equal(gl, np.minimum(cl, k), err_msg=msg)
            np.testing.assert_array_equal(gi, ci[:, :k], err_msg=msg)
            np.testing.assert_array_equal(bits(gd), bits(cd[:, :k]), err_msg=msg)
            for i in range(len(q)):
                assert (gi[i, int(gl[i]):] == ph.EMPTY).all() and (bits(gd[i, int(gl[i]):]) == bits(oracle.FMAX)).all(), msg


# ---------------------------------------------------------------- c: build
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("family,dim", [("lattice1", 8), ("scaled", 100), ("tiny", 100)])
def test_build_equals_the_oracle(family, dim, metric):
    """row merges, match_within_epsilon self-hits and promotion thresholds on distances that are exact ties, far from 0,
    or all equal"""
    n = 1500
    rows, _ = vf.make(family, n, dim, nq=4)
    kw = dict(seed=3, max_link_rounds=2, promote=1, order=6, neighborhood_size=6, zero_layer_neighborhood_size=12)
    oix = oracle.Index.generate(rows, np.arange(n), oracle.default_build_params(**kw), dim=dim, metric=metric,
                                sum_mode=oracle.SUM_BLOCKED64)
    g = ph.Hnsw.generate(ph.VectorStore(rows[:, :dim], metric=metric), np.arange(n, dtype=np.uint64), ph.BuildParameters(**kw))
    msg = "%s dim %d metric %d build" % (family, dim, metric)
    assert g.layer_count() == oix.layer_count, msg
    for l in range(oix.layer_count):
        nodes, nb = oix.layer(l)
        np.testing.assert_array_equal(g._layer(l).nodes, nodes, err_msg="%s layer %d nodes" % (msg, l))
        np.testing.assert_array_equal(g._layer(l).neighbors, nb, err_msg="%s layer %d neighbours" % (msg, l))


# ---------------------------------------------------------------- d: brute force
# n = 16 = k, and n not a multiple of 64; lattice1 ([-1, 1]) is for small dims, where nearly every distance ties
BF_SHAPES = ((16, 6), (100, 3), (333, 100), (1000, 256), (700, 260), (333, 768), (200, 1536))
BF_SHAPES_LATTICE1 = ((16, 6), (100, 3), (333, 6), (1000, 3))


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("family", FAMILIES + ["lattice1"])
def test_bruteforce_topk(family, metric):
    for n, dim in BF_SHAPES_LATTICE1 if family == "lattice1" else BF_SHAPES:
        rows, q = vf.make(family, n, dim, nq=70)
        store = ph.VectorStore(rows[:, :dim], metric=metric)
        oix = oracle.Index(rows, dim=dim, metric=metric)
        for k in (1, 10, 16):
            msg = "%s n %d dim %d metric %d bruteforce_topk k %d" % (family, n, dim, metric, k)
            gi, gd = store.bruteforce_topk(q, k)
            ci, cd = oix.bruteforce(q, k, sum_mode=oracle.SUM_SEQFMA)
            np.testing.assert_array_equal(gi, ci, err_msg=msg + " (ids, oracle SUM_SEQFMA)")
            np.testing.assert_array_equal(bits(gd), bits(cd), err_msg=msg + " (distance bits, oracle SUM_SEQFMA)")
            if family.startswith("lattice"):
                ti, td = vf.topk64(rows, q, metric, k)
                np.testing.assert_array_equal(gi, ti, err_msg=msg + " (ids, topk64)")
                np.testing.assert_array_equal(bits(gd), bits(td), err_msg=msg + " (distance bits, topk64)")


# ---------------------------------------------------------------- e: f16 store
@pytest.mark.parametrize("metric", METRICS)
def test_f16_store_on_the_lattice_returns_the_f32_bits(metric, monkeypatch):
    """integers up to 2048 are exact in binary16: the f16 store over the same graph is the f32 store"""
    monkeypatch.setenv("PHNSW_HOST_CHUNKS", HOST_LISTS_WHOLE)
    for dim in (6, 100, 256, 768):
        rows, q, qids, oix, store, gix = search_pair("lattice", metric, dim)
        f16 = ph.F16Store.from_full(store)
        np.testing.assert_array_equal(bits(f16.read()), bits(rows[:, :dim]))
        hix = ph.Hnsw.from_layers(f16, [oix.layer(l) for l in range(oix.layer_count)])
        msg = "lattice dim %d metric %d f16 store" % (dim, metric)
        ids = np.arange(rows.shape[0], dtype=np.uint64)
        np.testing.assert_array_equal(bits(np.stack([f16.compare_vec(ph.Unstored(x), ids) for x in q[:6]])),
                                      bits(vf.ref32(rows, q[:6], metric)), err_msg=msg + " distance_batch")
        for ef in (6, 64):
            assert_same(hix.search_batch(queries=q, sp=ph.SearchParameters(ef, ef, 2), stats=True),
                        oix.search(queries=q, sp=(ef, ef, 2), stats=True), "%s search ef %d" % (msg, ef))
            assert_same(hix.search_batch(qids=qids, sp=ph.SearchParameters(ef, ef, 2), exclude=qids, stats=True),
                        oix.search(qids=qids, sp=(ef, ef, 2), exclude=qids, stats=True), "%s Stored search ef %d" % (msg, ef))


@pytest.mark.parametrize("metric", METRICS)
def test_f16_search_and_rerank_on_scaled(metric, monkeypatch):
    """phnsw_f16_search_batch == the oracle's search over the rounded rows, then distances from the f32 rows, sorted by
    (d, id), first k (the helper of test_gpu_f16.py)"""
    from test_gpu_f16 import reranked_by_oracle
    monkeypatch.setenv("PHNSW_HOST_CHUNKS", HOST_LISTS_WHOLE)
    dim, k, ef = 100, 10, 64
    rows, q, qids, oix, store, gix = search_pair("scaled", metric, dim)
    f16 = ph.F16Store.from_full(store)
    held = f16.read()
    layers = [oix.layer(l) for l in range(oix.layer_count)]
    hix = ph.Hnsw.from_layers(f16, layers)
    o16 = oracle.Index(held, metric=metric, sum_mode=oracle.SUM_BLOCKED64)
    for nodes, nb in layers:
        o16.push_layer(nodes, nb, nb.shape[1])
    ofull = oracle.Index(rows, dim=dim, metric=metric)
    gi, gd, gl = hix.search_batch_reranked(store, q, ph.SearchParameters(ef, ef, 2), k)
    wi, wd, wl = reranked_by_oracle(o16, ofull, rows[:, :dim], q, (ef, ef, 2), k)
    msg = "scaled dim %d metric %d f16 search + re-rank" % (dim, metric)
    np.testing.assert_array_equal(gl, wl, err_msg=msg)
    for i in range(len(q)):
        np.testing.assert_array_equal(gi[i, :int(wl[i])], wi[i, :int(wl[i])], err_msg=msg)
        np.testing.assert_array_equal(bits(gd[i, :int(wl[i])]), bits(wd[i, :int(wl[i])]), err_msg=msg)
    if metric != 2:
        assert (wd < 0).any(), msg


# ---------------------------------------------------------------- f: PQ lookup tables
def ring(n):
    """one layer in which node i sees i - 1 and i + 1: with ef = n a search evaluates every node"""
    i = np.arange(n, dtype=np.uint64)
    return [(i, np.stack([(i + n - 1) % n, (i + 1) % n], axis=1).astype(np.uint64))]


def pq_pair(rows, dim, metric, m, ksub, mode, seed=0):
    full = ph.VectorStore(rows[:, :dim], metric=metric)
    pq = ph.PqStore(full, m, ksub, seed)
    codes, cb = oracle.pq_create(rows, dim, m, ksub, seed)
    np.testing.assert_array_equal(bits(pq.codebook()), bits(cb))
    np.testing.assert_array_equal(pq.codes(), codes)
    oix = oracle.Index(rows, dim=dim, metric=metric, sum_mode=oracle.SUM_BLOCKED64)
    oix.set_pq(codes, cb, table_f16=(mode == 1))
    if mode:
        pq.set_table_mode(mode)
        oracle.lib().orc_index_set_pq_table_f16(oix.h, mode)
    n = rows.shape[0]
    for nodes, nb in ring(n):
        oix.push_layer(nodes, nb, 2)
    return full, pq, codes, cb, oix, ph.Hnsw.from_layers(pq, ring(n))


@pytest.mark.parametrize("metric", METRICS)
def test_pq_mode0_on_the_lattice_is_f64_over_the_reconstructions(metric, monkeypatch):
    """random_centroids picks rows (pq.rs:261-285), so the centroids are integer valued: every table entry and every sum
    of entries is exact, whatever the order"""
    monkeypatch.setenv("PHNSW_HOST_CHUNKS", HOST_LISTS_WHOLE)
    n, dim, m, ksub = 240, 64, 16, 32
    rows, q = vf.lattice(n, dim, nq=8)
    full, pq, codes, cb, oix, gix = pq_pair(rows, dim, metric, m, ksub, 0)
    assert (cb == np.rint(cb)).all()
    rec = np.ascontiguousarray(cb[np.arange(m)[None, :], codes].reshape(n, dim))
    ids = np.arange(n, dtype=np.uint64)
    got = np.stack([pq.compare_vec(ph.Unstored(x), ids) for x in q] + [pq.compare_vec(ph.Stored(5), ids)])
    want = vf.ref32(rec, np.concatenate([q, rec[5:6]]), metric)
    np.testing.assert_array_equal(bits(got), bits(want), err_msg="lattice dim %d metric %d PQ mode 0" % (dim, metric))
    assert_same(gix.search_batch(queries=q, sp=ph.SearchParameters(n, n, 2), stats=True),
                oix.search(queries=q, sp=(n, n, 2), stats=True), "lattice metric %d PQ mode 0 search" % metric)


@pytest.mark.parametrize("metric", METRICS)
def test_pq_mode2_degenerate_table(metric, monkeypatch):
    """n rows that repeat one vector: the codebook rows of every sub-space are identical, widest == 0, scale == 0, every
    entry 0: each distance is the metric of `bias` alone -- the oracle's, and f64 over the one reconstruction"""
    monkeypatch.setenv("PHNSW_HOST_CHUNKS", HOST_LISTS_WHOLE)
    n, dim, m, ksub = 120, 32, 8, 16
    one, q = vf.lattice(1, dim, nq=6)
    rows = np.repeat(one, n, axis=0)
    full, pq, codes, cb, oix, gix = pq_pair(rows, dim, metric, m, ksub, 2)
    assert (cb == cb[:, :1]).all()
    ids = np.arange(n, dtype=np.uint64)
    got = np.stack([pq.compare_vec(ph.Unstored(x), ids) for x in q])
    want = np.repeat(vf.ref32(one, q, metric), n, axis=1)   # integer table: bias is exact
    np.testing.assert_array_equal(bits(got), bits(want), err_msg="degenerate PQ mode 2 metric %d" % metric)
    assert_same(gix.search_batch(queries=q, sp=ph.SearchParameters(n, n, 2), stats=True),
                oix.search(queries=q, sp=(n, n, 2), stats=True), "degenerate PQ mode 2 metric %d search" % metric)


def test_pq_mode1_entries_past_the_largest_half(monkeypatch):
    """scaled L2 rows whose squared sub-distances exceed 65504: the binary16 table entry is +inf, the distance +inf, and
    -- pinned to the oracle's f16-table mode -- such a candidate never enters the queue"""
    monkeypatch.setenv("PHNSW_HOST_CHUNKS", HOST_LISTS_WHOLE)
    n, dim, m, ksub = 300, 64, 16, 32
    rows, q = vf.scaled(n, dim, nq=24)
    full, pq, codes, cb, oix, gix = pq_pair(rows, dim, 2, m, ksub, 1)
    cpu = oix.search(queries=q, sp=(n, n, 2), stats=True)
    assert (cpu[2] < n).any() and (cpu[2] > 0).any()   # some entries overflowed, some queries still see finite ones
    keep = cpu[2] > 0   # an entry vector at +inf: the reference panics (lib.rs:181), outside the contract
    gpu = gix.search_batch(queries=q[keep], sp=ph.SearchParameters(n, n, 2), stats=True)
    assert_same(gpu, [x[keep] for x in cpu], "scaled dim %d metric 2 PQ mode 1 search" % dim)
    assert np.isfinite(gpu[1]).all()
