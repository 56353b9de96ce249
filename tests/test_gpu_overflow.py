"""The frontier spill list (the part of the reference's unbounded `visit_queue` that does not fit
the LDS queue, lib.rs:182-191) has a fixed capacity per resident wave; a query that outgrows it is
flagged and re-run with more room.  PHNSW_OVF_CAP forces a tiny list so that these paths run:
results must still equal the oracle's."""
import functools
import os

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import filter_reference as fr
from test_gpu_filter import device_search

pytestmark = pytest.mark.gpu


class tiny_spill:
    def __init__(self, cap):
        self.cap = cap

    def __enter__(self):
        os.environ["PHNSW_OVF_CAP"] = str(self.cap)

    def __exit__(self, *a):
        del os.environ["PHNSW_OVF_CAP"]


def test_search_reruns_overflowing_queries():
    import torch
    n, dim = 3000, 32
    rows = oracle.synth_rows(0, n, dim)
    oix = oracle.Index.generate(rows, np.arange(n), oracle.default_build_params(seed=1), dim=dim,
                                sum_mode=oracle.SUM_BLOCKED64)
    store = ph.VectorStore(rows[:, :dim])
    q = oracle.synth_rows(2 ** 32, 300, dim)[:, :dim]
    sp = (16, 16, 8)
    ci, cd, cl, cs = oix.search(queries=q, sp=sp, stats=True)
    with tiny_spill(8):
        g = ph.Hnsw.from_layers(store, [oix.layer(l) for l in range(oix.layer_count)])
        # the device entry point reports the overflow per query (status 5) and leaves the retry to the caller
        dev = torch.device("cuda", 0)
        qd = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
        ids = torch.empty((300, 16), dtype=torch.int32, device=dev)
        d = torch.empty((300, 16), dtype=torch.float32, device=dev)
        ln = torch.empty(300, dtype=torch.int32, device=dev)
        status = torch.empty(300, dtype=torch.int32, device=dev)
        g.search_batch_device(300, ph.SearchParameters(*sp), ids.data_ptr(), d.data_ptr(), ln.data_ptr(),
                              status.data_ptr(), queries=qd.data_ptr(), ldq=dim)
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        assert (st == 5).sum() > 0 and set(st.tolist()) <= {0, 5}
        ok = st == 0
        np.testing.assert_array_equal(ids.cpu().numpy()[ok].astype(np.uint64)[:, :1], ci[ok][:, :1])
        # the host entry point re-runs them with 8x the room until they fit
        g2 = ph.Hnsw.from_layers(store, [oix.layer(l) for l in range(oix.layer_count)])
        gi, gd, gl, gs = g2.search_batch(queries=q, sp=ph.SearchParameters(*sp), stats=True)
    np.testing.assert_array_equal(gi, ci)
    np.testing.assert_array_equal(gd.view(np.uint32), cd.view(np.uint32))
    np.testing.assert_array_equal(gl, cl)
    np.testing.assert_array_equal(gs, cs)


# ---- the host path's re-run of single queries with every staged field present: query rows that need padding (dim 30 in
# rows of 32), stored ids, exclude words, per-query bitmaps, counters, the instrumented index.  Expected values are
# the CPU side's throughout.
N30, DIM30, SP30, CAP30 = 3000, 30, (16, 16, 8), 8


@functools.lru_cache(maxsize=None)
def world30():
    """(oracle index, f32 store over the same rows, the graph's layers); made once, changed by no test"""
    rows = oracle.synth_rows(0, N30, DIM30)
    oix = oracle.Index.generate(rows, np.arange(N30), oracle.default_build_params(seed=1), dim=DIM30,
                                sum_mode=oracle.SUM_BLOCKED64)
    store = ph.VectorStore(rows[:, :DIM30])
    assert store.ld == 32
    return oix, store, [oix.layer(l) for l in range(oix.layer_count)]


def fresh(store, layers):
    """a workspace keeps the largest spill list it ever had: every call that must overflow gets a new index"""
    return ph.Hnsw.from_layers(store, layers)


def same_rows(got, want):
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(got[3], want[3])


def test_rerun_stages_stored_queries_exclude_filter_and_counters(monkeypatch):
    oix, store, layers = world30()
    sp = ph.SearchParameters(*SP30)
    qids = np.arange(7, N30, N30 // 300, dtype=np.uint64)[:300]
    assert len(qids) == 300
    allow = np.random.default_rng(2024).random((300, N30)) < 0.5
    D = fr.distance_rows(oix, qids=qids, mode=oracle.SUM_BLOCKED64)
    want_filtered = fr.search(oix, D, SP30, allow=allow, exclude=qids)
    want_plain = oix.search(qids=qids, sp=SP30, exclude=qids, stats=True)
    same_rows(fr.search(oix, D, SP30, allow=None, exclude=qids), want_plain)  # the restatement, on these very inputs
    with tiny_spill(CAP30):
        # the re-run loop runs: under this cap the device forms report overflow (status 5) and retry nothing
        for a in (allow, None):
            st = device_search(fresh(store, layers), sp, qids=qids, allow=a, exclude=qids)[4]
            assert (st == 5).sum() > 0 and set(st.tolist()) <= {0, 5}
        for chunks in (None, "64,16,100"):  # whole; then 16 + pieces of <= 100: re-run entries from both slots
            if chunks:
                monkeypatch.setenv("PHNSW_HOST_CHUNKS", chunks)
            same_rows(fresh(store, layers).search_batch_filtered(qids=qids, sp=sp, allow=allow, exclude=qids, stats=True),
                      want_filtered)
            same_rows(fresh(store, layers).search_batch(qids=qids, sp=sp, exclude=qids, stats=True), want_plain)


def test_rerun_stages_padded_raw_queries_for_the_instrumented_search():
    oix, store, layers = world30()
    sp = ph.SearchParameters(*SP30)
    q = oracle.synth_rows(2 ** 32, 300, DIM30)[:, :DIM30]
    ci, cd, cl, cx = oix.search_instrumented(queries=q, sp=SP30)
    with tiny_spill(CAP30):
        st = device_search(fresh(store, layers), sp, queries=q)[4]
        assert (st == 5).sum() > 0 and set(st.tolist()) <= {0, 5}
        gi, gd, gl, gx = fresh(store, layers).search_instrumented_batch(queries=q, sp=sp)
    np.testing.assert_array_equal(gl, cl)
    np.testing.assert_array_equal(gi, ci)
    np.testing.assert_array_equal(gd.view(np.uint32), cd.view(np.uint32))
    np.testing.assert_array_equal(gx, cx)


def test_build_reruns_overflowing_rounds():
    n, dim = 2500, 24
    store = ph.VectorStore.synthetic(n, dim, seed=42)
    bp = ph.BuildParameters(seed=5)
    ref = ph.Hnsw.generate(store, np.arange(n), bp)
    with tiny_spill(32):
        h = ph.Hnsw.generate(store, np.arange(n), bp)
    assert h.layer_count() == ref.layer_count()
    for a, b in zip(h.layers, ref.layers):
        np.testing.assert_array_equal(a.nodes, b.nodes)
        np.testing.assert_array_equal(a.neighbors, b.neighbors)
