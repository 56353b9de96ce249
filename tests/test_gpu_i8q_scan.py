"""The exhaustive int8 scan over an i8q store (phnsw_i8q_scan_topk / _search, scan_i8q.hip) against tests/i8q_reference.py
over the store's own codes and scales (phnsw_i8_read): plain numpy, int64 dot products and two f32 multiplies.  An integer
sum has no order, so every comparison is bit for bit, with no tolerance, on any data.  On the parent commit every case
fails for want of the symbol."""
import functools

import numpy as np
import pytest
import torch

import parallel_hnsw_amd as ph
from parallel_hnsw_amd.hnsw import _p, check, lib

import bits_reference as br
import i8q_reference as ref
from test_gpu_i8 import bits
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -7
COS, DOT, L2 = br.METRIC_COSINE_HALF, br.METRIC_ONE_MINUS_DOT, br.METRIC_L2
EMPTY, FMAX = np.uint64(0xFFFFFFFFFFFFFFFF), np.finfo(np.float32).max
# (dim, metric, n, r, nq): 6 is one partial step, 100 ragged; n = 1, a last row group of one row (17, 4097), n < r, r = 1,
# r = 1024; 70 and 130 queries are more than one tile of 64 with a partial last one (a wave with no query at 70)
CASES = [(6, COS, 1, 1, 70), (6, DOT, 17, 1024, 130), (64, COS, 17, 1, 130), (64, DOT, 1000, 10, 130), (100, DOT, 1000, 65, 130),
         (100, COS, 17, 20, 70), (768, COS, 4097, 100, 70), (768, DOT, 17, 10, 70), (1536, DOT, 1500, 1024, 70), (1536, COS, 1, 5, 70)]


def reference(q, st, metric, r):
    ids_l, ds_l = ref.ranked(ref.matrix(q, st.codes(), st.scales(), metric))
    nq, m = len(q), min(r, st.n)
    ids, d = np.full((nq, r), EMPTY, dtype=np.uint64), np.full((nq, r), FMAX, dtype=np.float32)
    for i in range(nq):
        ids[i, :m], d[i, :m] = ids_l[i][:m], ds_l[i][:m]
    return ids, d, np.full(nq, m, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def world(dim, metric, n, nq):
    """Gaussian rows, every fifth row of the upper half a copy of a row of the lower half: equal distances"""
    rng = np.random.default_rng(dim * 7 + n)
    rows, q = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((nq, dim)).astype(np.float32)
    dup = np.arange(n // 2, n, 5)
    rows[dup] = rows[dup - n // 2]
    full = ph.VectorStore(rows, metric=metric)
    return q, full, ph.I8QStore.from_full(full)


def same(got, want):
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]))


@pytest.mark.parametrize("dim,metric,n,r,nq", CASES)
def test_gaussian_rows_bit_for_bit(dim, metric, n, r, nq):
    q, _, st = world(dim, metric, n, nq)
    same(st.scan(q, r), reference(q, st, metric, r))


@pytest.mark.parametrize("metric", [COS, DOT])
def test_saturated_rows_bit_for_bit(metric):
    rng = np.random.default_rng(11)
    rows, c, _ = ref.saturated(200, 1536, rng)
    q, cq, _ = ref.saturated(70, 1536, rng)
    ref.assert_saturated(ref.idots(cq, c))  # dot products past 2^24, odd ones among them
    st = ph.I8QStore.from_full(ph.VectorStore(rows, metric=metric))
    np.testing.assert_array_equal(st.codes(), c)
    same(st.scan(q, 100), reference(q, st, metric, 100))


@pytest.mark.parametrize("metric", [COS, DOT])
def test_queries_on_the_quantisers_edges(metric):
    edges = ref.quantiser_edges(100)
    rows = np.random.default_rng(3).standard_normal((200, 100))
    for row_scale in sorted({e[4] for e in edges}):
        st = ph.I8QStore.from_full(ph.VectorStore((rows * row_scale).astype(np.float32), metric=metric))
        q = np.stack([e[1] for e in edges if e[4] == row_scale])
        same(st.scan(q, 50), reference(q, st, metric, 50))


def test_result_does_not_depend_on_tile_or_slices(monkeypatch):
    q, _, st = world(768, COS, 4097, 70)
    want = reference(q, st, COS, 100)
    for slices in ("1", "5", "16"):
        for tile in ("16", "32"):  # (64 rows: held to 32 at this dimension)
            with env(monkeypatch, PHNSW_I8Q_SCAN_SLICES=slices, PHNSW_I8Q_SCAN_TILE=tile):
                same(st.scan(q, 100), want)
    with env(monkeypatch, PHNSW_I8Q_SCAN_SLICES="5", PHNSW_I8Q_SCAN_TILE="64"):  # a tile of four groups
        q64, _, st64 = world(64, DOT, 1000, 130)
        same(st64.scan(q64, 10), reference(q64, st64, DOT, 10))


@pytest.mark.parametrize("dim,r,k", [(768, 64, 10), (100, 10, 10)])
def test_scan_search_is_the_rerank_of_the_reference_candidates(dim, r, k):
    q, full, st = world(dim, DOT, 1000, 70)
    ids, _, ln = reference(q, st, DOT, r)
    full_d = [full.compare_vec(q[i], ids[i][:int(ln[i])]) for i in range(len(q))]
    want = br.rerank(ids, ln, full_d, k)
    same(st.scan_search(full, q, r, k), want)
    # the device form on a stream of its own: rows of stride r, the first k live
    nq, dev = len(q), torch.device("cuda")
    qd = torch.zeros((nq, full.ld), dtype=torch.float32, device=dev)
    qd[:, :dim] = torch.from_numpy(q).to(dev)
    oid, od = torch.zeros((nq, r), dtype=torch.int32, device=dev), torch.zeros((nq, r), dtype=torch.float32, device=dev)
    oln, stream = torch.zeros(nq, dtype=torch.int32, device=dev), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    st.scan_search_device(full, nq, r, k, qd.data_ptr(), full.ld, oid.data_ptr(), od.data_ptr(), oln.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    got = (oid.cpu().numpy()[:, :k].astype(np.uint32).astype(np.uint64), od.cpu().numpy()[:, :k],
           np.minimum(oln.cpu().numpy().astype(np.uint64), np.uint64(k)))
    same(got, want)


@pytest.mark.parametrize("what", ["f32 as i8q", "i8 as i8q", "fp4 as i8q", "r 0", "r 1025", "k 0", "k r+1", "full n", "full metric",
                                  "NaN", "nq 0"])
def test_refusals_name_the_call(what):
    rows = np.random.default_rng(5).standard_normal((80, 24)).astype(np.float32)
    full = ph.VectorStore(rows, metric=COS)
    st, r, k, code = ph.I8QStore.from_full(full), 10, 5, E_INVALID
    if what.endswith("as i8q"):
        st = {"f32": full, "i8 ": ph.I8Store.from_full(full), "fp4": ph.FP4Store.from_full(full)}[what[:3]]
        code = E_UNSUPPORTED
    r = {"r 0": 0, "r 1025": 1025}.get(what, r)
    k = {"k 0": 0, "k r+1": r + 1}.get(what, k)
    other = {"full n": ph.VectorStore(rows[:79]), "full metric": ph.VectorStore(rows, metric=DOT)}.get(what, full)
    q = rows[:4].copy()
    if what == "NaN":
        q[2, 7] = np.nan
    ids, d, ln = np.full((4, 16), 7, dtype=np.uint64), np.zeros((4, 16), dtype=np.float32), np.zeros(4, dtype=np.uint64)
    nq = 0 if what == "nq 0" else 4
    calls = [("phnsw_i8q_scan_search", lambda: check(lib().phnsw_i8q_scan_search(st._h, other._h, _p(q), nq, r, k, _p(ids), _p(d), _p(ln))))]
    if what[0] != "k" and what[:4] != "full":
        calls.append(("phnsw_i8q_scan_topk", lambda: check(lib().phnsw_i8q_scan_topk(st._h, _p(q), nq, r, _p(ids), _p(d), _p(ln)))))
    for name, call in calls:
        if what == "nq 0":
            call()
            assert np.all(ids == 7)
            continue
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == code
        assert name in str(e.value) and (not what.endswith("as i8q") or what[:3].strip() in str(e.value))
