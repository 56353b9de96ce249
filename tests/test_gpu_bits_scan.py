"""The exhaustive Hamming scan over a bits store (phnsw_bits_scan_topk / _search, scan_bits.hip), bit for bit against
tests/bits_reference.py: h = hamming(pack(rows), pack(q)), order = lexsort((ids, h))[:r], distance(h[order]).  No
tolerance and no recall threshold anywhere; on the parent commit every case fails for want of the symbol."""
import functools

import numpy as np
import pytest

import parallel_hnsw_amd as ph

import bits_reference as br
from test_gpu_i8 import bits
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -7
COS, DOT, L2 = br.METRIC_COSINE_HALF, br.METRIC_ONE_MINUS_DOT, br.METRIC_L2
EMPTY, FMAX = np.uint64(0xFFFFFFFFFFFFFFFF), np.finfo(np.float32).max
NQ = 37
# (dim, metric, n, r): every value of every axis, and the corners n < r, n = 1, r = 1
CASES = [(6, COS, 1000, 10), (6, DOT, 1000, 1024), (6, L2, 1000, 65), (6, COS, 1, 1), (6, L2, 63, 65),
         (100, COS, 1000, 65), (100, DOT, 65, 10), (100, L2, 1000, 1), (100, DOT, 1, 1024), (100, L2, 63, 10),
         (768, COS, 1000, 1024), (768, DOT, 1000, 10), (768, L2, 65, 65), (768, COS, 63, 1), (768, DOT, 1, 10),
         (1536, COS, 1000, 10), (1536, DOT, 63, 1024), (1536, L2, 1000, 65), (1536, L2, 65, 1), (1536, COS, 1, 65)]


@functools.lru_cache(maxsize=None)
def world(dim, metric, n):
    """rows (value edges first, exact duplicates among them), queries (-0.0, a negative subnormal, a NaN), the stores"""
    rng = np.random.default_rng(dim * 7 + n)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    edge = br.bit_edge_rows(dim)[:7][:n]
    rows[:len(edge)] = edge
    for i in range(9, n, 97):
        rows[i] = rows[(i * 5) % n]
    q = rng.standard_normal((NQ, dim)).astype(np.float32)
    q[0, 0], q[1, dim - 1], q[2, dim // 2] = -0.0, -2.0 ** -149, np.nan
    q[3] = rows[n - 1]
    full = ph.VectorStore(rows, metric=metric)
    return rows, q, full, ph.BitStore.from_full(full)


def reference(rows, q, r, metric):
    n, dim = rows.shape
    ids = np.full((len(q), r), EMPTY, dtype=np.uint64)
    d = np.full((len(q), r), FMAX, dtype=np.float32)
    words = br.pack(rows)
    for i, qw in enumerate(br.pack(q)):
        h = br.hamming(words, qw[None, :])
        order = np.lexsort((np.arange(n), h))[:r]
        ids[i, :len(order)], d[i, :len(order)] = order, br.distance(h[order], dim, metric)
    return ids, d, np.full(len(q), min(r, n), dtype=np.uint64)


def same(got, want):
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]))


@pytest.mark.parametrize("dim,metric,n,r", CASES)
def test_scan_equals_the_reference(dim, metric, n, r):
    rows, q, _, st = world(dim, metric, n)
    same(st.scan(q, r), reference(rows, q, r, metric))


def test_result_does_not_depend_on_tile_or_slices(monkeypatch):
    rows, q, _, st = world(768, COS, 4097)  # a last batch of one row
    want = reference(rows, q, 100, COS)
    for slices in ("1", "3"):
        for tile in ("1", "5", "16"):
            with env(monkeypatch, PHNSW_BITS_SCAN_SLICES=slices, PHNSW_BITS_SCAN_TILE=tile):
                same(st.scan(q, 100), want)


def test_device_form_equals_host_form():
    torch = pytest.importorskip("torch")
    _, q, full, st = world(768, COS, 1000)
    r, k = 65, 10
    qd = torch.zeros((NQ, full.ld + 4), dtype=torch.float32, device="cuda")
    qd[:, :768] = torch.from_numpy(q).cuda()
    stream = torch.cuda.Stream()
    for search, host in ((False, st.scan(q, r)), (True, st.scan_search(full, q, r, k))):
        ids = torch.zeros((NQ, r), dtype=torch.int32, device="cuda")
        d = torch.zeros((NQ, r), dtype=torch.float32, device="cuda")
        ln = torch.zeros(NQ, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        a = (NQ, r) + ((k,) if search else ()) + (qd.data_ptr(), qd.shape[1], ids.data_ptr(), d.data_ptr(), ln.data_ptr())
        (st.scan_search_device(full, *a, stream=stream.cuda_stream) if search else st.scan_device(*a, stream=stream.cuda_stream))
        stream.synchronize()
        live = k if search else r
        i32 = ids.cpu().numpy().view(np.uint32)[:, :live]
        same((np.where(i32 == 0xFFFFFFFF, EMPTY, i32.astype(np.uint64)), d.cpu().numpy()[:, :live],
              np.minimum(ln.cpu().numpy().astype(np.uint64), live)), host)


@pytest.mark.parametrize("r,k", [(64, 10), (1024, 1024), (10, 1)])
def test_scan_search_is_the_rerank_of_the_scans_own_rows(r, k):
    n, dim = 1000, 100
    rng = np.random.default_rng(r)
    # integer components: every f32 dot product is exact, so the f64 order below is the f32 order
    rows = rng.integers(-8, 9, (n, dim)).astype(np.float32)
    q = rng.integers(-8, 9, (NQ, dim)).astype(np.float32)
    full = ph.VectorStore(rows, metric=DOT)
    st = ph.BitStore.from_full(full)
    ids, _, ln = st.scan(q, r)
    full_d = [full.compare_vec(q[i], ids[i][:int(ln[i])]) for i in range(NQ)]
    got = st.scan_search(full, q, r, k)
    same(got, br.rerank(ids, ln, full_d, k))
    if r >= n:  # every row was a candidate: the exact f32 top-k
        d64 = 1.0 - q.astype(np.float64) @ rows.astype(np.float64).T
        for i in range(NQ):
            order = np.lexsort((np.arange(n), d64[i]))[:k]
            np.testing.assert_array_equal(got[0][i, :len(order)], order.astype(np.uint64))
            np.testing.assert_array_equal(got[1][i, :len(order)], d64[i][order].astype(np.float32))


@pytest.mark.parametrize("what", ["f32 as bits", "f16 as bits", "r 0", "r 1025", "k 0", "k r+1", "full n", "full metric",
                                  "full f16"])
def test_refusals_name_the_call(what):
    rows = np.random.default_rng(5).standard_normal((80, 24)).astype(np.float32)
    full = ph.VectorStore(rows)
    st, r, k, other, code = ph.BitStore.from_full(full), 10, 5, full, E_INVALID
    if what.endswith("as bits"):
        st, code = (full if what[:3] == "f32" else ph.F16Store.from_full(full)), E_UNSUPPORTED
    r = {"r 0": 0, "r 1025": 1025}.get(what, r)
    k = {"k 0": 0, "k r+1": r + 1}.get(what, k)
    other = {"full n": ph.VectorStore(rows[:79]), "full metric": ph.VectorStore(rows, metric=L2),
             "full f16": ph.F16Store.from_full(full)}.get(what, full)
    calls = [("phnsw_bits_scan_search", lambda: ph.BitStore.scan_search(st, other, rows[:4], r, k))]
    if what[0] != "k" and what[:4] != "full":
        calls.append(("phnsw_bits_scan_topk", lambda: ph.BitStore.scan(st, rows[:4], r)))
    for name, call in calls:
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == code
        assert name in str(e.value) and (code != E_UNSUPPORTED or what[:3] in str(e.value))
