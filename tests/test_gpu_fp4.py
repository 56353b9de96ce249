"""The fp4 row store (quantiser and decoder: tests/fp4_reference.py).  Every result must equal -- ids, distance BITS, lengths,
counters -- the unchanged oracle over the decoded rows (what read() returns) in SUM_BLOCKED64 order.  No tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from parallel_hnsw_amd._lib import lib
from parallel_hnsw_amd.hnsw import _p

import exact_filter_reference as xr
import filter_reference as fr
import labeled_reference as lr
import radius_reference as rr
from fp4_reference import decode, quantize
from test_fp4_cpu import TABLE
from test_gpu_i8 import adopt, assert_same, bits, oracle_over
from test_gpu_i8q import env
from test_gpu_radius_exact import same as same_radius

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED, COS = -1, -7, oracle.METRIC_COSINE_HALF


@functools.lru_cache(maxsize=None)
def build_pair(n, dim, metric=COS):
    """f32 store, its graph, the fp4 store, the adopted index, the oracle over the decoded rows; changed by no test"""
    full = ph.VectorStore.synthetic(n, dim, seed=42, normalize=metric != oracle.METRIC_L2, metric=metric)
    g = ph.Hnsw.generate(full, np.arange(n, dtype=np.uint64), ph.BuildParameters(seed=1))
    fp4 = ph.FP4Store.from_full(full)
    return full, g, fp4, adopt(fp4, g), oracle_over(fp4, metric, g)


@pytest.mark.parametrize("dim", [4, 36, 256, 260, 768, 1536])
def test_codes_scales_and_read_equal_the_numpy_quantiser(dim):
    rng = np.random.default_rng(dim)
    rows = rng.standard_normal((67, dim)).astype(np.float32)
    b = min(dim, 32)
    ties = np.concatenate([TABLE, -TABLE[:15]])[:b]
    rows[1, :b] = 0.0                                   # a zero block (at dim 4: a zero row)
    rows[2, :b], rows[3, :b] = ties * 2.0 ** -3, ties * 2.0 ** 9
    rows[4, :b], rows[4, 0] = 1.0, 7.5 * 2.0 ** 5       # the block's maximum saturates
    rows[5, :b] = (rng.integers(-70000, 70001, size=b).astype(np.float64) * 2.0 ** -149).astype(np.float32)  # subnormals
    rows[6, :b], rows[6, 0] = 1.0e38, 3.4e38            # near FLT_MAX
    rows[7, ::2], rows[66, dim - 1] = -0.0, -3.0e38     # negative zeros; the last component of the last row
    fp4 = ph.FP4Store.from_full(ph.VectorStore(rows))
    codes, scales = quantize(rows)
    assert scales[1, 0] == 2 and scales[5, 0] == 2 and scales[6, 0] == 252 and (codes[4, 0] & 15) == 7
    np.testing.assert_array_equal(fp4.scales(), scales)
    np.testing.assert_array_equal(fp4.codes(), codes)
    held = fp4.read()
    np.testing.assert_array_equal(bits(held), bits(decode(codes, scales, dim)))
    np.testing.assert_array_equal(bits(fp4.read(first=17, count=40)), bits(held[17:57]))


@pytest.mark.parametrize("metric", [COS, oracle.METRIC_ONE_MINUS_DOT, oracle.METRIC_L2])
@pytest.mark.parametrize("dim", [36, 768, 1536])
def test_distance_batch_bit_exact(dim, metric):
    n, norm = 200, metric != oracle.METRIC_L2
    rows = oracle.synth_rows(0, n, dim, normalize=norm)[:, :dim].copy()
    rows[5] = 0.0
    fp4 = ph.FP4Store.from_full(ph.VectorStore(rows, metric=metric))
    held = fp4.read()
    ix = oracle.Index(held, metric=metric)
    q = oracle.synth_rows(2 ** 32, 1, dim, normalize=norm)[0, :dim]
    for query, qrow in ((ph.Unstored(q), q), (ph.Stored(3), held[3])):  # a stored query is its decoded row
        want = np.array([ix.distance(qrow, held[i], oracle.SUM_BLOCKED64) for i in range(n)], dtype=np.float32)
        np.testing.assert_array_equal(bits(fp4.compare_vec(query, np.arange(n, dtype=np.uint64))), bits(want))


@pytest.mark.parametrize("n,dim,ef,metric,stored", [(3000, 100, 64, COS, True), (3000, 768, 128, COS, False),
                                                    (2000, 32, 40, oracle.METRIC_L2, False)])
def test_search_parity_with_and_without_dense_tables(monkeypatch, n, dim, ef, metric, stored):
    full, g, fp4, hix, oix = build_pair(n, dim, metric)
    kw = dict(qids=np.arange(0, n, 23, dtype=np.uint64)) if stored else dict(
        queries=oracle.synth_rows(2 ** 32, 129, dim, normalize=metric != oracle.METRIC_L2)[:, :dim])
    want = oix.search(sp=(ef, ef, 2), stats=True, **kw)
    table = hix.search_batch(sp=ph.SearchParameters(ef, ef, 2), stats=True, **kw)
    assert_same(table, want)
    with env(monkeypatch, PHNSW_NO_TINY="1"):
        per_hop = hix.search_batch(sp=ph.SearchParameters(ef, ef, 2), stats=True, **kw)
    assert_same(per_hop, want)
    assert_same(per_hop, table)


def test_filtered_walk_exact_labeled_and_exact_radius():
    n, dim, nq, k = 3000, 100, 16, 10
    full, g, fp4, hix, oix = build_pair(n, dim)
    q = oracle.synth_rows(2 ** 32, nq, dim)[:, :dim].copy()
    D = fr.distance_rows(oix, queries=q, mode=oracle.SUM_BLOCKED64)
    allow = np.random.default_rng(1).random((nq, n)) < 0.3
    assert_same(hix.search_batch_filtered(queries=q, sp=ph.SearchParameters(64, 24, 2), allow=allow, stats=True),
                fr.search(oix, D, (64, 24, 2), allow=allow, layers=fr.layers_of(oix)))
    labels = (np.arange(n) * 7919 % 13).astype(np.uint32)
    want = np.arange(nq) % 13
    assert_same(hix.search_exact_labeled(queries=q, labels=ph.Labels(hix, labels), want=want, k=k),
                xr.exact_topk(D, lr.masks_of(labels, want), None, None, k))
    r = np.sort(D, axis=1)[:, 70]  # 70 rows inside, more than a wave's 64
    same_radius(hix.search_exact_radius(queries=q, radius=r), rr.exact_radius(D, r))


@pytest.mark.parametrize("k", [1, 10])
def test_rerank_is_the_search_rescored_on_the_f32_store_and_both_forms_agree(k):
    torch = pytest.importorskip("torch")
    n, dim, ef, nq = 3000, 100, 64, 60
    full, g, fp4, hix, oix = build_pair(n, dim)
    qp = oracle.synth_rows(2 ** 32, nq, dim)
    q = np.ascontiguousarray(qp[:, :dim])
    sp = ph.SearchParameters(ef, ef, 2)
    gi, gd, gl = hix.search_batch_reranked(full, q, sp, k)
    si, sd, sl = hix.search_batch(queries=q, sp=sp)
    for i in range(nq):
        c = si[i, :int(sl[i])]
        dd = full.compare_vec(ph.Unstored(q[i]), c)
        order = np.lexsort((c, dd + np.float32(0.0)))[:k]
        assert gl[i] == len(order)
        np.testing.assert_array_equal(gi[i, :len(order)], c[order])
        np.testing.assert_array_equal(bits(gd[i, :len(order)]), bits(dd[order]))
    dq = torch.from_numpy(qp).cuda()
    ids, ln, status = (torch.empty(s, dtype=torch.int32, device="cuda") for s in ((nq, ef), nq, nq))
    d = torch.empty((nq, ef), dtype=torch.float32, device="cuda")
    hix.search_batch_reranked_device(full, nq, sp, k, dq.data_ptr(), qp.shape[1], ids.data_ptr(), d.data_ptr(), ln.data_ptr(),
                                     status.data_ptr())
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    np.testing.assert_array_equal(ln.cpu().numpy().astype(np.uint64), gl)
    live = np.arange(ef)[None, :] < gl[:, None]
    np.testing.assert_array_equal(ids.cpu().numpy().view(np.uint32).astype(np.uint64)[live], gi[live[:, :k]])
    np.testing.assert_array_equal(bits(d.cpu().numpy())[live], bits(gd)[live[:, :k]])


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_store_rejects_infinities_and_nans(bad):
    torch = pytest.importorskip("torch")
    t = torch.ones((64, 24), dtype=torch.float32, device="cuda")
    full = ph.VectorStore.from_device(t.data_ptr(), 64, 24, 24, keepalive=t)
    t[5, 7] = float(bad)
    torch.cuda.synchronize()
    with pytest.raises(ph.PhnswError) as e:
        ph.FP4Store.from_full(full)
    assert e.value.code == E_INVALID


def test_refusals_by_name():
    full, g, fp4, hix, oix = build_pair(2000, 32, oracle.METRIC_L2)
    for src in (fp4, ph.I8Store.from_full(full)):  # a source that is not an f32 store
        with pytest.raises(ph.PhnswError) as e:
            ph.FP4Store.from_full(src)
        assert e.value.code == E_INVALID
    L, out, q, big_u64, big_f = lib(), C.c_uint64(), np.ones((4, 32), "f4"), np.zeros(2000 * 3, "u8"), np.zeros(2000 * 3, "f4")
    for name, call in (("phnsw_store_append", lambda: L.phnsw_store_append(fp4._h, _p(q), 4, C.byref(out))),
                       ("phnsw_knn", lambda: L.phnsw_knn(hix._h, 3, 2, _p(big_u64), _p(big_f), _p(big_u64)))):
        assert call() == E_UNSUPPORTED
        msg = (L.phnsw_last_error() or b"").decode()
        assert "fp4" in msg and name in msg, msg
