"""The exhaustive MXFP4 scan on the block-scaled matrix cores (phnsw_fp4_scan_topk / _search, scan_fp4.hip) against
numpy f64 over tests/fp4_reference.py: rows and queries as decode(quantize(.)), s = q^ . x^, the metric's last step.
Exact inputs bit for bit, Gaussian inputs inside the first-order bound of an f32 summation.  On the parent commit every
case fails for want of the symbol."""
import functools

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd.hnsw import _p, check, lib

import bits_reference as br
import fp4_reference as fr
from test_gpu_i8 import bits
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -7
COS, DOT, L2 = br.METRIC_COSINE_HALF, br.METRIC_ONE_MINUS_DOT, br.METRIC_L2
EMPTY, FMAX = np.uint64(0xFFFFFFFFFFFFFFFF), np.finfo(np.float32).max
NQ = 37
# (dim, metric, n, r): every value of every axis, with n < r, n = 1, r = 1 and a last row group of one row
EXACT_CASES = [(6, COS, 1000, 10), (6, DOT, 17, 1024), (100, DOT, 1000, 65), (100, COS, 1, 1), (768, COS, 1000, 1024),
               (768, DOT, 15, 10), (1056, COS, 17, 65), (1056, DOT, 1000, 1), (1536, DOT, 1000, 10), (1536, COS, 15, 65)]


def exact_values(rng, n, dim):
    """decoded MXFP4 values the quantiser leaves as they are: grid magnitudes, component 0 of a block +-4 or +-6, the
    block times 2^0 or 2^1"""
    nb = (dim + 31) // 32
    x = rng.choice(fr.GRID, (n, nb, 32))
    x[:, :, 0] = rng.choice([4.0, 6.0], (n, nb))
    x *= rng.choice([-1.0, 1.0], x.shape) * rng.choice([1.0, 2.0], (n, nb, 1))
    return x.reshape(n, -1)[:, :dim].astype(np.float32)


def decoded(x):
    return fr.decode(*fr.quantize(x), x.shape[1]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def world(dim, metric, n, exact=True):
    rng = np.random.default_rng(1 if not exact else dim * 7 + n)
    rows, q = (exact_values(rng, n, dim), exact_values(rng, NQ, dim)) if exact else (
        rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((NQ, dim)).astype(np.float32))
    full = ph.VectorStore(rows, metric=metric)
    xh, qh = decoded(rows), decoded(q)
    if exact:
        assert np.array_equal(xh, rows) and np.array_equal(qh, q)
    return rows, q, full, ph.FP4Store.from_full(full), qh @ xh.T, np.abs(qh) @ np.abs(xh).T


def exact_reference(s, r, metric):
    """s exact and a multiple of 0.25 below 2^22: 1 - s rounds once, the halving is exact"""
    nq, n = s.shape
    ids = np.full((nq, r), EMPTY, dtype=np.uint64)
    d = np.full((nq, r), FMAX, dtype=np.float32)
    dist = (1.0 - s).astype(np.float32) / np.float32(2.0 if metric == COS else 1.0)
    for i in range(nq):
        order = np.lexsort((np.arange(n), dist[i]))[:r]
        ids[i, :len(order)], d[i, :len(order)] = order, dist[i][order]
    return ids, d, np.full(nq, min(r, n), dtype=np.uint64)


def same(got, want):
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]))


@pytest.mark.parametrize("dim,metric,n,r", EXACT_CASES)
def test_exact_inputs_bit_for_bit(dim, metric, n, r):
    _, q, _, st, s, _ = world(dim, metric, n)
    same(st.scan(q, r), exact_reference(s, r, metric))


def test_result_does_not_depend_on_tile_or_slices(monkeypatch):
    _, q, _, st, s, _ = world(768, COS, 4097)  # a last row group of one row
    want = exact_reference(s, 100, COS)
    for slices in ("1", "3"):
        for tile in ("16", "32"):
            with env(monkeypatch, PHNSW_FP4_SCAN_SLICES=slices, PHNSW_FP4_SCAN_TILE=tile):
                same(st.scan(q, 100), want)
    same(st.scan(q, 100), want)


@pytest.mark.parametrize("dim,n,r,metric", [(768, 1000, 10, COS), (768, 1000, 256, DOT), (100, 1000, 65, COS), (1536, 4097, 100, DOT)])
def test_gaussian_inputs_inside_the_summation_bound(dim, n, r, metric):
    _, q, _, st, s, A = world(dim, metric, n, exact=False)
    half = 0.5 if metric == COS else 1.0
    ref = (1.0 - s) * half
    B = (dim * 2.0 ** -24 * A + 2.0 ** -23 * np.maximum(1.0, np.abs(s))) * half
    t = np.sort(ref, axis=1)[:, r - 1:r]
    near = (np.abs(ref - t) <= B).sum(axis=1) - 1  # beside the r-th row itself
    print("rows inside +-B of the r-th distance, at most:", near.max(), " largest B:", B.max())
    assert near.max() <= 4  # the band cannot hide a wrong order
    ids, d, ln = st.scan(q, r)
    assert np.all(ln == r)
    worst = 0.0
    for i in range(NQ):
        got = ids[i].astype(np.int64)
        assert len(set(got)) == r
        key = list(zip((d[i] + np.float32(0.0)).tolist(), got.tolist()))
        assert key == sorted(key)
        err = np.abs(d[i].astype(np.float64) - ref[i][got])
        worst = max(worst, float((err / half / (2.0 ** -24 * A[i][got])).max()))
        assert np.all(err <= B[i][got])
        assert np.all(ref[i][got] <= t[i] + B[i][got])
        assert np.all(np.isin(np.nonzero(ref[i] < t[i] - B[i])[0], got))
    print("largest |error| / (2^-24 A):", worst, " (bound: dim =", dim, ")")


@pytest.mark.parametrize("dim,r,k", [(768, 64, 10), (100, 10, 10)])
def test_scan_search_is_the_rerank_of_the_reference_candidates(dim, r, k):
    _, q, full, st, s, _ = world(dim, DOT, 1000)
    ids, _, ln = exact_reference(s, r, DOT)
    full_d = [full.compare_vec(q[i], ids[i][:int(ln[i])]) for i in range(NQ)]
    same(st.scan_search(full, q, r, k), br.rerank(ids, ln, full_d, k))


@pytest.mark.parametrize("what", ["f32 as fp4", "bits as fp4", "L2", "r 0", "r 1025", "k 0", "k r+1", "full n", "full metric",
                                  "full f16", "NULL queries", "NULL ids", "nq 2^32", "NaN", "inf", "nq 0"])
def test_refusals_name_the_call(what):
    rows = np.random.default_rng(5).standard_normal((80, 24)).astype(np.float32)
    full = ph.VectorStore(rows, metric=L2 if what == "L2" else COS)
    st, r, k, code = ph.FP4Store.from_full(full), 10, 5, E_INVALID
    if what.endswith("as fp4"):
        st = full if what[:3] == "f32" else ph.BitStore.from_full(full)
    if what.endswith("as fp4") or what == "L2":
        code = E_UNSUPPORTED
    r = {"r 0": 0, "r 1025": 1025}.get(what, r)
    k = {"k 0": 0, "k r+1": r + 1}.get(what, k)
    other = {"full n": ph.VectorStore(rows[:79]), "full metric": ph.VectorStore(rows, metric=DOT),
             "full f16": ph.F16Store.from_full(full)}.get(what, full)
    q = rows[:4].copy()
    if what in ("NaN", "inf"):
        q[2, 7] = np.nan if what == "NaN" else -np.inf
    ids, d, ln = np.full((4, 16), 7, dtype=np.uint64), np.zeros((4, 16), dtype=np.float32), np.zeros(4, dtype=np.uint64)
    nq = {"nq 2^32": 1 << 32, "nq 0": 0}.get(what, 4)
    pq, pids = (None if what == "NULL queries" else _p(q)), (None if what == "NULL ids" else _p(ids))
    calls = [("phnsw_fp4_scan_search", lambda: check(lib().phnsw_fp4_scan_search(st._h, other._h, pq, nq, r, k, pids, _p(d), _p(ln))))]
    if what[0] != "k" and what[:4] != "full":
        calls.append(("phnsw_fp4_scan_topk", lambda: check(lib().phnsw_fp4_scan_topk(st._h, pq, nq, r, pids, _p(d), _p(ln)))))
    for name, call in calls:
        if what == "nq 0":
            call()
            assert np.all(ids == 7)
            continue
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == code
        assert name in str(e.value) and (not what.endswith("as fp4") or what[:3] in str(e.value))
