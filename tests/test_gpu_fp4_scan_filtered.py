"""The MXFP4 matrix-core scan over an allow-list (phnsw_fp4_scan_topk_filtered / _search_filtered, scan_fp4_filtered.hip):
the LIST form (one bitmap for the batch, compacted on the device) and the MASK form (a bitmap per query) against numpy f64
over tests/fp4_reference.py with the disallowed columns removed before the (distance, id) sort.  Every bitmap is handed
over packed, with every bit at or past n SET: those must be ignored.  On the parent commit every case fails for want of
the symbol."""
import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd.hnsw import _p, check, lib

import bits_reference as br
from test_gpu_fp4_scan import COS, DOT, E_INVALID, E_UNSUPPORTED, EMPTY, FMAX, L2, NQ, exact_reference, same, world
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

# (dim, metric, n, r, mask): allowed counts 0, 1, 15, 16, 17 and half, m < r, the last row alone, every row, and rows in
# each of the three turns of the prefix loop at 2188 words; n is never a multiple of 32
EXACT_CASES = [(6, DOT, 1000, 1, 0), (100, DOT, 1000, 65, 1), (100, COS, 1000, 65, 15), (768, COS, 1000, 1024, 16),
               (768, DOT, 1000, 65, 17), (1536, DOT, 1000, 1, "last"), (1536, COS, 1000, 10, 500), (6, COS, 1000, 10, "all"),
               (768, COS, 1000, 1024, "all"), (6, COS, 70001, 65, "turns"), (6, COS, 70001, 1024, 17)]


def mask(n, m, seed=3):
    """bool [n]: m random rows, or a named set"""
    rng, a = np.random.default_rng(seed), np.zeros(n, dtype=np.bool_)
    if m == "all":
        a[:] = True
    elif m == "last":
        a[n - 1] = True
    elif m == "turns":  # words 0, 1250 and 2187, and a sparse sample
        a[[3, 40000, n - 1]] = True
        a |= rng.random(n) < 0.01
    else:
        a[rng.choice(n, m, replace=False)] = True
    return a


def words(allow):
    """packed u32 words of a bool mask [n] or [nq, n], the bits at or past n set"""
    a = np.atleast_2d(allow)
    w = np.packbits(np.hstack([a, np.ones((a.shape[0], -a.shape[1] % 32), dtype=np.bool_)]), axis=1, bitorder="little").view("<u4")
    return w if allow.ndim == 2 else w[0]


def reference(s, r, metric, allow):
    """exact_reference of test_gpu_fp4_scan over each query's allowed columns (allow: bool [nq, n])"""
    nq = s.shape[0]
    ids = np.full((nq, r), EMPTY, dtype=np.uint64)
    d = np.full((nq, r), FMAX, dtype=np.float32)
    ln = np.zeros(nq, dtype=np.uint64)
    for i in range(nq):
        cols = np.nonzero(allow[i])[0]
        if len(cols):
            ci, cd, cl = exact_reference(s[i:i + 1, cols], r, metric)
            ln[i] = cl[0]
            ids[i, :int(cl[0])], d[i] = cols[ci[0, :int(cl[0])].astype(np.int64)], cd[0]
    return ids, d, ln


def both_forms(st, q, r, allow):
    """the LIST form and the MASK form with the same mask for every query"""
    return st.scan_filtered(q, r, words(allow)), st.scan_filtered(q, r, words(np.tile(allow, (len(q), 1))))


@pytest.mark.parametrize("dim,metric,n,r,m", EXACT_CASES)
def test_exact_inputs_bit_for_bit(dim, metric, n, r, m):
    _, q, _, st, s, _ = world(dim, metric, n)
    allow = mask(n, m)
    want = reference(s, r, metric, np.tile(allow, (NQ, 1)))
    for got in both_forms(st, q, r, allow):
        same(got, want)


def test_exact_inputs_a_mask_of_its_own_per_query():
    _, q, _, st, s, _ = world(768, COS, 1000)
    allow = np.random.default_rng(9).random((NQ, 1000)) < 0.5
    allow[0], allow[1] = False, mask(1000, "last")  # a query with no row, one with the last row alone
    same(st.scan_filtered(q, 65, words(allow)), reference(s, 65, COS, allow))


def test_result_does_not_depend_on_tile_or_slices(monkeypatch):
    _, q, _, st, s, _ = world(768, COS, 4097)
    allow, few = mask(4097, 2048), mask(4097, 20)
    want, want_few = reference(s, 100, COS, np.tile(allow, (NQ, 1))), reference(s, 100, COS, np.tile(few, (NQ, 1)))
    for knobs in [dict(PHNSW_FP4_SCAN_SLICES=sl, PHNSW_FP4_SCAN_TILE=t) for sl in ("1", "3") for t in ("16", "32")] + [{}]:
        with env(monkeypatch, **knobs):
            for got in both_forms(st, q, 100, allow):
                same(got, want)
    with env(monkeypatch, PHNSW_FP4_SCAN_SLICES="7"):  # ceil(20 / 16) = 2 row groups: five empty slices reach the merge
        for got in both_forms(st, q, 100, few):
            same(got, want_few)


@pytest.mark.parametrize("dim,n,r,metric", [(768, 1000, 10, COS), (100, 1000, 65, COS), (1536, 4097, 100, DOT)])
def test_gaussian_inputs_inside_the_summation_bound(dim, n, r, metric):
    _, q, _, st, s, A = world(dim, metric, n, exact=False)
    allow = np.random.default_rng(4).random(n) < 0.3
    half = 0.5 if metric == COS else 1.0
    ref = (1.0 - s) * half
    B = (dim * 2.0 ** -24 * A + 2.0 ** -23 * np.maximum(1.0, np.abs(s))) * half
    t = np.sort(ref[:, allow], axis=1)[:, r - 1:r]
    near = ((np.abs(ref - t) <= B) & allow).sum(axis=1) - 1  # beside the r-th allowed row itself
    print("allowed rows inside +-B of the r-th allowed distance, at most:", near.max(), " largest B:", B.max())
    assert near.max() <= 4  # the band cannot hide a wrong order
    for ids, d, ln in both_forms(st, q, r, allow):
        assert np.all(ln == r)
        for i in range(NQ):
            got = ids[i].astype(np.int64)
            assert len(set(got)) == r and np.all(allow[got])
            key = list(zip((d[i] + np.float32(0.0)).tolist(), got.tolist()))
            assert key == sorted(key)
            assert np.all(np.abs(d[i].astype(np.float64) - ref[i][got]) <= B[i][got])
            assert np.all(ref[i][got] <= t[i] + B[i][got])
            assert np.all(np.isin(np.nonzero((ref[i] < t[i] - B[i]) & allow)[0], got))
    for got in both_forms(st, q, r, mask(n, "all")):  # every bit set: the unfiltered scan, bit for bit
        same(got, st.scan(q, r))


@pytest.mark.parametrize("dim,r,k,per_query", [(768, 64, 10, False), (100, 10, 10, True)])
def test_scan_search_filtered_is_the_rerank_of_the_reference_candidates(dim, r, k, per_query):
    _, q, full, st, s, _ = world(dim, DOT, 1000)
    allow = np.random.default_rng(6).random((NQ, 1000) if per_query else 1000) < 0.3
    ids, _, ln = reference(s, r, DOT, allow if per_query else np.tile(allow, (NQ, 1)))
    full_d = [full.compare_vec(q[i], ids[i][:int(ln[i])]) for i in range(NQ)]
    same(st.scan_search_filtered(full, q, r, k, words(allow)), br.rerank(ids, ln, full_d, k))


@pytest.mark.parametrize("what", ["NULL filter", "stride 2 of 3", "L2", "f32 as fp4", "r 0", "nq 0"])
def test_refusals_name_the_call(what):
    rows = np.random.default_rng(5).standard_normal((80, 24)).astype(np.float32)
    full = ph.VectorStore(rows, metric=L2 if what == "L2" else COS)
    st = full if what == "f32 as fp4" else ph.FP4Store.from_full(full)
    code = E_UNSUPPORTED if what in ("L2", "f32 as fp4") else E_INVALID
    r, nq, stride = (0 if what == "r 0" else 10), (0 if what == "nq 0" else 4), (2 if what[:6] == "stride" else 0)
    q, w = rows[:4].copy(), np.full(12, 0xFFFFFFFF, dtype=np.uint32)
    pw = None if what == "NULL filter" else _p(w)
    ids, d, ln = np.full((4, 16), 7, dtype=np.uint64), np.zeros((4, 16), dtype=np.float32), np.zeros(4, dtype=np.uint64)
    for name, call in [
            ("phnsw_fp4_scan_topk_filtered",
             lambda: check(lib().phnsw_fp4_scan_topk_filtered(st._h, _p(q), nq, r, pw, stride, _p(ids), _p(d), _p(ln)))),
            ("phnsw_fp4_scan_search_filtered",
             lambda: check(lib().phnsw_fp4_scan_search_filtered(st._h, full._h, _p(q), nq, r, 5, pw, stride, _p(ids), _p(d), _p(ln))))]:
        if what == "nq 0":
            call()
            assert np.all(ids == 7)
            continue
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == code and name in str(e.value)
