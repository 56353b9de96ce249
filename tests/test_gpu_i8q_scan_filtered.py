"""The int8 matrix-core scan over an allow-list (phnsw_i8q_scan_topk_filtered / _search_filtered, scan_i8q_filtered.hip):
the LIST form (one bitmap for the batch, compacted on the device, the listed rows gathered through the LDS tile) and the
MASK form (a bitmap per query) against tests/i8q_reference.py over the store's own codes and scales, the disallowed columns
removed before the (distance, id) sort.  An integer sum has no order, so every comparison is bit for bit.  Every bitmap is
handed over packed, with every bit at or past n SET: those must be ignored.  On the parent commit every case fails for
want of the symbol."""
import functools

import numpy as np
import pytest
import torch

import parallel_hnsw_amd as ph
from parallel_hnsw_amd.hnsw import _p, check, lib

import bits_reference as br
import i8q_reference as ref
from test_gpu_fp4_scan_filtered import mask, words
from test_gpu_i8q import env
from test_gpu_i8q_scan import COS, DOT, E_INVALID, E_UNSUPPORTED, EMPTY, FMAX, same, world

pytestmark = pytest.mark.gpu

NQ = 70  # a partial query tile, and a wave with no query
# (dim, metric, r, allowed rows) at n = 1000, never a multiple of 32: counts around one and two row groups, m < r, the last
# row alone; 6 is one partial step, 768 the 13th step
CASES = [(6, COS, 1, 0), (6, DOT, 65, 1), (100, DOT, 65, 15), (100, COS, 1024, 16), (768, COS, 65, 17), (768, DOT, 1, 31),
         (768, COS, 1024, 33), (100, COS, 65, 500), (768, DOT, 65, "last"), (1536, DOT, 1024, 500)]


@functools.lru_cache(maxsize=None)
def distances(dim, metric, n):
    q, _, st = world(dim, metric, n, NQ)
    return ref.matrix(q, st.codes(), st.scales(), metric)


def reference(D, r, allow):
    """reference of test_gpu_i8q_scan over each query's allowed columns of the distances D (allow: bool [n] or [nq, n])"""
    nq, allow = len(D), np.broadcast_to(allow, D.shape)
    ids, d = np.full((nq, r), EMPTY, dtype=np.uint64), np.full((nq, r), FMAX, dtype=np.float32)
    ln = np.zeros(nq, dtype=np.uint64)
    for i in range(nq):
        cols = np.nonzero(allow[i])[0]
        ids_l, ds_l = ref.ranked(D[i:i + 1, cols])
        m = min(r, len(cols))
        ids[i, :m], d[i, :m], ln[i] = cols[ids_l[0][:m]], ds_l[0][:m], m
    return ids, d, ln


def both_forms(st, q, r, allow):
    """the LIST form and the MASK form with the same mask for every query"""
    return st.scan_filtered(q, r, words(allow)), st.scan_filtered(q, r, words(np.tile(allow, (len(q), 1))))


@pytest.mark.parametrize("dim,metric,r,m", CASES)
def test_gaussian_rows_bit_for_bit(dim, metric, r, m):
    q, _, st = world(dim, metric, 1000, NQ)
    allow = mask(1000, m)
    want = reference(distances(dim, metric, 1000), r, allow)
    for got in both_forms(st, q, r, allow):
        same(got, want)


def test_every_row_allowed_is_the_unfiltered_scan():
    q, _, st = world(768, COS, 1000, NQ)
    for got in both_forms(st, q, 65, mask(1000, "all")):
        same(got, st.scan(q, 65))


def test_a_mask_of_its_own_per_query():
    q, _, st = world(768, COS, 1000, NQ)
    allow = np.random.default_rng(9).random((NQ, 1000)) < 0.5
    allow[0], allow[1] = False, mask(1000, "last")  # a query with no row, one with the last row alone
    same(st.scan_filtered(q, 65, words(allow)), reference(distances(768, COS, 1000), 65, allow))


def test_result_does_not_depend_on_tile_or_slices(monkeypatch):
    q, _, st = world(768, COS, 4097, NQ)
    D, allow, few = distances(768, COS, 4097), mask(4097, 2048), mask(4097, 20)
    want = reference(D, 100, allow)
    for knobs in [dict(PHNSW_I8Q_SCAN_SLICES=sl, PHNSW_I8Q_SCAN_TILE=t) for sl in ("1", "5") for t in ("16", "32")]:
        with env(monkeypatch, **knobs):
            for got in both_forms(st, q, 100, allow):
                same(got, want)
    with env(monkeypatch, PHNSW_I8Q_SCAN_SLICES="7"):  # two row tiles of 16: five empty slices reach the merge
        for got in both_forms(st, q, 100, few):
            same(got, reference(D, 100, few))
    q64, _, st64 = world(64, DOT, 1000, NQ)
    with env(monkeypatch, PHNSW_I8Q_SCAN_TILE="64"):  # a tile of 64 positions over a list padded to 16: the clamp
        for m in (63, 65):
            for got in both_forms(st64, q64, 100, mask(1000, m)):
                same(got, reference(distances(64, DOT, 1000), 100, mask(1000, m)))


@pytest.mark.parametrize("dim,r,k,per_query", [(768, 64, 10, False), (100, 10, 10, True)])
def test_scan_search_filtered_is_the_rerank_of_the_reference_candidates(dim, r, k, per_query):
    q, full, st = world(dim, DOT, 1000, NQ)
    allow = np.random.default_rng(6).random((NQ, 1000) if per_query else 1000) < 0.3
    ids, _, ln = reference(distances(dim, DOT, 1000), r, allow)
    want = br.rerank(ids, ln, [full.compare_vec(q[i], ids[i][:int(ln[i])]) for i in range(NQ)], k)
    same(st.scan_search_filtered(full, q, r, k, words(allow)), want)
    if per_query:
        return
    # the device form on a stream of its own: rows of stride r, the first k live
    dev = torch.device("cuda")
    qd = torch.zeros((NQ, full.ld), dtype=torch.float32, device=dev)
    qd[:, :dim] = torch.from_numpy(q).to(dev)
    wd = torch.from_numpy(words(allow).view(np.int32)).to(dev)
    oid, od = torch.zeros((NQ, r), dtype=torch.int32, device=dev), torch.zeros((NQ, r), dtype=torch.float32, device=dev)
    oln, stream = torch.zeros(NQ, dtype=torch.int32, device=dev), torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    st.scan_search_filtered_device(full, NQ, r, k, qd.data_ptr(), full.ld, wd.data_ptr(), 0, oid.data_ptr(), od.data_ptr(),
                                   oln.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    same((oid.cpu().numpy()[:, :k].astype(np.uint32).astype(np.uint64), od.cpu().numpy()[:, :k],
          np.minimum(oln.cpu().numpy().astype(np.uint64), np.uint64(k))), want)


@pytest.mark.parametrize("what", ["NULL filter", "stride 2 of 3", "f32 as i8q", "r 0", "nq 0"])
def test_refusals_name_the_call(what):
    rows = np.random.default_rng(5).standard_normal((80, 24)).astype(np.float32)
    full = ph.VectorStore(rows, metric=COS)
    st = full if what == "f32 as i8q" else ph.I8QStore.from_full(full)
    code = E_UNSUPPORTED if what == "f32 as i8q" else E_INVALID
    r, nq, stride = (0 if what == "r 0" else 10), (0 if what == "nq 0" else 4), (2 if what[:6] == "stride" else 0)
    q, w = rows[:4].copy(), np.full(12, 0xFFFFFFFF, dtype=np.uint32)
    pw = None if what == "NULL filter" else _p(w)
    ids, d, ln = np.full((4, 16), 7, dtype=np.uint64), np.zeros((4, 16), dtype=np.float32), np.zeros(4, dtype=np.uint64)
    for name, call in [
            ("phnsw_i8q_scan_topk_filtered",
             lambda: check(lib().phnsw_i8q_scan_topk_filtered(st._h, _p(q), nq, r, pw, stride, _p(ids), _p(d), _p(ln)))),
            ("phnsw_i8q_scan_search_filtered",
             lambda: check(lib().phnsw_i8q_scan_search_filtered(st._h, full._h, _p(q), nq, r, 5, pw, stride, _p(ids), _p(d), _p(ln))))]:
        if what == "nq 0":
            call()
            assert np.all(ids == 7)
            continue
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == code and name in str(e.value)
