"""The exact top-k for a TABLE of allow-lists with a selector per query, grouped by bitmap on the device
(phnsw_search_exact_grouped[_device], filter_grouped.hip).  Every comparison is on ids, distance bits, lengths and
status, no tolerance anywhere.

Two yardsticks, both for every case, neither made by the code under test: tests/exact_filter_reference.py over the
oracle's ORC_SUM_BLOCKED64 distances of store.read() (lattice rows on i8q) with the per-query mask masks[allow_of], and the
existing scan, search_exact_filtered with that mask as per-query bitmaps, whose rows the new call promises bit for bit.

The worlds are those of tests/test_gpu_exact_shared.py (N = 5000, 157 bitmap words, n no multiple of 32, 40 copies of row
0 spread over the id range, 65 raw and 65 stored queries; query 0 is the duplicated row).  Groups of fewer than 32
queries run on the vector units at every dimension, groups of 32 and more on the matrix cores at 256 / 768 floats and on
i8q; the layouts below have both.  A batch may name a query of the world more than once (`pick`)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import filter_reference as fr
from test_gpu_exact_filter import DUPS, EMPTY, N, NW, mask, ring, same
from test_gpu_exact_shared import NQX, exactly, fetch, sworld
from test_gpu_i8 import bits, oracle_over
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

ALL = -1
WORDS = NW + 1  # what a group costs besides its list: the per-word offsets (group_plan.h)


# ---------------------------------------------------------------- group_plan.h and dense_plan.h restated
def rounds(counts, budget):
    """the rounds group_plan.h cuts groups with these candidate counts into: a round takes groups while
    4 * sum(count + nwords + 1) fits the budget, and always at least one"""
    out, g0 = [], 0
    while g0 < len(counts):
        words, g = counts[g0] + WORDS, g0 + 1
        while g < len(counts) and (words + counts[g] + WORDS) * 4 <= budget:
            words, g = words + counts[g] + WORDS, g + 1
        out.append((g0, g))
        g0 = g
    return out


def node_chunks(count, nodes=8192):
    return -(-count // nodes)


def pos_chunks(count, size, table_bytes, nodes=8192):
    stride = (min(count, nodes) + 63) // 64 * 64
    pos = max(1, min(table_bytes // (stride * 4), 1 << 20, size))
    return -(-size // pos)


def groups_of(allow_of, nb):
    """(sizes, keys) of the groups in the call's order: bitmaps ascending, then ALL (key nb)"""
    key = np.where(np.asarray(allow_of) < 0, nb, allow_of)
    keys = [g for g in range(nb + 1) if (key == g).any()]
    return [int((key == g).sum()) for g in keys], keys


# ---------------------------------------------------------------- the calls
def per_query(masks, allow_of):
    """bool [nq, N]: the mask of every query, all ones where the selector names no bitmap"""
    allow_of = np.asarray(allow_of)
    out = np.ones((len(allow_of), masks.shape[1]), dtype=bool)
    out[allow_of >= 0] = masks[allow_of[allow_of >= 0]]
    return out


def device_grouped(hix, k, masks, allow_of, queries=None, qids=None, exclude=None, stream=None, sync=True, stride=None,
                   words=None):
    """phnsw_search_exact_grouped_device with torch buffers -> ids u64, d, len u64, status (or the tensors, sync=False).
    allow_of: integers, -1 = FILTER_ALL, anything else as it stands (u32).  words: a packed table instead of masks"""
    import torch
    dev = torch.device("cuda", 0)
    keep = []

    def up(a, dt):
        t = torch.from_numpy(np.ascontiguousarray(a).view(dt) if dt is not None else np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t

    nq = len(queries) if queries is not None else len(qids)
    qd = qi = ex = ld = 0
    if queries is not None:
        ld = hix.store.ld
        qp = np.zeros((nq, ld), dtype=np.float32)
        qp[:, :queries.shape[1]] = queries
        qd = up(qp, None).data_ptr()
    else:
        qi = up(np.asarray(qids, dtype=np.uint32), np.int32).data_ptr()
    if exclude is not None:
        ex = up(np.asarray(exclude, dtype=np.uint32), np.int32).data_ptr()
    if words is None:
        words, stride = ph.hnsw.pack_allow_table(masks, hix.store.n)
    sel = np.asarray(allow_of, dtype=np.int64).copy()
    sel[sel == ALL] = ph.FILTER_ALL
    wd = up(words, np.int32).data_ptr()
    sd = up(sel.astype(np.uint32), np.int32).data_ptr()
    ids = torch.full((nq, k), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev)
    ln = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    status = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    hix.search_exact_grouped_device(nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd, ldq=ld,
                                    qids=qi, exclude=ex, allows=wd, allow_stride=stride, nallows=words.shape[0], allow_of=sd,
                                    stream=0 if stream is None else stream.cuda_stream)
    out = (ids, d, ln, status, keep)
    return fetch(out) if sync else out


def check(w, masks, allow_of, exclude=None, k=10, members=None, hix=None, device=True, forms=(0, 1), pick=None, scan=True):
    """raw (0) and stored (1) queries, host and device form, against both yardsticks.  Query i of the batch is query
    pick[i] of the world (default i); exclude has one entry per query of the BATCH.  Returns the host results by form."""
    hix = hix or w["hix"]
    allow_of = np.asarray(allow_of)
    pick = np.arange(len(allow_of)) if pick is None else np.asarray(pick)
    pq = per_query(masks, allow_of)
    out = {}
    for form in forms:
        kw, D = (dict(queries=w["q"][pick]), w["Dq"][pick]) if form == 0 else (dict(qids=w["qids"][pick]), w["Ds"][pick])
        ref = xr.exact_topk(D, pq, exclude, members, k)
        got = hix.search_exact_grouped(allows=masks, allow_of=allow_of, exclude=exclude, k=k, **kw)
        same(got, ref)
        if scan:
            same(got, hix.search_exact_filtered(allow=pq, exclude=exclude, k=k, **kw))
        assert (got[0][np.arange(k)[None, :] >= got[2][:, None]] == EMPTY).all()
        assert (bits(got[1])[np.arange(k)[None, :] >= got[2][:, None]] == bits(xr.FMAX)).all()
        if device:
            dv = device_grouped(hix, k, masks, allow_of, exclude=exclude, **kw)
            assert not dv[3].any()
            same(dv, ref)
        out[form] = got
    return out


@functools.lru_cache(maxsize=None)
def five():
    """five bitmaps with 0, 1, 65, about 1500 and all 5000 candidates; the copies of row 0 where they fit"""
    dense = mask(0.3, N, 41)
    dense[DUPS] = True
    m = np.stack([np.zeros(N, dtype=bool), exactly(1, 11), exactly(65, 12), dense, np.ones(N, dtype=bool)])
    m.setflags(write=False)
    return m


def shuffled(sizes_by_selector, seed):
    """selectors with the given multiplicities, scattered over the batch"""
    of = np.concatenate([np.full(c, s, dtype=np.int64) for s, c in sizes_by_selector])
    return of[np.random.default_rng(seed).permutation(len(of))]


# ---------------------------------------------------------------- 1: kinds and paths
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("f32", 256), ("f32", 768), ("f16", 24), ("i8", 256), ("i8q", 24),
                                      ("i8q", 256)])
def test_kinds_and_paths(kind, dim):
    w = sworld(kind, dim)
    masks = five()
    # six interleaved groups of 10 or 11 queries, never contiguous, each below 32: the vector units at every dimension
    of = np.arange(NQX) % 6
    of[of == 5] = ALL
    got = check(w, masks, of, k=64)
    counts = np.array([0, 1, 65, masks[3].sum(), N, N])
    for form in (0, 1):
        np.testing.assert_array_equal(got[form][2], np.minimum(counts[np.arange(NQX) % 6], 64))
    # one group of 33 (a partial position tile), one of exactly 32, one of 1; bitmaps 0 and 1 named by no query.  66
    # queries: the world's 65 and query 0 once more
    of = shuffled([(3, 33), (4, 32), (2, 1)], 5)
    assert groups_of(of, 5) == ([1, 33, 32], [2, 3, 4])
    check(w, masks, of, k=64, pick=np.arange(66) % NQX)


# ---------------------------------------------------------------- 2: chunks and rounds
def test_every_loop_turns_more_than_once(monkeypatch):
    w = sworld("f32", 256)
    dense = mask(0.3, N, 5)
    dense[DUPS] = True
    masks = np.stack([exactly(64, 1), exactly(65, 2), exactly(192, 3), dense, exactly(700, 4)])
    counts = [int(m.sum()) for m in masks]
    of = shuffled([(0, 8), (1, 8), (2, 33), (3, 8), (4, 8)], 7)
    assert groups_of(of, 5) == ([8, 8, 33, 8, 8], [0, 1, 2, 3, 4])
    base = check(w, masks, of, k=100)

    def again(device=True, **knobs):
        with env(monkeypatch, **knobs):
            now = check(w, masks, of, k=100, device=device, scan=False)
        for form in (0, 1):
            same(base[form], now[form])

    assert [node_chunks(c, 64) for c in counts[:3]] == [1, 2, 3]  # 64, 65 and 192 candidates in chunks of 64
    again(PHNSW_DENSE_NODES="64")
    table = 192 * 4 * 11  # eleven positions of the 192-candidate group's table: its 33 queries in three position chunks
    assert pos_chunks(192, 33, table) == 3 and pos_chunks(64, 8, table) == 1
    again(PHNSW_DENSE_TABLE_BYTES=str(table))
    assert pos_chunks(192, 33, table, 64) == 1 and pos_chunks(64, 33, 64 * 4 * 11, 64) == 3
    again(PHNSW_DENSE_NODES="64", PHNSW_DENSE_TABLE_BYTES=str(64 * 4 * 11), device=False)  # 3 node chunks x 3 position chunks
    budget = 4 * (max(counts) + WORDS)  # the largest group fits alone
    r = rounds(counts, budget)
    assert len(r) >= 3 and r[0][1] - r[0][0] > 1, r
    again(PHNSW_GROUP_LIST_BYTES=str(budget))
    assert rounds(counts, 1) == [(g, g + 1) for g in range(5)]  # every group exceeds it: at least one per round
    again(PHNSW_GROUP_LIST_BYTES="1", device=False)
    assert len(rounds(counts, 256 << 20)) == 1  # the default: one round


# ---------------------------------------------------------------- 3: the kept node operand
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("i8q", 256), ("i8q", 24)])
def test_two_bitmaps_of_equal_count_do_not_share_a_packed_operand(monkeypatch, kind, dim):
    """consecutive groups with two bitmaps of EQUAL candidate count in rounds of one group: the second list sits at the
    first one's address with its length, so a node operand kept under (address, length) would serve the first group's
    rows to the second"""
    w = sworld(kind, dim)
    perm = np.random.default_rng(3).permutation(N)
    perm = perm[~np.isin(perm, DUPS)]
    a, b = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    a[DUPS[:8]] = b[DUPS[:8]] = True
    a[perm[:692]] = True
    b[perm[692:1384]] = True
    assert a.sum() == b.sum() == 700 and (a & b).sum() == 8
    masks = np.stack([a, b])
    of = shuffled([(0, 33), (1, 32)], 9)
    budget = 4 * (700 + WORDS)
    assert rounds([700, 700], budget) == [(0, 1), (1, 2)]
    with env(monkeypatch, PHNSW_GROUP_LIST_BYTES=str(budget)):
        got = check(w, masks, of, k=10)
    for form in (0, 1):
        ids = got[form][0]
        assert np.isin(ids[of == 0], np.nonzero(a)[0]).all() and np.isin(ids[of == 1], np.nonzero(b)[0]).all()


# ---------------------------------------------------------------- 4: exclude and ties
@pytest.mark.parametrize("k", [1, 10, 64, 1024])
def test_exclude_and_ties(k):
    w = sworld("f32", 256)
    some = mask(0.1, N, 77)
    some[DUPS] = True  # all 40 copies
    few = exactly(300, 21)  # 8 of them
    masks = np.stack([some, few])
    of = np.arange(NQX) % 2
    pick = np.arange(NQX)
    pick[1] = 0  # query 0, the duplicated row, in both groups
    inside = [np.nonzero(m)[0] for m in masks]
    outside = [np.nonzero(~m)[0] for m in masks]
    ex = np.full(NQX, EMPTY, dtype=np.uint64)  # a candidate, a non-candidate, PHNSW_EMPTY, in turn
    for q in range(NQX):
        if q % 3 == 0:
            ex[q] = inside[of[q]][5 + q]
        elif q % 3 == 1:
            ex[q] = outside[of[q]][5 + q]
    ex[0] = EMPTY
    ex[1] = DUPS[3]  # a tied candidate leaves: the other seven stay in id order
    got = check(w, masks, of, exclude=ex, k=k, pick=pick, device=k in (1, 1024))
    for form in (0, 1):
        cand = np.array([masks[of[q]].sum() - (q % 3 == 0 and q > 0) - (q == 1) for q in range(NQX)])
        np.testing.assert_array_equal(got[form][2], np.minimum(cand, k))
        if k >= 64:  # nothing is nearer to a row than its copies, and ids decide among them
            np.testing.assert_array_equal(got[form][0][0, :40], DUPS.astype(np.uint64))
            np.testing.assert_array_equal(got[form][0][1, :7], np.delete(DUPS[:8], 3).astype(np.uint64))


# ---------------------------------------------------------------- 5: stride and garbage
def test_a_wider_stride_and_garbage_past_the_bitmaps():
    w = sworld("f32", 256)
    masks = five()
    of = np.arange(NQX) % 6
    of[of == 5] = ALL
    clean, stride = ph.hnsw.pack_allow_table(masks, N)
    assert stride == NW and clean.shape == (5, NW)
    dirty = np.full((5, NW + 3), 0xFFFFFFFF, dtype=np.uint32)  # three padding words per bitmap, all ones
    dirty[:, :NW] = clean
    dirty[:, NW - 1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)  # the bits at and past n of the last word
    base = check(w, masks, of, k=64, device=False)
    for form, kw in ((0, dict(queries=w["q"])), (1, dict(qids=w["qids"]))):
        same(w["hix"].search_exact_grouped(allows=dirty, allow_of=of, k=64, **kw), base[form])
        dv = device_grouped(w["hix"], 64, None, of, words=dirty, stride=NW + 3, **kw)
        same(dv, base[form])
        assert not dv[3].any()


# ---------------------------------------------------------------- 6: an index over part of its store
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("f32", 256), ("i8q", 256)])
def test_vectors_outside_the_index_are_never_candidates(kind, dim):
    w = sworld(kind, dim)
    masks = five()
    even = np.arange(N) % 2 == 0
    hix = ph.Hnsw.from_layers(w["store"], ring(np.arange(0, N, 2)))  # every second vector: vec2node is not the identity
    of = shuffled([(2, 10), (3, 33), (ALL, 22)], 13)
    got = check(w, masks, of, members=even, hix=hix, k=100)
    for form in (0, 1):
        assert not (got[form][0][got[form][0] != EMPTY] % 2).any()
        assert (got[form][2][of == ALL] == 100).all()


# ---------------------------------------------------------------- 7: what the device form reports
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("f32", 24), ("i8q", 256)])
def test_bad_ids_and_selectors_are_reported_and_harm_nobody(kind, dim):
    w = sworld(kind, dim)
    masks = five()
    of = shuffled([(2, 10), (3, 33), (ALL, 22)], 17)
    bad_id, bad_sel = [3, 17, 39], [5, 40, 64]
    sel = of.copy()
    sel[bad_sel] = [5, 0xFFFFFFFE, 5]  # == nfilters, and the largest value that is not FILTER_ALL
    qids = w["qids"].copy()
    qids[bad_id] = [N, N + 12345, 0xFFFFFFFE]
    ref = xr.exact_topk(w["Ds"], per_query(masks, of), None, None, 10)
    dv = device_grouped(w["hix"], 10, masks, sel, qids=qids)  # the outputs are pre-filled with garbage
    good = np.setdiff1d(np.arange(NQX), bad_id + bad_sel)
    same(tuple(x[good] for x in dv[:3]), tuple(x[good] for x in ref))
    assert (dv[3][bad_id] == 4).all() and (dv[3][bad_sel] == 6).all() and not dv[3][good].any()
    bad = bad_id + bad_sel
    assert (dv[0][bad] == EMPTY).all() and (bits(dv[1][bad]) == bits(xr.FMAX)).all() and not dv[2][bad].any()
    # raw queries: selectors alone
    dv = device_grouped(w["hix"], 10, masks, sel, queries=w["q"])
    ref = xr.exact_topk(w["Dq"], per_query(masks, of), None, None, 10)
    good = np.setdiff1d(np.arange(NQX), bad_sel)
    same(tuple(x[good] for x in dv[:3]), tuple(x[good] for x in ref))
    assert (dv[3][bad_sel] == 6).all() and not dv[3][good].any() and not dv[2][bad_sel].any()
    assert (dv[0][bad_sel] == EMPTY).all() and (bits(dv[1][bad_sel]) == bits(xr.FMAX)).all()
    # the host form refuses both before any device work and writes no output
    L = ph.lib()
    words, stride = ph.hnsw.pack_allow_table(masks, N)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for q64, s32, what in ((qids.astype(np.uint64), ph.hnsw.pack_allow_of(of, NQX), "stored query id"),
                           (w["qids"].astype(np.uint64), sel.astype(np.uint32), "query 5 selects bitmap 5")):
        ids = np.full((NQX, 10), 7, dtype=np.uint64)
        d = np.full((NQX, 10), -1.0, dtype=np.float32)
        ln = np.full(NQX, 7, dtype=np.uint64)
        rc = L.phnsw_search_exact_grouped(w["hix"]._h, None, ptr(q64), NQX, None, ptr(words), stride, 5, ptr(s32), 10, ptr(ids),
                                          ptr(d), ptr(ln))
        assert rc == -1 and what in L.phnsw_last_error().decode()
        assert (ids == 7).all() and (d == -1.0).all() and (ln == 7).all()


def test_a_refused_selector_beside_a_group_of_three_node_chunks(monkeypatch):
    """A selector outside the table puts its query into the reject group, which has no candidates: its row is written by
    the select over no table, whatever the other groups need -- here 130 candidates in three node chunks of 64."""
    w = sworld("f32", 256)
    masks = np.stack([exactly(130, 77)])
    sel = np.array([0, 0, 1, 0, 0])  # 1 == nfilters
    qids = w["qids"][:5]
    with env(monkeypatch, PHNSW_DENSE_NODES="64"):
        dv = device_grouped(w["hix"], 10, masks, sel, qids=qids)
    ref = xr.exact_topk(w["Ds"][:5], per_query(masks, np.zeros(5, dtype=np.int64)), None, None, 10)
    good = [0, 1, 3, 4]
    same(tuple(x[good] for x in dv[:3]), tuple(x[good] for x in ref))
    assert not dv[3][good].any() and (ref[2][good] == 10).all()
    assert dv[3][2] == 6 and dv[2][2] == 0
    assert (dv[0][2] == EMPTY).all() and (bits(dv[1][2]) == bits(xr.FMAX)).all()


# ---------------------------------------------------------------- 8: two streams, one stream twice
def test_calls_in_flight_on_two_streams_and_twice_on_one():
    import torch
    w = sworld("f32", 256)
    ma = five()
    mb = np.stack([mask(0.2, N, 32), exactly(700, 33), mask(0.02, N, 34)])
    oa = shuffled([(2, 10), (3, 33), (ALL, 22)], 19)
    ob = shuffled([(0, 33), (1, 20), (2, 12)], 20)
    one = xr.exact_topk(w["Dq"], per_query(ma, oa), None, None, 100)
    two = xr.exact_topk(w["Ds"], per_query(mb, ob), None, None, 100)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(2):
        o1 = device_grouped(w["hix"], 100, ma, oa, queries=w["q"], stream=s1, sync=False)
        o2 = device_grouped(w["hix"], 100, mb, ob, qids=w["qids"], stream=s2, sync=False)
        o3 = device_grouped(w["hix"], 100, ma, oa, queries=w["q"], stream=s1, sync=False)  # the same call again, same stream
        r1, r2, r3 = fetch(o1), fetch(o2), fetch(o3)
        same(r1, one)
        same(r2, two)
        same(r3, r1)
        assert not r1[3].any() and not r2[3].any() and not r3[3].any()


# ---------------------------------------------------------------- 9: a table of one bitmap
def test_one_bitmap_for_all_equals_the_shared_call():
    w = sworld("f32", 256)
    allow = mask(0.3, N, 51)
    got = check(w, allow[None, :], np.zeros(NQX, dtype=np.int64), k=100)
    same(got[0], w["hix"].search_exact_shared(queries=w["q"], allow=allow, k=100))
    same(got[1], w["hix"].search_exact_shared(qids=w["qids"], allow=allow, k=100))


# ---------------------------------------------------------------- 10: many small groups
@functools.lru_cache(maxsize=None)
def many_world():
    """600 raw and 600 stored queries on the N = 5000 f32 rows at 24 floats, the yardstick's distances; made once"""
    base = sworld("f32", 24)
    q = oracle.synth_rows(2 ** 34, 600, 24)[:, :24].copy()
    qids = np.random.default_rng(8).integers(0, N, 600).astype(np.uint64)
    oix = oracle_over(base["store"], oracle.METRIC_COSINE_HALF)
    return dict(store=base["store"], hix=base["hix"], q=q, qids=qids,
                Dq=fr.distance_rows(oix, queries=q, mode=oracle.SUM_BLOCKED64),
                Ds=fr.distance_rows(oix, qids=qids, mode=oracle.SUM_BLOCKED64))


def test_many_small_groups():
    w = many_world()
    rng = np.random.default_rng(10)
    masks = np.zeros((257, N), dtype=bool)
    for m in masks:
        m[rng.permutation(N)[:rng.integers(40, 61)]] = True
    of = np.arange(600) % 257  # more than one block of queries in the grouping pass, more than 256 groups
    got = check(w, masks, of, k=10)
    assert (got[0][2] == 10).all()


# ---------------------------------------------------------------- 11: L2, and the vector units forced
def test_l2():
    w = sworld("f32", 256, oracle.METRIC_L2)
    check(w, five(), shuffled([(2, 10), (3, 33), (ALL, 22)], 23), k=64)


def test_the_vector_unit_pass_gives_the_same_bits(monkeypatch):
    w = sworld("f32", 256)
    of = shuffled([(2, 10), (3, 33), (ALL, 22)], 29)
    base = check(w, five(), of, k=64)
    with env(monkeypatch, PHNSW_TINY_VALU="1"):
        now = check(w, five(), of, k=64, scan=False)
    for form in (0, 1):
        same(base[form], now[form])


# ---------------------------------------------------------------- 12: refusals, in the header's order
def test_refusals():
    w = sworld("f32", 24)
    hix, q = w["hix"], w["q"][:4]
    masks, of = five(), np.array([0, 1, 2, ALL])
    dev = dict(qids=8, allows=8, allow_stride=NW, nallows=5, allow_of=8)  # never dereferenced: refused before
    # a PQ store: after k, before everything else
    rows = oracle.synth_rows(0, 400, 32)[:, :32].copy()
    f2 = ph.VectorStore(rows, metric=ph.METRIC_L2)
    pix = ph.Hnsw.from_layers(ph.PqStore(f2, 16), ring(np.arange(400)))
    pmasks, pof = np.ones((2, 400), dtype=bool), np.array([0, 1])
    with pytest.raises(ph.PhnswError) as e:
        pix.search_exact_grouped(queries=rows[:2], allows=pmasks, allow_of=pof, k=0)
    assert e.value.code == -1 and "k must be 1..1024" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:
        pix.search_exact_grouped(queries=rows[:2], allows=pmasks, allow_of=pof, k=3)
    assert e.value.code == -7 and "phnsw_search_exact_grouped:" in str(e.value)  # PHNSW_E_UNSUPPORTED, naming the call
    with pytest.raises(ph.PhnswError) as e:  # ... before nq == 0 is a no-op, before the arguments are looked at
        pix.search_exact_grouped_device(0, 3, 0, 0, 0, 0)
    assert e.value.code == -7 and "phnsw_search_exact_grouped_device:" in str(e.value)
    for k in (0, 1025):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_grouped(queries=q, allows=masks, allow_of=of, k=k)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_grouped: k must be 1..1024 (got %d)" % k
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_grouped_device(4, k, 8, 8, 8, 8, **dev)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_grouped_device: k must be 1..1024 (got %d)" % k
    # nq == 0: a no-op, whatever the other arguments
    ids, d, ln = hix.search_exact_grouped(queries=np.zeros((0, 24), dtype=np.float32), allows=masks,
                                          allow_of=np.zeros(0, dtype=np.int64), k=3)
    assert ids.shape == (0, 3)
    hix.search_exact_grouped_device(0, 3, 0, 0, 0, 0)
    bad = [dict(dev, queries=16, ldq=24),  # queries and qids
           dict(dev, qids=0),              # neither
           dict(dev, allow_stride=0), dict(dev, allow_stride=NW - 1), dict(dev, nallows=0), dict(dev, allows=0),
           dict(dev, allow_of=0)]
    for kw in bad:
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_grouped_device(4, 3, 8, 8, 8, 8, **kw)
        assert e.value.code == -1 and "phnsw_search_exact_grouped_device" in str(e.value), kw
    L = ph.lib()
    buf = np.zeros(4 * NW * 5, dtype=np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    for stride, nf, filters, filter_of in ((0, 5, p, p), (NW - 1, 5, p, p), (NW, 0, p, p), (NW, 5, None, p), (NW, 5, p, None)):
        assert L.phnsw_search_exact_grouped(hix._h, None, p, 4, None, filters, stride, nf, filter_of, 3, p, p, p) == -1
        assert "phnsw_search_exact_grouped:" in L.phnsw_last_error().decode()
    assert L.phnsw_search_exact_grouped(hix._h, p, p, 4, None, p, NW, 5, p, 3, p, p, p) == -1  # both
    assert L.phnsw_search_exact_grouped(hix._h, None, None, 4, None, p, NW, 5, p, 3, p, p, p) == -1  # neither
    with pytest.raises(ValueError):
        hix.search_exact_grouped(queries=q, qids=w["qids"][:4], allows=masks, allow_of=of)
    with pytest.raises(ValueError):
        hix.search_exact_grouped(allows=masks, allow_of=of)
