"""phnsw_search_collect[_device] and phnsw_search_collect_labeled[_device]: the walk that keeps the best allowed rows it
evaluates.  Every comparison is on ids, distance BITS, lengths and the per-query evaluation and hop counters against
tests/collect_reference.py (pinned to the oracle by tests/test_collect_cpu.py).  No tolerance.

The setting is tests/test_gpu_kernel_choice.py's: n = 2000, the oracle's graph over the f32 rows adopted by every store
kind, 129 raw queries (two full waves plus one), probe depth 2, the throughput kernels (PHNSW_NO_LAT=1) unless a case
says otherwise.  Every layer of 2000 nodes is a dense one, so each grid case runs as it comes (the last layer walked in
table ids, distances from the table) and under PHNSW_NO_TINY=1 (every distance gathered), against ONE reference.

Without EXTEND the traversal does not depend on k, and `kept` of capacity 64 begins with `kept` of any smaller capacity:
one reference at k = 64 serves k = 1, 10 and 64.  With EXTEND each k has a walk of its own."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from parallel_hnsw_amd._lib import check, lib

import collect_reference as cr
import filter_reference as fr
from test_gpu_i8q import env
from test_gpu_kernel_choice import N, NQ, PD, bits, graph, oracle_over, queries

pytestmark = pytest.mark.gpu

EMPTY = fr.EMPTY
E_INVALID = -1
KINDS = [("f32", 32), ("f32", 768), ("f16", 768), ("i8", 768)]
EFS = [64, 300, 600]
ABSENT = 1000  # a label no row carries (labels = v mod 7)


def dist(oix, **kw):
    """the oracle's distances in the kernels' summation order (ORC_SUM_BLOCKED64)"""
    return fr.distance_rows(oix, mode=oracle.SUM_BLOCKED64, **kw)


@functools.lru_cache(maxsize=None)
def world(kind, dim):
    """(GPU index over that store, oracle over store_read of it, its layers as filter_reference takes them, the
    distances of the 129 queries to every row); made once, changed by no test"""
    rows, layers = graph(dim)
    full = ph.VectorStore(rows)
    store = {"f32": lambda s: s, "f16": ph.F16Store.from_full, "i8": ph.I8Store.from_full}[kind](full)
    hix = ph.Hnsw.from_layers(store, layers, ph.BuildParameters(seed=1))
    oix = oracle_over(store.read(), layers)
    return hix, oix, fr.layers_of(oix), dist(oix, queries=queries(dim))


@functools.lru_cache(maxsize=None)
def mixed(seed=5):
    """per-query bitmaps [129, 2000]: density 0.5, density 0.05, five rows, none at all, in turn"""
    rng = np.random.default_rng(seed)
    a = np.zeros((NQ, N), dtype=bool)
    for i in range(NQ):
        if i % 4 == 0:
            a[i] = rng.random(N) < 0.5
        elif i % 4 == 1:
            a[i] = rng.random(N) < 0.05
        elif i % 4 == 2:
            a[i, rng.choice(N, size=5, replace=False)] = True
    return a


def same(got, ref, k=None):
    """a GPU result against a reference row; k: the reference was made with a larger capacity, compare its head"""
    gi, gd, gl, gs = got
    ri, rd, rl, rs = ref
    if k is not None:
        ri, rd, rl = ri[:, :k], rd[:, :k], np.minimum(rl, k)
    np.testing.assert_array_equal(gl, rl)
    np.testing.assert_array_equal(gi, ri)
    np.testing.assert_array_equal(bits(gd), bits(rd))
    np.testing.assert_array_equal(gs, rs)
    for i in range(len(gl)):  # the padding
        assert (gi[i, int(gl[i]):] == EMPTY).all() and (bits(gd[i, int(gl[i]):]) == bits(fr.FMAX)).all()


# ---------------------------------------------------------------- 1: the grid, dense and gathered last layers
@pytest.mark.parametrize("ef", EFS)
@pytest.mark.parametrize("kind,dim", KINDS)
def test_grid(monkeypatch, kind, dim, ef):
    hix, oix, layers, D = world(kind, dim)
    q, allow = queries(dim), mixed()
    spt, sp = (ef, ef, PD), ph.SearchParameters(ef, ef, PD)
    plain = oix.search(queries=q, sp=spt, stats=True)
    ref = cr.search(oix, D, spt, 64, allow=allow, layers=layers)
    np.testing.assert_array_equal(ref[3], plain[3])  # the traversal is the plain search's
    ref_ext = cr.search(oix, D, spt, 10, allow=allow, extend=True, layers=layers)
    assert (ref_ext[3] >= ref[3]).all()
    if ef == 64:
        assert (ref_ext[3][:, 1] > ref[3][:, 1]).any()  # EXTEND walks on somewhere: the flag is not a no-op here
    # the cases the grid is there for: rows shorter than k, an empty row, several keys entering a `kept` of one slot
    assert (ref[2][2::4] > 0).any() and (ref[2][2::4] <= 5).all() and (ref[2][3::4] == 0).all() and (ref[2][0::4] == 64).any()
    for kv in (dict(PHNSW_NO_LAT="1"), dict(PHNSW_NO_LAT="1", PHNSW_NO_TINY="1")):
        with env(monkeypatch, **kv):
            for k in (1, 10, 64):
                same(hix.search_collect(queries=q, sp=sp, allow=allow, k=k, stats=True), ref, k=k)
            assert (hix.dispatches()[1]["n_table"] == 0) == ("PHNSW_NO_TINY" in kv)
            same(hix.search_collect(queries=q, sp=sp, allow=allow, k=10, extend=True, stats=True), ref_ext)


@pytest.mark.parametrize("k", [1, 64])
def test_extend_at_the_other_capacities(monkeypatch, k):
    hix, oix, layers, D = world("f32", 768)
    q, allow = queries(768), mixed()
    ref = cr.search(oix, D, (64, 64, PD), k, allow=allow, extend=True, layers=layers)
    for kv in (dict(PHNSW_NO_LAT="1"), dict(PHNSW_NO_LAT="1", PHNSW_NO_TINY="1"), dict()):  # (the last: the latency kernel)
        with env(monkeypatch, **kv):
            same(hix.search_collect(queries=q, sp=ph.SearchParameters(64, 64, PD), allow=allow, k=k, extend=True, stats=True), ref)


# ---------------------------------------------------------------- 2: shared bitmaps, every row allowed, no filter at all
@pytest.mark.parametrize("extend", [False, True])
def test_shared_bitmaps(monkeypatch, extend):
    hix, oix, layers, D = world("f32", 32)
    q = queries(32)
    spt, sp = (64, 64, PD), ph.SearchParameters(64, 64, PD)
    rng = np.random.default_rng(17)
    five = np.zeros(N, dtype=bool)
    five[rng.choice(N, size=5, replace=False)] = True
    plain = oix.search(queries=q, sp=spt, stats=True)
    with env(monkeypatch, PHNSW_NO_LAT="1", PHNSW_NO_TINY="1"):
        for allow in (rng.random(N) < 0.5, rng.random(N) < 0.05, five, np.zeros(N, dtype=bool)):
            same(hix.search_collect(queries=q, sp=sp, allow=allow, k=10, extend=extend, stats=True),
                 cr.search(oix, D, spt, 10, allow=allow, extend=extend, layers=layers))
        # every row allowed, as a bitmap and as "no filter": the head of the plain search, whatever the flag
        for allow in (np.ones(N, dtype=bool), None):
            for k in (1, 10, 64):
                got = hix.search_collect(queries=q, sp=sp, allow=allow, k=k, extend=extend, stats=True)
                same(got, plain, k=k)
        same(hix.search_collect(queries=q, sp=sp, allow=None, k=10, extend=extend, stats=True),
             hix.search_batch(queries=q, sp=sp, stats=True), k=10)


def test_the_default_filter_is_the_filter_of_a_call_without_one():
    import torch
    hix, oix, layers, D = world("f32", 32)
    q = queries(32)
    allow = np.random.default_rng(23).random(N) < 0.1
    words = torch.from_numpy(fr.pack(allow).view(np.int32)).to("cuda:0")
    try:
        hix.set_filter(words.data_ptr())
        got = hix.search_collect(queries=q, sp=ph.SearchParameters(64, 64, PD), k=10, stats=True)
    finally:
        hix.set_filter(0)
    same(got, cr.search(oix, D, (64, 64, PD), 10, allow=allow, layers=layers))


# ---------------------------------------------------------------- 3: exclude, stored queries, upto_layers
@pytest.mark.parametrize("extend", [False, True])
def test_stored_queries_and_an_exclude_that_is_itself_allowed(monkeypatch, extend):
    hix, oix, layers, _ = world("f32", 768)
    qids = np.arange(0, N, 15, dtype=np.uint64)  # 134 stored queries
    D = dist(oix, qids=qids)
    allow = np.random.default_rng(31).random((len(qids), N)) < 0.2
    allow[np.arange(len(qids)), qids.astype(np.int64)] = True  # the query's own row: allowed, and excluded
    spt, sp = (64, 64, PD), ph.SearchParameters(64, 64, PD)
    for kv in (dict(PHNSW_NO_LAT="1"), dict(PHNSW_NO_LAT="1", PHNSW_NO_TINY="1")):
        with env(monkeypatch, **kv):
            for ex in (qids, None):
                for upto in (0, 2):
                    got = hix.search_collect(qids=qids, sp=sp, allow=allow, exclude=ex, k=10, extend=extend, upto=upto, stats=True)
                    same(got, cr.search(oix, D, spt, 10, allow=allow, exclude=ex, extend=extend, upto=upto, layers=layers))
                    if ex is not None:
                        assert (got[0] != qids[:, None]).all()
                    elif upto == 0:
                        assert (got[0][:, 0] == qids).all()  # its own row is the nearest allowed one


# ---------------------------------------------------------------- 4: equal distances inside one hop's batch
def test_duplicated_rows_are_ordered_by_id(monkeypatch):
    dim = 32
    rows = oracle.synth_rows(0, N, dim)[:, :dim].copy()
    rows[N // 2:] = rows[:N // 2]  # every row twice: v and v + 1000 are at the same distance from everything
    oix = oracle.Index.generate(np.ascontiguousarray(rows), np.arange(N), oracle.default_build_params(seed=1), dim=dim,
                                sum_mode=oracle.SUM_BLOCKED64)
    raw = [oix.layer(l) for l in range(oix.layer_count)]
    hix = ph.Hnsw.from_layers(ph.VectorStore(rows), raw, ph.BuildParameters(seed=1))
    layers = fr.layers_of(oix)
    q = queries(dim)
    D = dist(oix, queries=q)
    allow = np.random.default_rng(41).random((NQ, N // 2)) < 0.3
    allow = np.concatenate([allow, allow], axis=1)  # both copies or neither
    pairs = 0
    for ef, k, extend in ((64, 10, False), (64, 10, True), (300, 64, False)):
        ref = cr.search(oix, D, (ef, ef, PD), k, allow=allow, extend=extend, layers=layers)
        pairs += int(((ref[1][:, 1:] == ref[1][:, :-1]) & (ref[0][:, 1:] != EMPTY)).sum())
        for kv in (dict(PHNSW_NO_LAT="1"), dict(PHNSW_NO_LAT="1", PHNSW_NO_TINY="1")):
            with env(monkeypatch, **kv):
                same(hix.search_collect(queries=q, sp=ph.SearchParameters(ef, ef, PD), allow=allow, k=k, extend=extend, stats=True), ref)
    assert pairs > 100  # rows really hold neighbours at equal distance


# ---------------------------------------------------------------- 5: a seed that falls out of the layer's queue
def test_the_best_allowed_row_is_a_seed_that_leaves_the_queue(monkeypatch):
    hix, oix, layers, D = world("f32", 32)
    q = queries(32)
    spt, sp = (64, 64, PD), ph.SearchParameters(64, 64, PD)
    seeds = fr.search(oix, D, spt, upto=oix.layer_count - 1, layers=layers)  # the running candidates the last layer starts from
    final = oix.search(queries=q, sp=spt)
    allow = np.zeros((NQ, N), dtype=bool)
    fell = np.zeros(NQ, dtype=bool)
    for i in range(NQ):
        gone = [int(v) for v in seeds[0][i, :int(seeds[2][i])] if int(v) not in set(final[0][i].tolist())]
        fell[i] = bool(gone)
        allow[i, gone[-1] if gone else int(seeds[0][i, 0])] = True
    assert fell.sum() > NQ // 2
    ref = cr.search(oix, D, spt, 10, allow=allow, layers=layers)
    assert (ref[2] == 1).all() and (ref[0][:, 0] == np.argmax(allow, axis=1)).all()
    for kv in (dict(PHNSW_NO_LAT="1"), dict(PHNSW_NO_LAT="1", PHNSW_NO_TINY="1")):
        with env(monkeypatch, **kv):
            same(hix.search_collect(queries=q, sp=sp, allow=allow, k=10, stats=True), ref)


# ---------------------------------------------------------------- 6: by label
@functools.lru_cache(maxsize=None)
def labels_of(kind, dim):
    lab = np.arange(N) % 7
    return lab, ph.Labels(world(kind, dim)[0], lab)


def wants(nq):
    return np.array([(ABSENT if i % 9 == 7 else (-1 if i % 9 == 8 else i % 9)) for i in range(nq)], dtype=np.int64)


@pytest.mark.parametrize("kind,dim", [("f32", 32), ("f32", 768), ("i8", 768)])
def test_by_label(monkeypatch, kind, dim):
    hix, oix, layers, D = world(kind, dim)
    lab, lb = labels_of(kind, dim)
    q, want = queries(dim), wants(NQ)
    masks = lab[None, :] == want[:, None]  # ABSENT and NONE (-1) match no row
    ex = np.array([np.nonzero(m)[0][3] if m.any() else 0 for m in masks], dtype=np.uint64)
    for ef, k, extend, e in ((64, 10, False, None), (64, 10, True, ex), (300, 64, False, ex), (600, 1, True, None)):
        spt, sp = (ef, ef, PD), ph.SearchParameters(ef, ef, PD)
        ref = cr.search(oix, D, spt, k, allow=masks, exclude=e, extend=extend, layers=layers)
        assert (ref[2][want == ABSENT] == 0).all() and (ref[2][want == -1] == 0).all() and (ref[2][want == 0] == k).all()
        for kv in (dict(PHNSW_NO_LAT="1"), dict(PHNSW_NO_LAT="1", PHNSW_NO_TINY="1")):
            with env(monkeypatch, **kv):
                got = hix.search_collect_labeled(queries=q, sp=sp, labels=lb, want=want, exclude=e, k=k, extend=extend, stats=True)
                same(got, ref)
                same(got, hix.search_collect(queries=q, sp=sp, allow=masks, exclude=e, k=k, extend=extend, stats=True))


# ---------------------------------------------------------------- 6b: the other store kinds the filtered walk accepts
from test_gpu_kernel_choice import i8q_pairs, i8q_queries  # noqa: E402,F401  (i8q_pairs: a module fixture, used below)


def test_i8q_rows(i8q_pairs, monkeypatch):
    """an i8q store equals the oracle on lattice data (tests/test_gpu_kernel_choice.py): its rows, graph and queries"""
    hix, oix = i8q_pairs(32)
    layers, q, allow = fr.layers_of(oix), i8q_queries(32), mixed()
    D = dist(oix, queries=q)
    for ef, k, extend in ((64, 10, False), (64, 10, True), (300, 64, False)):
        ref = cr.search(oix, D, (ef, ef, PD), k, allow=allow, extend=extend, layers=layers)
        for kv in (dict(PHNSW_NO_LAT="1"), dict(PHNSW_NO_LAT="1", PHNSW_NO_TINY="1")):
            with env(monkeypatch, **kv):
                same(hix.search_collect(queries=q, sp=ph.SearchParameters(ef, ef, PD), allow=allow, k=k, extend=extend, stats=True), ref)


def test_pq_rows_against_the_plain_search_of_the_same_store(monkeypatch):
    """a PQ store has no oracle: with every row allowed the row is the head of search_batch's, and with a filter the
    stats are search_batch's and the row holds every allowed entry of search_batch's row up to its own tail"""
    from test_gpu_filter import N as NF, raw_queries, world as filter_world
    hix = filter_world("pq", 128)[0]
    q = raw_queries("pq", 128, 40)
    allow = np.random.default_rng(47).random((len(q), NF)) < 0.3
    for ef in (64, 300):
        sp = ph.SearchParameters(ef, ef, PD)
        for kv in (dict(PHNSW_NO_LAT="1"), dict(PHNSW_NO_LAT="1", PHNSW_NO_TINY="1")):
            with env(monkeypatch, **kv):
                plain = hix.search_batch(queries=q, sp=sp, stats=True)
                for extend in (False, True):
                    same(hix.search_collect(queries=q, sp=sp, allow=np.ones(NF, dtype=bool), k=10, extend=extend, stats=True), plain, k=10)
                gi, gd, gl, gs = hix.search_collect(queries=q, sp=sp, allow=allow, k=10, stats=True)
                np.testing.assert_array_equal(gs, plain[3])
                for i in range(len(q)):
                    g = [(float(gd[i, j]), int(gi[i, j])) for j in range(int(gl[i]))]
                    p_ = [(float(plain[1][i, j]), int(plain[0][i, j])) for j in range(int(plain[2][i])) if allow[i, int(plain[0][i, j])]]
                    assert g == sorted(g) and all(allow[i, v] for _, v in g) and len(g) == 10
                    assert all(x in g or x > g[-1] for x in p_)


# ---------------------------------------------------------------- 7: the device forms against the host forms
def device_collect(hix, sp, k, queries=None, qids=None, allow=None, labels=None, want=None, exclude=None, extend=False, upto=0,
                   statuses=None):
    """phnsw_search_collect_device / phnsw_search_collect_labeled_device with torch buffers -> ids u64, d, len u64, stats
    u64; 64 guard words behind every output must come back as they went in.  Every status must be 0, unless the caller
    passes a list: it then gets status[nq] appended instead"""
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
    G = 64
    ids = torch.full((nq * k + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * k + G,), -1.0, dtype=torch.float32, device=dev)
    ln, status = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(2))
    st = torch.full((2 * nq + G,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if labels is not None:
        wd = up(ph.hnsw.pack_labels(want, nq, "want"), np.int32).data_ptr()
        hix.search_collect_labeled_device(labels, nq, sp, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(),
                                          queries=qd, ldq=ld, qids=qi, exclude=ex, want=wd, extend=extend,
                                          out_stats=st.data_ptr(), upto=upto)
    else:
        words, stride = ph.hnsw.pack_allow(allow, hix.store.n, nq)
        ad = 0 if words is None else up(words, np.int32).data_ptr()
        hix.search_collect_device(nq, sp, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd, ldq=ld,
                                  qids=qi, exclude=ex, allow=ad, allow_stride=stride, extend=extend, out_stats=st.data_ptr(),
                                  upto=upto)
    torch.cuda.synchronize()
    assert (ids[nq * k:] == 7).all() and (d[nq * k:] == -1.0).all()
    assert (ln[nq:] == -1).all() and (status[nq:] == -1).all() and (st[2 * nq:] == -1).all()
    if statuses is None:
        assert (status[:nq] == 0).all()
    else:
        statuses.append(status[:nq].cpu().numpy())
    i64 = ids[:nq * k].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, k)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return (i64, d[:nq * k].cpu().numpy().reshape(nq, k), ln[:nq].cpu().numpy().view(np.uint32).astype(np.uint64),
            st[:2 * nq].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, 2))


def test_device_forms_equal_the_host_forms(monkeypatch):
    hix = world("f32", 768)[0]
    lab, lb = labels_of("f32", 768)
    q, allow, want = queries(768), mixed(), wants(NQ)
    qids = np.arange(0, N, 15, dtype=np.uint64)[:NQ]
    sp = ph.SearchParameters(64, 64, PD)
    with env(monkeypatch, PHNSW_NO_LAT="1"):
        for extend in (False, True):
            for kw in (dict(queries=q), dict(qids=qids, exclude=qids)):
                same(device_collect(hix, sp, 10, allow=allow, extend=extend, **kw),
                     hix.search_collect(sp=sp, allow=allow, k=10, extend=extend, stats=True, **kw))
                same(device_collect(hix, sp, 10, labels=lb, want=want, extend=extend, **kw),
                     hix.search_collect_labeled(sp=sp, labels=lb, want=want, k=10, extend=extend, stats=True, **kw))
        same(device_collect(hix, sp, 64, allow=allow[0], queries=q), hix.search_collect(queries=q, sp=sp, allow=allow[0], k=64, stats=True))
        same(device_collect(hix, sp, 3, queries=q), hix.search_collect(queries=q, sp=sp, k=3, stats=True))  # no filter at all


# ---------------------------------------------------------------- 8: the other paths of a descent
def test_visited_in_the_bitmap_split_descents_and_chunks(monkeypatch):
    hix, oix, layers, D = world("f32", 768)
    lab, lb = labels_of("f32", 768)
    q, allow, want = queries(768), mixed(), wants(NQ)
    masks = lab[None, :] == want[:, None]
    spt, sp = (256, 256, PD), ph.SearchParameters(256, 256, PD)
    refs = {e: (cr.search(oix, D, spt, 10, allow=allow, extend=e, layers=layers),
                cr.search(oix, D, spt, 10, allow=masks, extend=e, layers=layers)) for e in (False, True)}
    count = lib().phnsw_debug_two_launch_count
    count.restype = C.c_uint64
    split = dict(PHNSW_TWO_LAUNCH_MIN="1", PHNSW_SPLIT_BYTES="1", PHNSW_NO_LAT="1")
    settings = [dict(PHNSW_NO_LAT="1", PHNSW_VISITED="global"), dict(PHNSW_NO_LAT="1", PHNSW_VISITED="global", PHNSW_NO_TINY="1"),
                dict(PHNSW_NO_LAT="1", PHNSW_NO_TINY="1", PHNSW_VISITED_LDS_SLOTS="256"),  # the table moves into the bitmap part-way
                dict(split, PHNSW_TINY_MAX="200"),  # the top layers in the dense-only launch, then a launch per layer
                dict(split, PHNSW_NO_TINY="1"),
                dict(PHNSW_NO_LAT="1", PHNSW_HOST_CHUNKS="0,50,40"),  # the host path in chunks: bitmaps and labels follow
                dict(PHNSW_NO_LAT="1", PHNSW_TINY_TABLE_BYTES=str(50 * 4 * N))]  # the dense table holds ~50 queries
    for kv in settings:
        with env(monkeypatch, **kv):
            before = count()
            for e in (False, True):
                same(hix.search_collect(queries=q, sp=sp, allow=allow, k=10, extend=e, stats=True), refs[e][0])
                same(hix.search_collect_labeled(queries=q, sp=sp, labels=lb, want=want, k=10, extend=e, stats=True), refs[e][1])
                if "PHNSW_HOST_CHUNKS" not in kv:
                    same(device_collect(hix, sp, 10, queries=q, allow=allow, extend=e), refs[e][0])
                    same(device_collect(hix, sp, 10, queries=q, labels=lb, want=want, extend=e), refs[e][1])
            assert (count() > before) == ("PHNSW_TWO_LAUNCH_MIN" in kv)
            if "PHNSW_TINY_TABLE_BYTES" in kv:
                assert lib().phnsw_debug_last_search_chunks(hix._h) > 1


def test_the_overflow_rerun_rebuilds_kept(monkeypatch):
    """PHNSW_OVF_CAP=64 on gathered layers at ef 256: a walk evaluates about a thousand rows, so its spill list overflows.
    A workspace keeps the largest spill list it ever had, so every call that must overflow gets a fresh index (and a
    Labels handle made for it).  The device forms, which re-run nothing, report status 5 for those queries and leave their
    rows empty; the host forms re-run them with 8x the room until they fit, and return the reference's rows"""
    hix0, oix, layers, D = world("f32", 768)
    raw = graph(768)[1]
    q, allow, want = queries(768), mixed(), wants(NQ)
    lab = np.arange(N) % 7
    masks = lab[None, :] == want[:, None]
    spt, sp = (256, 256, PD), ph.SearchParameters(256, 256, PD)

    def fresh():
        return ph.Hnsw.from_layers(hix0.store, raw, ph.BuildParameters(seed=1))

    with env(monkeypatch, PHNSW_NO_LAT="1", PHNSW_NO_TINY="1", PHNSW_OVF_CAP="64"):
        for e in (False, True):
            refs = (cr.search(oix, D, spt, 10, allow=allow, extend=e, layers=layers),
                    cr.search(oix, D, spt, 10, allow=masks, extend=e, layers=layers))
            for form in range(2):
                g = fresh()
                dkw = dict(allow=allow) if form == 0 else dict(labels=ph.Labels(g, lab), want=want)
                stt = []
                got = device_collect(g, sp, 10, queries=q, extend=e, statuses=stt, **dkw)
                over = stt[0] == 5
                assert over.any() and ((stt[0] == 0) | over).all()  # the overflow really happens here
                assert (got[2][over] == 0).all() and (got[0][over] == EMPTY).all()
                same(tuple(x[~over] for x in got), tuple(x[~over] for x in refs[form]))
                g = fresh()
                if form == 0:
                    same(g.search_collect(queries=q, sp=sp, allow=allow, k=10, extend=e, stats=True), refs[0])
                else:
                    same(g.search_collect_labeled(queries=q, sp=sp, labels=ph.Labels(g, lab), want=want, k=10, extend=e, stats=True),
                         refs[1])


# ---------------------------------------------------------------- 9: argument checks
def test_argument_checks():
    hix = world("f32", 32)[0]
    lab, lb = labels_of("f32", 32)
    sp = ph.SearchParameters(16, 16, 2)
    q = queries(32)[:4]
    want = wants(4)
    L = lib()
    buf = C.c_void_p(8)

    def host(flags=0, k=10, queries=q.ctypes.data_as(C.c_void_p), qids=None, nq=4, stride=0, sp_=sp):
        return L.phnsw_search_collect(hix._h, queries, qids, nq, C.byref(sp_), 0, None, None, stride, flags, k, buf, buf, buf, None)

    def host_labeled(flags=0, k=10, queries=q.ctypes.data_as(C.c_void_p), qids=None, nq=4, want_=buf, handle=lb._h):
        return L.phnsw_search_collect_labeled(hix._h, handle, queries, qids, nq, C.byref(sp), 0, None, want_, flags, k, buf, buf,
                                              buf, None)

    def device(flags=0, k=10, queries=None, qids=buf, nq=4, stride=0):
        return L.phnsw_search_collect_device(hix._h, queries, hix.store.ld, qids, nq, C.byref(sp), 0, None, None, stride, flags, k,
                                             buf, buf, buf, None, buf, None)

    def device_labeled(flags=0, k=10, queries=None, qids=buf, nq=4, want_=buf):
        return L.phnsw_search_collect_labeled_device(hix._h, lb._h, queries, hix.store.ld, qids, nq, C.byref(sp), 0, None, want_,
                                                     flags, k, buf, buf, buf, None, buf, None)

    for f in (host, host_labeled, device, device_labeled):
        assert f(flags=2) == E_INVALID and "unknown flag bits" in ph.lib().phnsw_last_error().decode()
        assert f(k=0) == E_INVALID and "k must be 1..64" in ph.lib().phnsw_last_error().decode()
        assert f(k=65) == E_INVALID
        assert f(queries=None, qids=None) == E_INVALID and "exactly one" in ph.lib().phnsw_last_error().decode()
        assert f(queries=buf, qids=buf) == E_INVALID
        assert f(nq=0, queries=None, qids=None) == 0  # a no-op, whatever the pointers
        assert f(nq=0, flags=2) == E_INVALID  # ... behind the checks of flags and k
    for f in (host, device):
        assert f(stride=(N + 31) // 32 - 1) == E_INVALID and "filter_stride_words" in ph.lib().phnsw_last_error().decode()
    assert host(sp_=ph.SearchParameters(1025, 16, 2)) == E_INVALID  # the parameters come first
    assert host_labeled(want_=None) == E_INVALID and device_labeled(want_=None) == E_INVALID
    assert host_labeled(handle=None) == E_INVALID and "labels" in ph.lib().phnsw_last_error().decode()
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses a Stored query id at or past n
        hix.search_collect(qids=np.array([N], dtype=np.uint64), sp=sp, k=3)
    assert e.value.code == E_INVALID and "out of range" in str(e.value)
    with pytest.raises(ValueError):
        hix.search_collect(sp=sp, k=3)
    # k may exceed number_of_candidates: `kept` has a capacity of its own
    ids, d, ln = hix.search_collect(queries=q, sp=sp, k=64)
    assert ids.shape == (4, 64) and (ln > 16).all()
    # flag value 2 stays invalid on the filtered walk
    with pytest.raises(ph.PhnswError):
        check(L.phnsw_search_batch_filtered(hix._h, q.ctypes.data_as(C.c_void_p), None, 4, C.byref(sp), 0, None, None, 0, 2, 0, buf,
                                            buf, buf, None))
