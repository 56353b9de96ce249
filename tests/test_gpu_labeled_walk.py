"""phnsw_search_batch_labeled[_device]: the graph walk restricted by row label, on the search kernels' label mode.  Every
comparison is on ids, distance bits, lengths, stats and statuses; none has a tolerance.

Yardsticks, named per assertion below:
  * A -- tests/filter_reference.search, the restatement of search_layers / closest_vectors over the oracle's distances,
         with the masks tests/labeled_reference.masks_of makes of the label column: masks the code under test never saw.
  * B -- search_batch_filtered with those masks as per-query bitmaps: rows, lengths and stats must be equal bit for bit.

The worlds are those of tests/test_gpu_filter.py (N = 2000, built multi-layer graphs: the smallest at which the walk's
loops turn) and, for unlisted vectors, the every-second-vector index of tests/test_gpu_filter_auto.py (N = 5000).  The
label column is constructed, not drawn."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from parallel_hnsw_amd._lib import check, lib

import filter_reference as fr
import labeled_reference as lr
import test_gpu_filter_auto as ta
from test_gpu_exact_filter import ring
from test_gpu_filter import COS, EMPTY, KINDS, N, dist, raw_queries, same, world
from test_gpu_i8 import bits
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

NONE = lr.LABEL_NONE
HALF, TENTH, HUNDREDTH, ZERO = 7, 1000003, 5, 0
ONE, L64, L65, TOP, ABSENT = 11, 12, 13, 0xFFFFFFFE, 999
SIZES = [(ONE, 1), (L64, 64), (L65, 65), (TOP, 30), (NONE, 100), (HUNDREDTH, 20), (TENTH, 200), (ZERO, 520)]
# what the queries want, in turn: every label of the column, the absent one and NONE
WANTS = [HALF, TENTH, HUNDREDTH, ONE, L64, L65, TOP, ABSENT, NONE, ZERO]
NQ = 20
E_INVALID = -1


def column(n, entry, seed=3, members=None):
    """i64 [n]: the entry vector carries HALF; the other rows, in a random order, get the labels of SIZES in exactly those
    numbers (NONE: rows without a label) and HALF for the rest -- about half of them"""
    lab = np.full(n, HALF, dtype=np.int64)
    pool = np.arange(n) if members is None else np.nonzero(members)[0]
    rest = np.random.default_rng(seed).permutation(pool[pool != entry])
    at = 0
    for value, count in SIZES:
        lab[rest[at:at + count]] = value
        at += count
    return lab


@functools.lru_cache(maxsize=None)
def labels_of(kind, dim):
    """(the column, a Labels over world(kind, dim)'s index); made once, changed by no test"""
    hix, _, _, g = world(kind, dim)
    lab = column(N, int(g.entry_vector()))
    return lab, ph.Labels(hix, lab)


def wants(nq, shift=0):
    return np.array([WANTS[(i + shift) % len(WANTS)] for i in range(nq)], dtype=np.int64)


def test_the_column_is_what_the_docstring_says():
    hix, _, _, g = world("f32", 100)
    lab, lb = labels_of("f32", 100)
    counts = {v: int((lab == v).sum()) for v in set(lab.tolist())}
    assert counts[ONE] == 1 and counts[L64] == 64 and counts[L65] == 65 and counts[NONE] == 100 and counts[TOP] == 30
    assert counts[HUNDREDTH] == 20 and counts[TENTH] == 200 and 900 <= counts[HALF] <= 1100 and ABSENT not in counts
    assert lab[int(g.entry_vector())] == HALF
    np.testing.assert_array_equal(lb.count(wants(len(WANTS))), [counts[HALF], 200, 20, 1, 64, 65, 30, 0, 0, 520])
    assert lb.listed == N - 100 and lb.nlabels == 8


def device_walk(hix, lb, sp, queries=None, qids=None, want=None, exclude=None, strict=False, upto=0, stream=0):
    """phnsw_search_batch_labeled_device with torch buffers -> ids u64, d, len u64, stats u64, status; 64 guard words
    behind every output must come back as they went in"""
    import torch
    dev = torch.device("cuda", 0)
    keep = []

    def up(a, dt):
        t = torch.from_numpy(np.ascontiguousarray(a).view(dt) if dt is not None else np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t

    nq = len(queries) if queries is not None else len(qids)
    ef = sp.number_of_candidates
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
    wd = up(ph.hnsw.pack_labels(want, nq, "want"), np.int32).data_ptr()
    G = 64
    ids = torch.full((nq * ef + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * ef + G,), -1.0, dtype=torch.float32, device=dev)
    ln, status = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(2))
    st = torch.full((2 * nq + G,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    hix.search_batch_labeled_device(lb, nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd,
                                    ldq=ld, qids=qi, exclude=ex, want=wd, strict=strict, out_stats=st.data_ptr(), upto=upto,
                                    stream=stream)
    torch.cuda.synchronize()
    assert (ids[nq * ef:] == 7).all() and (d[nq * ef:] == -1.0).all()
    assert (ln[nq:] == -1).all() and (status[nq:] == -1).all() and (st[2 * nq:] == -1).all()
    i64 = ids[:nq * ef].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, ef)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return (i64, d[:nq * ef].cpu().numpy().reshape(nq, ef), ln[:nq].cpu().numpy().view(np.uint32).astype(np.uint64),
            st[:2 * nq].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, 2), status[:nq].cpu().numpy())


# ---------------------------------------------------------------- 1: both yardsticks, every twin family
@pytest.mark.parametrize("kind,dim", KINDS)
def test_the_label_walk_equals_the_restatement_and_the_bitmap_walk(kind, dim):
    hix, oix, layers, g = world(kind, dim)
    lab, lb = labels_of(kind, dim)
    spt = (64, 24, 2)
    sp = ph.SearchParameters(*spt)
    want = wants(NQ)
    masks = lr.masks_of(lab, want)
    q = raw_queries(kind, dim, NQ)
    qids = np.arange(11, N, N // NQ, dtype=np.uint64)[:NQ]
    # exclude: a listed vector of the wanted label where there is one (it matters), else any id
    ex = np.array([np.nonzero(masks[i])[0][i % 3 % max(int(masks[i].sum()), 1)] if masks[i].any() else i for i in range(NQ)],
                  dtype=np.uint64)
    seen_entry = False
    for kw in (dict(queries=q), dict(qids=qids)):
        D = None if oix is None else dist(oix, **kw)
        for upto in (0, 1, 2):
            for e in (None, ex):
                got = hix.search_batch_labeled(sp=sp, labels=lb, want=want, exclude=e, upto=upto, stats=True, **kw)
                same(got, hix.search_batch_filtered(sp=sp, allow=masks, exclude=e, upto=upto, stats=True, **kw))       # B
                strict = hix.search_batch_labeled(sp=sp, labels=lb, want=want, strict=True, exclude=e, upto=upto, stats=True, **kw)
                same(strict, hix.search_batch_filtered(sp=sp, allow=masks, strict=True, exclude=e, upto=upto, stats=True, **kw))  # B
                if oix is not None:
                    ref = fr.search(oix, D, spt, allow=masks, exclude=e, upto=upto, layers=layers)
                    same(got, ref)                                                                                     # A
                    same(strict, fr.strict(ref, masks), stats=False)                                                   # A
                    np.testing.assert_array_equal(strict[3], ref[3])  # strict drops ids after the walk: the same stats
                seen_entry |= bool(((got[0] == g.entry_vector()) & ~masks[:, int(g.entry_vector())][:, None]).any())
        cut = hix.search_batch_labeled(sp=sp, labels=lb, want=want, exclude=ex, k=5, **kw)                             # the k cut
        same(cut, hix.search_batch_filtered(sp=sp, allow=masks, exclude=ex, k=5, **kw))
        whole = hix.search_batch_labeled(sp=sp, labels=lb, want=want, exclude=ex, **kw)
        assert cut[0].shape == (NQ, 5) and whole[0].shape == (NQ, 64)
        np.testing.assert_array_equal(cut[0], whole[0][:, :5])
        np.testing.assert_array_equal(cut[2], np.minimum(whole[2], 5))
        dv = device_walk(hix, lb, sp, want=want, exclude=ex, **kw)
        assert not dv[4].any()
        same(dv, hix.search_batch_labeled(sp=sp, labels=lb, want=want, exclude=ex, stats=True, **kw))
    # the entry vector carries HALF: returned to queries that want another label, unless strict (asserted above by B and A)
    assert seen_entry


# ---------------------------------------------------------------- 2: every queue capacity class
@pytest.mark.parametrize("ef", [64, 128, 256, 512])
def test_queue_capacity_classes(monkeypatch, ef):
    hix, oix, layers, _ = world("f32", 100)
    lab, lb = labels_of("f32", 100)
    q = raw_queries("f32", 100, 12)
    want = wants(12, shift=ef // 64)
    masks = lr.masks_of(lab, want)
    sp = ph.SearchParameters(ef, ef, 2)
    ref = hix.search_batch_filtered(queries=q, sp=sp, allow=masks, stats=True)                                        # B
    same(hix.search_batch_labeled(queries=q, sp=sp, labels=lb, want=want, stats=True), ref)
    with env(monkeypatch, PHNSW_NO_LAT="1", PHNSW_NO_TINY="1"):  # the throughput kernel of pick_kernel_rows, rows gathered per hop
        same(hix.search_batch_labeled(queries=q, sp=sp, labels=lb, want=want, stats=True), ref)
        same(hix.search_batch_labeled(queries=q, sp=sp, labels=lb, want=want, strict=True, stats=True),
             hix.search_batch_filtered(queries=q, sp=sp, allow=masks, strict=True, stats=True))


# ---------------------------------------------------------------- 3: independence of the schedule
@pytest.mark.parametrize("kind,dim", [("f32", 100), ("f16", 100), ("i8q", 128)])
def test_labeled_results_do_not_depend_on_the_schedule(monkeypatch, kind, dim):
    hix, oix, layers, _ = world(kind, dim)
    lab, lb = labels_of(kind, dim)
    spt = (64, 24, 2)
    sp = ph.SearchParameters(*spt)
    nq = 2100  # past the batch sizes of the small-batch kernels and of the dense-only launch of a split descent
    qids = (np.arange(nq, dtype=np.uint64) * 7) % N
    want = wants(nq)
    masks = lr.masks_of(lab, want)
    ex = (qids + 1) % N
    base = hix.search_batch_labeled(qids=qids, sp=sp, labels=lb, want=want, exclude=ex, stats=True)
    same(base, hix.search_batch_filtered(qids=qids, sp=sp, allow=masks, exclude=ex, stats=True))                      # B
    same(tuple(x[:8] for x in base), fr.search(oix, dist(oix, qids=qids[:8]), spt, allow=masks[:8], exclude=ex[:8], layers=layers))  # A
    base_strict = hix.search_batch_labeled(qids=qids, sp=sp, labels=lb, want=want, exclude=ex, strict=True, stats=True)
    same(base_strict, hix.search_batch_filtered(qids=qids, sp=sp, allow=masks, exclude=ex, strict=True, stats=True))  # B
    small = hix.search_batch_labeled(qids=qids[:300], sp=sp, labels=lb, want=want[:300], exclude=ex[:300], stats=True)
    same(small, tuple(x[:300] for x in base))  # a small batch: the latency kernels on f32
    split = dict(PHNSW_TWO_LAUNCH_MIN="1", PHNSW_SPLIT_BYTES="1")
    count = lib().phnsw_debug_two_launch_count
    count.restype = C.c_uint64
    settings = [dict(PHNSW_NO_TINY="1"), dict(PHNSW_VISITED="global"), dict(PHNSW_NO_LAT="1"),
                dict(PHNSW_TINY_TABLE_BYTES=str(300 * 4 * N)),  # the table holds ~300 queries: chunks of the list
                dict(PHNSW_HOST_CHUNKS="0,100,250"),
                dict(split, PHNSW_TINY_MAX="200"), dict(split, PHNSW_NO_TINY="1"), dict(split, PHNSW_NO_LOCALITY="1")]
    for kv in settings:
        with env(monkeypatch, **kv):
            before = count()
            same(hix.search_batch_labeled(qids=qids, sp=sp, labels=lb, want=want, exclude=ex, stats=True), base)
            if "PHNSW_NO_LAT" in kv:
                same(hix.search_batch_labeled(qids=qids[:300], sp=sp, labels=lb, want=want[:300], exclude=ex[:300], stats=True),
                     tuple(x[:300] for x in base))
            if "PHNSW_TWO_LAUNCH_MIN" in kv:  # the split descent ran, or PHNSW_NO_LOCALITY switched it off
                assert (count() == before) == ("PHNSW_NO_LOCALITY" in kv)
            if "PHNSW_TINY_TABLE_BYTES" in kv:  # the wanted labels followed the chunks of the list
                assert lib().phnsw_debug_last_search_chunks(hix._h) > 1
            same(hix.search_batch_labeled(qids=qids, sp=sp, labels=lb, want=want, exclude=ex, strict=True, stats=True), base_strict)


# ---------------------------------------------------------------- 4: unlisted vectors, a non-identity vec2node
def test_an_index_over_every_second_vector():
    w = ta.world("f32", 24, 2)
    hix, n = w["hix"], ta.N
    lab = column(n, int(w["entry"]), seed=5)  # odd rows carry labels too, and the index does not hold them: unlisted
    lb = ph.Labels(hix, lab)
    assert lb.listed == int((lab[::2] != NONE).sum()) < int((lab != NONE).sum())
    want = wants(ta.NQ)
    listed = lr.masks_of(lab, want) & w["members"][None, :]
    sp = ph.SearchParameters(64, 24, 2)
    for kw in (dict(queries=w["q"]), dict(qids=w["qids"])):
        for strict in (False, True):
            got = hix.search_batch_labeled(sp=sp, labels=lb, want=want, strict=strict, stats=True, **kw)
            same(got, hix.search_batch_filtered(sp=sp, allow=listed, strict=strict, stats=True, **kw))                # B
        ids = got[0][got[0] != EMPTY].astype(np.int64)
        assert len(ids) and not (ids % 2).any()  # strict: listed vectors only
        rows = np.repeat(np.arange(ta.NQ), got[2].astype(np.int64))
        assert listed[rows, np.concatenate([got[0][i, :int(got[2][i])] for i in range(ta.NQ)]).astype(np.int64)].all()
    # a wanted NONE does not match the unlisted vectors, which carry NONE in the handle's column
    none = hix.search_batch_labeled(queries=w["q"], sp=sp, labels=lb, want=np.full(ta.NQ, -1), strict=True)
    assert not none[2].any() and (none[0] == EMPTY).all()


# ---------------------------------------------------------------- 5: an empty want
def test_none_and_an_absent_label_give_the_rows_of_an_all_zero_bitmap():
    hix, oix, layers, g = world("f32", 100)
    lab, lb = labels_of("f32", 100)
    sp = ph.SearchParameters(64, 64, 2)
    q = raw_queries("f32", 100, NQ)
    zero = np.zeros((NQ, N), dtype=bool)
    for w in (np.full(NQ, NONE, dtype=np.uint64), np.full(NQ, -1), np.full(NQ, ABSENT)):
        for strict in (False, True):
            got = hix.search_batch_labeled(queries=q, sp=sp, labels=lb, want=w, strict=strict, stats=True)
            same(got, hix.search_batch_filtered(queries=q, sp=sp, allow=zero, strict=strict, stats=True))             # B
            if strict:
                assert not got[2].any() and (got[0] == EMPTY).all() and (bits(got[1]) == bits(fr.FMAX)).all()
            else:  # the entry vector enters before any filter runs
                assert ((got[0] == g.entry_vector()).sum(axis=1) == got[2]).all()
        dv = device_walk(hix, lb, sp, queries=q, want=w, strict=True)
        assert not dv[4].any() and not dv[2].any() and (dv[0] == EMPTY).all()


# ---------------------------------------------------------------- 6: the device form on a stream of its own
def test_device_form_on_a_side_stream():
    import torch
    hix = world("f32", 100)[0]
    lab, lb = labels_of("f32", 100)
    sp = ph.SearchParameters(128, 32, 2)
    qids = (np.arange(70, dtype=np.uint64) * 29 + 3) % N
    want = wants(70, shift=3)
    ex = (qids + 2) % N
    stream = torch.cuda.Stream()
    for strict in (False, True):
        host = hix.search_batch_labeled(qids=qids, sp=sp, labels=lb, want=want, exclude=ex, strict=strict, stats=True)
        dv = device_walk(hix, lb, sp, qids=qids, want=want, exclude=ex, strict=strict, stream=stream.cuda_stream)
        assert set(dv[4].tolist()) == {0}
        same(dv, host)
    one = device_walk(hix, lb, sp, qids=qids[:40], want=want[:40], upto=1, stream=stream.cuda_stream)
    same(one, hix.search_batch_filtered(qids=qids[:40], sp=sp, allow=lr.masks_of(lab, want[:40]), upto=1, stats=True))  # B


# ---------------------------------------------------------------- 7: argument checks
def test_argument_checks():
    hix = world("f32", 100)[0]
    lab, lb = labels_of("f32", 100)
    sp = ph.SearchParameters(16, 16, 2)
    q = raw_queries("f32", 100, 4)
    want = wants(4)
    other = ph.Hnsw.from_layers(hix.store, ring(np.arange(N)))  # a handle of another index over the same store
    for call in (lambda: other.search_batch_labeled(queries=q, sp=sp, labels=lb, want=want),
                 lambda: other.search_batch_labeled_device(lb, 4, sp, 8, 8, 8, 8, qids=8, want=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == E_INVALID and "the labels are stale" in str(e.value) and "another index" in str(e.value)
        assert "phnsw_search_batch_labeled" in str(e.value)
    # the device form: no want, both of queries and qids, neither
    for bad in (dict(qids=8), dict(queries=16, ldq=hix.store.ld, qids=8, want=8), dict(want=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_batch_labeled_device(lb, 4, sp, 8, 8, 8, 8, **bad)
        assert e.value.code == E_INVALID and "phnsw_search_batch_labeled_device: invalid argument" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # a null want reaches the host form only past the wrapper
        check(lib().phnsw_search_batch_labeled(hix._h, lb._h, q.ctypes.data_as(C.c_void_p), None, 4, C.byref(sp), 0, None, None,
                                               0, 0, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None))
    assert "phnsw_search_batch_labeled: invalid argument" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # k past the queue
        hix.search_batch_labeled(queries=q, sp=sp, labels=lb, want=want, k=17)
    assert e.value.code == E_INVALID and "k must be 0" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # the parameters come first
        hix.search_batch_labeled(queries=q, sp=ph.SearchParameters(1025, 16, 2), labels=lb, want=want)
    assert e.value.code == E_INVALID and "number_of_candidates" in str(e.value)
    ids, d, ln = hix.search_batch_labeled(queries=np.zeros((0, 100), dtype=np.float32), sp=sp, labels=lb,
                                          want=np.zeros(0, dtype=np.int64))
    assert ids.shape == (0, 16)  # nq == 0: a no-op
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses a Stored query id at or past n
        hix.search_batch_labeled(qids=np.array([N], dtype=np.uint64), sp=sp, labels=lb, want=np.array([HALF]))
    assert e.value.code == E_INVALID and "out of range" in str(e.value)


def test_a_handle_is_stale_after_the_store_has_grown():
    rows = oracle.synth_rows(0, 300, 24)[:, :24].copy()
    store = ph.VectorStore(rows[:200], metric=COS)
    hix = ph.Hnsw.from_layers(store, ring(np.arange(200)))
    lab = np.arange(200) % 4
    lb = ph.Labels(hix, lab)
    sp = ph.SearchParameters(16, 16, 2)
    want = np.array([0, 1, 2])
    got = hix.search_batch_labeled(queries=rows[:3], sp=sp, labels=lb, want=want, stats=True)
    same(got, hix.search_batch_filtered(queries=rows[:3], sp=sp, allow=lr.masks_of(lab, want), stats=True))
    store.append(rows[200:])
    for call in (lambda: hix.search_batch_labeled(queries=rows[:3], sp=sp, labels=lb, want=want),
                 lambda: hix.search_batch_labeled_device(lb, 3, sp, 8, 8, 8, 8, qids=8, want=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == E_INVALID and "the labels are stale" in str(e.value)
    lab2 = np.concatenate([lab, np.full(100, 1)])
    lb2 = ph.Labels(hix, lab2)  # a new handle: the appended vectors are not in the index, so they are not listed
    got = hix.search_batch_labeled(queries=rows[:3], sp=sp, labels=lb2, want=want, strict=True, stats=True)
    same(got, hix.search_batch_filtered(queries=rows[:3], sp=sp, allow=lr.masks_of(lab2, want) & (np.arange(300) < 200), strict=True,
                                        stats=True))
    assert (got[0][got[0] != EMPTY] < 200).all()
