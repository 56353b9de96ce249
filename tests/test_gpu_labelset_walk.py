"""phnsw_search_batch_labelset[_device]: the graph walk restricted by a SET of row labels per query, on the search
kernels' set mode.  Every comparison is on ids, distance bits, lengths, stats and statuses; none has a tolerance.

Yardsticks, named per assertion below:
  * A -- tests/filter_reference.search, the restatement of search_layers / closest_vectors over the oracle's distances,
         with the masks tests/labelset_reference.masks_of_sets makes of the label column and the sets: masks the code
         under test never saw.
  * B -- search_batch_filtered with those masks as per-query bitmaps: rows, lengths and stats must be equal bit for bit.

The world is that of tests/test_gpu_labeled_walk.py (N = 2000, its column()) and, for unlisted vectors, the
every-second-vector index of tests/test_gpu_filter_auto.py (N = 5000)."""
import ctypes as C

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd._lib import check, lib

import filter_reference as fr
import labelset_reference as sr
import test_gpu_filter_auto as ta
from test_gpu_exact_filter import ring
from test_gpu_filter import EMPTY, KINDS, N, dist, raw_queries, same, world
from test_gpu_i8q import env
from test_gpu_labeled_walk import (ABSENT, HALF, HUNDREDTH, L64, L65, NONE, ONE, TENTH, TOP, ZERO, column, labels_of)

pytestmark = pytest.mark.gpu

E_INVALID = -1
NQ = 22
# what the queries want, in turn.  The last two: a match past one chunk of 64 labels, and a long set with duplicates whose
# only carried label is its last entry
SETS = [[], [ONE], [HALF], [L64, L65], [L64, L64, ONE], [ABSENT, NONE], [NONE], [TENTH, HUNDREDTH, ZERO, TOP],
        [HALF, TENTH, HUNDREDTH, ZERO, ONE, L64, L65, TOP, NONE],
        [2000 + i for i in range(64)] + [HALF],
        [3000 + i % 50 for i in range(199)] + [TENTH]]


def sets_of(nq, shift=0):
    return [SETS[(i + shift) % len(SETS)] for i in range(nq)]


def masks_for(lab, sets):
    """bool [nq, n] by tests/labelset_reference.masks_of_sets: computed once per distinct set, shared by the queries"""
    distinct = sorted({tuple(s) for s in sets})
    first, values = sr.csr([list(s) for s in distinct])
    m = sr.masks_of_sets(lab, first, values)
    at = {s: i for i, s in enumerate(distinct)}
    return m[[at[tuple(s)] for s in sets]]


def test_the_sets_are_what_the_docstring_says():
    lab, _ = labels_of("f32", 100)
    m = masks_for(lab, SETS)
    counts = m.sum(axis=1).tolist()
    half = int((lab == HALF).sum())
    assert counts == [0, 1, half, 129, 65, 0, 0, 200 + 20 + 520 + 30, N - 100, half, 200]
    assert len(SETS[9]) == 65 and len(SETS[10]) == 200 and len(set(SETS[10])) < 200


def device_walk(hix, lb, sp, queries=None, qids=None, want=None, exclude=None, strict=False, upto=0, stream=0, first=None,
                nwant=None):
    """phnsw_search_batch_labelset_device with torch buffers -> ids u64, d, len u64, stats u64, status; 64 guard words
    behind every output must come back as they went in.  first / nwant: offsets and a table length of the test's own in
    place of the packed ones (the values stay those of `want`)"""
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
    f32, v32 = ph.hnsw.pack_label_sets(want, nq)
    if first is not None:
        f32 = np.asarray(first, dtype=np.uint32)
    nw = len(v32) if nwant is None else nwant
    fd = up(f32, np.int32).data_ptr()
    vd = up(v32, np.int32).data_ptr() if len(v32) else 0
    G = 64
    ids = torch.full((nq * ef + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * ef + G,), -1.0, dtype=torch.float32, device=dev)
    ln, status = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(2))
    st = torch.full((2 * nq + G,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    hix.search_batch_labelset_device(lb, nq, nw, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd,
                                     ldq=ld, qids=qi, exclude=ex, want_first=fd, want_values=vd, strict=strict,
                                     out_stats=st.data_ptr(), upto=upto, stream=stream)
    torch.cuda.synchronize()
    assert (ids[nq * ef:] == 7).all() and (d[nq * ef:] == -1.0).all()
    assert (ln[nq:] == -1).all() and (status[nq:] == -1).all() and (st[2 * nq:] == -1).all()
    i64 = ids[:nq * ef].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, ef)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return (i64, d[:nq * ef].cpu().numpy().reshape(nq, ef), ln[:nq].cpu().numpy().view(np.uint32).astype(np.uint64),
            st[:2 * nq].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, 2), status[:nq].cpu().numpy())


# ---------------------------------------------------------------- 1: both yardsticks, every twin family
@pytest.mark.parametrize("kind,dim", KINDS)
def test_the_set_walk_equals_the_restatement_and_the_bitmap_walk(kind, dim):
    hix, oix, layers, g = world(kind, dim)
    lab, lb = labels_of(kind, dim)
    spt = (64, 24, 2)
    sp = ph.SearchParameters(*spt)
    want = sets_of(NQ)
    masks = masks_for(lab, want)
    q = raw_queries(kind, dim, NQ)
    qids = np.arange(11, N, N // NQ, dtype=np.uint64)[:NQ]
    # exclude: a listed vector of a wanted label where there is one (it matters), else any id
    ex = np.array([np.nonzero(masks[i])[0][i % 3 % max(int(masks[i].sum()), 1)] if masks[i].any() else i for i in range(NQ)],
                  dtype=np.uint64)
    seen_entry = False
    for kw in (dict(queries=q), dict(qids=qids)):
        D = None if oix is None else dist(oix, **kw)
        for upto in (0, 1, 2):
            for e in (None, ex):
                got = hix.search_batch_labelset(sp=sp, labels=lb, want=want, exclude=e, upto=upto, stats=True, **kw)
                same(got, hix.search_batch_filtered(sp=sp, allow=masks, exclude=e, upto=upto, stats=True, **kw))       # B
                strict = hix.search_batch_labelset(sp=sp, labels=lb, want=want, strict=True, exclude=e, upto=upto, stats=True, **kw)
                same(strict, hix.search_batch_filtered(sp=sp, allow=masks, strict=True, exclude=e, upto=upto, stats=True, **kw))  # B
                if oix is not None:
                    ref = fr.search(oix, D, spt, allow=masks, exclude=e, upto=upto, layers=layers)
                    same(got, ref)                                                                                     # A
                    same(strict, fr.strict(ref, masks), stats=False)                                                   # A
                    np.testing.assert_array_equal(strict[3], ref[3])  # strict drops ids after the walk: the same stats
                seen_entry |= bool(((got[0] == g.entry_vector()) & ~masks[:, int(g.entry_vector())][:, None]).any())
        cut = hix.search_batch_labelset(sp=sp, labels=lb, want=want, exclude=ex, k=5, **kw)                            # the k cut
        same(cut, hix.search_batch_filtered(sp=sp, allow=masks, exclude=ex, k=5, **kw))
        whole = hix.search_batch_labelset(sp=sp, labels=lb, want=want, exclude=ex, **kw)
        assert cut[0].shape == (NQ, 5) and whole[0].shape == (NQ, 64)
        np.testing.assert_array_equal(cut[0], whole[0][:, :5])
        np.testing.assert_array_equal(cut[2], np.minimum(whole[2], 5))
        dv = device_walk(hix, lb, sp, want=want, exclude=ex, **kw)
        assert not dv[4].any()
        same(dv, hix.search_batch_labelset(sp=sp, labels=lb, want=want, exclude=ex, stats=True, **kw))
    # the entry vector carries HALF: returned to queries whose set does not hold HALF, unless strict (asserted by B and A)
    assert seen_entry


# ---------------------------------------------------------------- 2: every queue capacity class
@pytest.mark.parametrize("ef", [64, 128, 256, 512])
def test_queue_capacity_classes(monkeypatch, ef):
    hix = world("f32", 100)[0]
    lab, lb = labels_of("f32", 100)
    q = raw_queries("f32", 100, 12)
    want = sets_of(12, shift=ef // 64)
    masks = masks_for(lab, want)
    sp = ph.SearchParameters(ef, ef, 2)
    ref = hix.search_batch_filtered(queries=q, sp=sp, allow=masks, stats=True)                                        # B
    same(hix.search_batch_labelset(queries=q, sp=sp, labels=lb, want=want, stats=True), ref)
    with env(monkeypatch, PHNSW_NO_LAT="1", PHNSW_NO_TINY="1"):  # the throughput kernel of pick_kernel_rows, rows gathered per hop
        same(hix.search_batch_labelset(queries=q, sp=sp, labels=lb, want=want, stats=True), ref)
        same(hix.search_batch_labelset(queries=q, sp=sp, labels=lb, want=want, strict=True, stats=True),
             hix.search_batch_filtered(queries=q, sp=sp, allow=masks, strict=True, stats=True))


# ---------------------------------------------------------------- 3: independence of the schedule
def test_set_results_do_not_depend_on_the_schedule(monkeypatch):
    hix, oix, layers, _ = world("f32", 100)
    lab, lb = labels_of("f32", 100)
    spt = (64, 24, 2)
    sp = ph.SearchParameters(*spt)
    nq = 2100  # past the batch sizes of the small-batch kernels and of the dense-only launch of a split descent
    qids = (np.arange(nq, dtype=np.uint64) * 7) % N
    want = sets_of(nq)
    masks = masks_for(lab, want)
    ex = (qids + 1) % N
    base = hix.search_batch_labelset(qids=qids, sp=sp, labels=lb, want=want, exclude=ex, stats=True)
    same(base, hix.search_batch_filtered(qids=qids, sp=sp, allow=masks, exclude=ex, stats=True))                      # B
    same(tuple(x[:11] for x in base), fr.search(oix, dist(oix, qids=qids[:11]), spt, allow=masks[:11], exclude=ex[:11], layers=layers))  # A
    base_strict = hix.search_batch_labelset(qids=qids, sp=sp, labels=lb, want=want, exclude=ex, strict=True, stats=True)
    same(base_strict, hix.search_batch_filtered(qids=qids, sp=sp, allow=masks, exclude=ex, strict=True, stats=True))  # B
    small = hix.search_batch_labelset(qids=qids[:300], sp=sp, labels=lb, want=want[:300], exclude=ex[:300], stats=True)
    same(small, tuple(x[:300] for x in base))  # a small batch: the latency kernels on f32
    split = dict(PHNSW_TWO_LAUNCH_MIN="1", PHNSW_SPLIT_BYTES="1")
    count = lib().phnsw_debug_two_launch_count
    count.restype = C.c_uint64
    # The last two cut the query list into chunks (the dense table holds ~300, then ~700 queries): set_first follows the
    # chunk, the offsets stay absolute.  The host form by set stages its arrays once and does not go through the chunk
    # plan PHNSW_HOST_CHUNKS steers, so that knob alone makes no chunk here: it is given together with a small table.
    settings = [dict(split, PHNSW_TINY_MAX="200"), dict(split, PHNSW_NO_TINY="1"), dict(PHNSW_NO_TINY="1"),
                dict(PHNSW_VISITED="global"), dict(PHNSW_NO_LAT="1"),
                dict(PHNSW_TINY_TABLE_BYTES=str(300 * 4 * N)),
                dict(PHNSW_HOST_CHUNKS="0,100,250", PHNSW_TINY_TABLE_BYTES=str(700 * 4 * N))]
    for kv in settings:
        with env(monkeypatch, **kv):
            before = count()
            same(hix.search_batch_labelset(qids=qids, sp=sp, labels=lb, want=want, exclude=ex, stats=True), base)
            if "PHNSW_TWO_LAUNCH_MIN" in kv:
                assert count() > before  # the split descent ran
            if "PHNSW_TINY_TABLE_BYTES" in kv:  # the offsets followed the chunks of the list
                assert lib().phnsw_debug_last_search_chunks(hix._h) > 1
            same(hix.search_batch_labelset(qids=qids, sp=sp, labels=lb, want=want, exclude=ex, strict=True, stats=True), base_strict)


# ---------------------------------------------------------------- 4: the order of the batch and the order inside a set
def test_permuting_the_batch_permutes_the_rows_and_the_order_inside_a_set_does_not_matter():
    hix = world("f32", 100)[0]
    lab, lb = labels_of("f32", 100)
    sp = ph.SearchParameters(64, 24, 2)
    nq = 2 * len(SETS)
    q = raw_queries("f32", 100, nq)
    want = sets_of(nq, shift=2)
    base = hix.search_batch_labelset(queries=q, sp=sp, labels=lb, want=want, stats=True)
    rng = np.random.default_rng(11)
    perm = rng.permutation(nq)
    got = hix.search_batch_labelset(queries=q[perm], sp=sp, labels=lb, want=[want[i] for i in perm], stats=True)
    same(got, tuple(x[perm] for x in base))
    rev = [list(reversed(s)) for s in want]
    same(hix.search_batch_labelset(queries=q, sp=sp, labels=lb, want=rev, stats=True), base)
    shuffled = [list(rng.permutation(np.array(s, dtype=np.int64))) if len(s) else [] for s in want]
    same(hix.search_batch_labelset(queries=q, sp=sp, labels=lb, want=shuffled, stats=True), base)
    same(hix.search_batch_labelset(queries=q, sp=sp, labels=lb, want=shuffled, strict=True, stats=True),
         hix.search_batch_labelset(queries=q, sp=sp, labels=lb, want=want, strict=True, stats=True))


# ---------------------------------------------------------------- 5: one label per set is the walk by label
def test_one_label_sets_equal_the_walk_by_label():
    hix = world("f32", 100)[0]
    lab, lb = labels_of("f32", 100)
    sp = ph.SearchParameters(64, 24, 2)
    one = np.array([[HALF, TENTH, HUNDREDTH, ONE, L64, L65, TOP, ABSENT, NONE, ZERO][i % 10] for i in range(30)], dtype=np.int64)
    qids = (np.arange(30, dtype=np.uint64) * 61 + 5) % N
    for strict in (False, True):
        same(hix.search_batch_labelset(qids=qids, sp=sp, labels=lb, want=[[int(w)] for w in one], strict=strict, stats=True),
             hix.search_batch_labeled(qids=qids, sp=sp, labels=lb, want=one, strict=strict, stats=True))


# ---------------------------------------------------------------- 6: unlisted vectors, a non-identity vec2node
def test_an_index_over_every_second_vector():
    w = ta.world("f32", 24, 2)
    hix, n = w["hix"], ta.N
    lab = column(n, int(w["entry"]), seed=5)  # odd rows carry labels too, and the index does not hold them: unlisted
    lb = ph.Labels(hix, lab)
    want = sets_of(ta.NQ)
    listed = masks_for(lab, want) & w["members"][None, :]
    sp = ph.SearchParameters(64, 24, 2)
    for kw in (dict(queries=w["q"]), dict(qids=w["qids"])):
        for strict in (False, True):
            got = hix.search_batch_labelset(sp=sp, labels=lb, want=want, strict=strict, stats=True, **kw)
            same(got, hix.search_batch_filtered(sp=sp, allow=listed, strict=strict, stats=True, **kw))                # B
        ids = got[0][got[0] != EMPTY].astype(np.int64)
        assert len(ids) and not (ids % 2).any()  # strict: listed vectors only
    # a set of NONE does not match the unlisted vectors, which carry NONE in the handle's column
    none = hix.search_batch_labelset(queries=w["q"], sp=sp, labels=lb, want=[[-1, NONE]] * ta.NQ, strict=True)
    assert not none[2].any() and (none[0] == EMPTY).all()


# ---------------------------------------------------------------- 7: the device form on a side stream; unsound offsets
def test_device_form_on_a_side_stream_and_offsets_that_are_not_sound():
    import torch
    hix = world("f32", 100)[0]
    lab, lb = labels_of("f32", 100)
    sp = ph.SearchParameters(128, 32, 2)
    nq = 44
    qids = (np.arange(nq, dtype=np.uint64) * 29 + 3) % N
    want = sets_of(nq, shift=3)
    ex = (qids + 2) % N
    stream = torch.cuda.Stream()
    for strict in (False, True):
        host = hix.search_batch_labelset(qids=qids, sp=sp, labels=lb, want=want, exclude=ex, strict=strict, stats=True)
        dv = device_walk(hix, lb, sp, qids=qids, want=want, exclude=ex, strict=strict, stream=stream.cuda_stream)
        assert set(dv[4].tolist()) == {0}
        same(dv, host)
    # Offsets that are not sound, each spoiling only its own query.  CSR shares an offset between neighbours, so the sets
    # the OTHER queries want are read off the spoiled offsets themselves: query `back` runs backwards (its end is pulled
    # below its start, which makes the range of the query behind it longer, and still sound), the last query ends one
    # past nwant.
    first, values = ph.hnsw.pack_label_sets(want, nq)
    nwant = len(values)
    back = 12
    assert first[back] >= 1 and first[back + 1] > first[back]
    f = first.astype(np.int64).copy()
    f[back + 1] = f[back] - 1
    f[nq] = nwant + 1
    bad = [back, nq - 1]
    assert f[back] > f[back + 1] and f[nq - 1] <= nwant < f[nq]
    meant = [[] if q in bad else [int(v) for v in values[f[q]:f[q + 1]]] for q in range(nq)]
    assert meant[back + 1] != want[back + 1] and all(0 <= f[q] <= f[q + 1] <= nwant for q in range(nq) if q not in bad)
    for strict in (False, True):
        sound = device_walk(hix, lb, sp, qids=qids, want=meant, exclude=ex, strict=strict, stream=stream.cuda_stream)
        assert not sound[4].any()
        same(sound, hix.search_batch_filtered(qids=qids, sp=sp, allow=masks_for(lab, meant), exclude=ex, strict=strict, stats=True))  # B
        got = device_walk(hix, lb, sp, qids=qids, want=want, exclude=ex, strict=strict, stream=stream.cuda_stream,
                          first=f.astype(np.uint32), nwant=nwant)
        ok = np.ones(nq, dtype=bool)
        ok[bad] = False
        assert (got[4][bad] == 8).all() and not got[4][ok].any()
        assert not got[2][bad].any() and (got[0][bad] == EMPTY).all() and not got[3][bad].any()
        assert (got[1][bad].view(np.uint32) == np.float32(fr.FMAX).view(np.uint32)).all()
        same(tuple(x[ok] for x in got), tuple(x[ok] for x in sound))


# ---------------------------------------------------------------- 8: argument checks
def test_argument_checks():
    hix = world("f32", 100)[0]
    lab, lb = labels_of("f32", 100)
    sp = ph.SearchParameters(16, 16, 2)
    q = raw_queries("f32", 100, 4)
    want = sets_of(4, shift=1)
    first, values = ph.hnsw.pack_label_sets(want, 4)
    other = ph.Hnsw.from_layers(hix.store, ring(np.arange(N)))  # a handle of another index over the same store
    for call in (lambda: other.search_batch_labelset(queries=q, sp=sp, labels=lb, want=want),
                 lambda: other.search_batch_labelset_device(lb, 4, 4, sp, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == E_INVALID and "the labels are stale" in str(e.value) and "another index" in str(e.value)
        assert "phnsw_search_batch_labelset" in str(e.value)
    # the device form: no want_first, want_values null with nwant > 0, both of queries and qids, neither
    for bad in (dict(qids=8, want_values=8), dict(qids=8, want_first=8),
                dict(queries=16, ldq=hix.store.ld, qids=8, want_first=8, want_values=8), dict(want_first=8, want_values=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_batch_labelset_device(lb, 4, 4, sp, 8, 8, 8, 8, **bad)
        assert e.value.code == E_INVALID and "phnsw_search_batch_labelset_device: invalid argument" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # nwant past 2^31 - 2
        hix.search_batch_labelset_device(lb, 4, 2 ** 31 - 1, sp, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)
    assert e.value.code == E_INVALID and "phnsw_search_batch_labelset_device: nq and nwant" in str(e.value)
    qp = q.ctypes.data_as(C.c_void_p)
    fp, vp = first.ctypes.data_as(C.c_void_p), values.ctypes.data_as(C.c_void_p)
    host = lib().phnsw_search_batch_labelset
    with pytest.raises(ph.PhnswError) as e:  # a null want_first reaches the host form only past the wrapper
        check(host(hix._h, lb._h, qp, None, 4, C.byref(sp), 0, None, None, vp, 0, 0, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None))
    assert "phnsw_search_batch_labelset: invalid argument" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # want_values null although want_first[nq] > 0
        check(host(hix._h, lb._h, qp, None, 4, C.byref(sp), 0, None, fp, None, 0, 0, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None))
    assert "phnsw_search_batch_labelset: invalid argument (want_values" in str(e.value)
    for kw in (dict(), dict(queries=q, qids=np.arange(4, dtype=np.uint64))):  # neither, both: the wrapper refuses them ...
        with pytest.raises(ValueError):
            hix.search_batch_labelset(sp=sp, labels=lb, want=want, **kw)
    with pytest.raises(ph.PhnswError) as e:  # ... and so does the library
        check(host(hix._h, lb._h, None, None, 4, C.byref(sp), 0, None, fp, vp, 0, 0, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None))
    assert "phnsw_search_batch_labelset: pass queries or qids" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # k past the queue
        hix.search_batch_labelset(queries=q, sp=sp, labels=lb, want=want, k=17)
    assert e.value.code == E_INVALID and "k must be 0" in str(e.value) and "phnsw_search_batch_labelset" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # the parameters come first
        other.search_batch_labelset(queries=q, sp=ph.SearchParameters(1025, 16, 2), labels=lb, want=want)
    assert e.value.code == E_INVALID and "number_of_candidates" in str(e.value) and "stale" not in str(e.value)
    ids, d, ln = hix.search_batch_labelset(queries=np.zeros((0, 100), dtype=np.float32), sp=sp, labels=lb, want=[])
    assert ids.shape == (0, 16)  # nq == 0: a no-op
    # the host form refuses, naming the query, before any device work
    with pytest.raises(ph.PhnswError) as e:
        hix.search_batch_labelset(qids=np.array([3, N], dtype=np.uint64), sp=sp, labels=lb, want=[[HALF], [HALF]])
    assert e.value.code == E_INVALID and "phnsw_search_batch_labelset: query 1" in str(e.value) and "out of range" in str(e.value)
    q2 = q.ctypes.data_as(C.c_void_p)
    for bad_first, who in ((np.array([1, 1, 2, 3, 3], dtype=np.uint32), "query 0"),
                           (np.array([0, 2, 1, 3, 3], dtype=np.uint32), "query 1")):
        with pytest.raises(ph.PhnswError) as e:
            check(host(hix._h, lb._h, q2, None, 4, C.byref(sp), 0, None, bad_first.ctypes.data_as(C.c_void_p), vp, 0, 0,
                       C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None))
        assert e.value.code == E_INVALID and "phnsw_search_batch_labelset: " + who in str(e.value)
        assert "never run backwards" in str(e.value)


def test_a_handle_is_stale_after_the_store_has_grown():
    import oracle
    from test_gpu_filter import COS
    rows = oracle.synth_rows(0, 300, 24)[:, :24].copy()
    store = ph.VectorStore(rows[:200], metric=COS)
    hix = ph.Hnsw.from_layers(store, ring(np.arange(200)))
    lab = np.arange(200) % 4
    lb = ph.Labels(hix, lab)
    sp = ph.SearchParameters(16, 16, 2)
    want = [[0, 3], [1], [2, 2]]
    got = hix.search_batch_labelset(queries=rows[:3], sp=sp, labels=lb, want=want, stats=True)
    same(got, hix.search_batch_filtered(queries=rows[:3], sp=sp, allow=masks_for(lab, want), stats=True))
    store.append(rows[200:])
    for call in (lambda: hix.search_batch_labelset(queries=rows[:3], sp=sp, labels=lb, want=want),
                 lambda: hix.search_batch_labelset_device(lb, 3, 5, sp, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == E_INVALID and "the labels are stale" in str(e.value)
