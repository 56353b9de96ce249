"""phnsw_search_batch_labelset_ranged[_device]: the graph walk restricted by a SET of row labels and a numeric range, on
the search kernels' set-range mode (search_labelset_ranged.hip).  Every comparison is on ids, distance bits, lengths,
stats and statuses; none has a tolerance.

Yardsticks, named per assertion below:
  * A -- tests/filter_reference.search, the restatement of search_layers / closest_vectors over the oracle's distances,
         with the masks tests/labelset_ranged_reference.masks_of makes of the two columns and the sets: masks the code
         under test never saw.
  * B -- search_batch_filtered with those masks as per-query bitmaps: rows, lengths and stats must be equal bit for bit.

The worlds, the two columns, the eleven sets and the twelve ranges are those of tests/test_gpu_exact_labelset_ranged.py
(N = 2000, built multi-layer graphs; the entry vector carries label 4 at rank 1500), and the every-second-vector index of
tests/test_gpu_filter_auto.py."""
import ctypes as C

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd._lib import check, lib

import filter_reference as fr
import labelset_ranged_reference as sr
import test_gpu_filter_auto as ta
from test_gpu_exact_filter import ring
from test_gpu_exact_labelset_ranged import LABELS, NONE, RANGES, SETS, attr_of, batch, csr, label_column, labeled_attribute
from test_gpu_filter import EMPTY, KINDS, N, dist, raw_queries, same, world
from test_gpu_i8 import bits
from test_gpu_i8q import env
from test_gpu_ranged_walk import column, values_of

pytestmark = pytest.mark.gpu

NQ = 33  # three rounds of the sets, nearly three of the ranges
E_INVALID = -1


def device_walk(hix, at, sp, first, values, lo, hi, queries=None, qids=None, exclude=None, strict=False, upto=0, stream=0,
                nwant=None):
    """phnsw_search_batch_labelset_ranged_device with torch buffers -> ids u64, d, len u64, stats u64, status; 64 guard
    words behind every output must come back as they went in"""
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
    fd, lod, hid = (up(np.asarray(x, dtype=np.uint32), np.int32).data_ptr() for x in (first, lo, hi))
    vd = up(np.asarray(values, dtype=np.uint32), np.int32).data_ptr() if len(values) else 0
    G = 64
    ids = torch.full((nq * ef + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * ef + G,), -1.0, dtype=torch.float32, device=dev)
    ln, status = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(2))
    st = torch.full((2 * nq + G,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    hix.search_batch_labelset_ranged_device(at, nq, len(values) if nwant is None else nwant, sp, ids.data_ptr(), d.data_ptr(),
                                            ln.data_ptr(), status.data_ptr(), queries=qd, ldq=ld, qids=qi, exclude=ex,
                                            want_first=fd, want_values=vd, lo=lod, hi=hid, strict=strict,
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
def test_the_walk_equals_the_restatement_and_the_bitmap_walk(kind, dim):
    hix, oix, layers, g = world(kind, dim)
    labels, keys, at = attr_of(kind, dim)
    spt = (64, 24, 2)
    sp = ph.SearchParameters(*spt)
    sets, lo, hi = batch(NQ)
    vlo, vhi = values_of(lo), values_of(hi)
    masks = sr.masks_of(labels, keys, sets, lo, hi)
    q = raw_queries(kind, dim, NQ)
    qids = np.arange(11, N, N // NQ, dtype=np.uint64)[:NQ]
    # exclude: a vector inside the spans where there is one (it matters), else any id
    ex = np.array([np.nonzero(masks[i])[0][i % 3 % max(int(masks[i].sum()), 1)] if masks[i].any() else i for i in range(NQ)],
                  dtype=np.uint64)
    seen_entry = False
    for kw in (dict(queries=q), dict(qids=qids)):
        D = None if oix is None else dist(oix, **kw)
        for upto in (0, 1, 2):
            for e in (None, ex):
                a = dict(sp=sp, attr=at, want=sets, lo=vlo, hi=vhi, exclude=e, upto=upto, stats=True, **kw)
                b = dict(sp=sp, allow=masks, exclude=e, upto=upto, stats=True, **kw)
                got = hix.search_batch_labelset_ranged(**a)  # k = 0: the whole queue
                same(got, hix.search_batch_filtered(**b))                                                             # B
                strict = hix.search_batch_labelset_ranged(strict=True, **a)
                same(strict, hix.search_batch_filtered(strict=True, **b))                                             # B
                if oix is not None:
                    ref = fr.search(oix, D, spt, allow=masks, exclude=e, upto=upto, layers=layers)
                    same(got, ref)                                                                                    # A
                    same(strict, fr.strict(ref, masks), stats=False)                                                  # A
                    np.testing.assert_array_equal(strict[3], ref[3])  # strict drops ids after the walk: the same stats
                seen_entry |= bool(((got[0] == g.entry_vector()) & ~masks[:, int(g.entry_vector())][:, None]).any())
        for strict in (False, True):
            cut = hix.search_batch_labelset_ranged(sp=sp, attr=at, want=sets, lo=vlo, hi=vhi, exclude=ex, strict=strict, k=10, **kw)
            same(cut, hix.search_batch_filtered(sp=sp, allow=masks, exclude=ex, strict=strict, k=10, **kw))           # B, k = 10
            assert cut[0].shape == (NQ, 10)
            dv = device_walk(hix, at, sp, *csr(sets), lo, hi, exclude=ex, strict=strict, **kw)
            assert not dv[4].any()
            same(dv, hix.search_batch_labelset_ranged(sp=sp, attr=at, want=sets, lo=vlo, hi=vhi, exclude=ex, strict=strict, stats=True, **kw))
    # the entry vector is outside most sets and ranges: returned to their queries all the same, unless strict
    assert seen_entry


# ---------------------------------------------------------------- 2: every queue capacity class
@pytest.mark.parametrize("ef", [64, 128, 256, 512])
def test_queue_capacity_classes(monkeypatch, ef):
    hix = world("f32", 100)[0]
    labels, keys, at = attr_of("f32", 100)
    q = raw_queries("f32", 100, 12)
    sets, lo, hi = batch(12, shift=ef // 64)
    masks = sr.masks_of(labels, keys, sets, lo, hi)
    sp = ph.SearchParameters(ef, ef, 2)
    a = dict(queries=q, sp=sp, attr=at, want=sets, lo=values_of(lo), hi=values_of(hi), stats=True)
    ref = hix.search_batch_filtered(queries=q, sp=sp, allow=masks, stats=True)                                        # B
    same(hix.search_batch_labelset_ranged(**a), ref)
    with env(monkeypatch, PHNSW_NO_LAT="1", PHNSW_NO_TINY="1"):  # the throughput kernel of pick_kernel_rows, rows gathered per hop
        same(hix.search_batch_labelset_ranged(**a), ref)
        same(hix.search_batch_labelset_ranged(strict=True, **a),
             hix.search_batch_filtered(queries=q, sp=sp, allow=masks, strict=True, stats=True))


# ---------------------------------------------------------------- 3: independence of the schedule
def test_results_do_not_depend_on_the_schedule(monkeypatch):
    hix, oix, layers, _ = world("f32", 100)
    labels, keys, at = attr_of("f32", 100)
    spt = (64, 24, 2)
    sp = ph.SearchParameters(*spt)
    nq = 2100  # past the batch sizes of the small-batch kernels and of the dense-only launch of a split descent
    qids = (np.arange(nq, dtype=np.uint64) * 7) % N
    sets, lo, hi = batch(nq)
    vlo, vhi = values_of(lo), values_of(hi)
    masks = sr.masks_of(labels, keys, sets, lo, hi)
    ex = (qids + 1) % N
    a = dict(qids=qids, sp=sp, attr=at, want=sets, lo=vlo, hi=vhi, exclude=ex, stats=True)
    base = hix.search_batch_labelset_ranged(**a)
    same(base, hix.search_batch_filtered(qids=qids, sp=sp, allow=masks, exclude=ex, stats=True))                      # B
    same(tuple(x[:11] for x in base), fr.search(oix, dist(oix, qids=qids[:11]), spt, allow=masks[:11], exclude=ex[:11], layers=layers))  # A
    base_strict = hix.search_batch_labelset_ranged(strict=True, **a)
    same(base_strict, hix.search_batch_filtered(qids=qids, sp=sp, allow=masks, exclude=ex, strict=True, stats=True))  # B
    small = hix.search_batch_labelset_ranged(qids=qids[:300], sp=sp, attr=at, want=sets[:300], lo=vlo[:300], hi=vhi[:300],
                                             exclude=ex[:300], stats=True)
    same(small, tuple(x[:300] for x in base))  # a small batch: the latency kernels on f32
    split = dict(PHNSW_TWO_LAUNCH_MIN="1", PHNSW_SPLIT_BYTES="1")
    count = lib().phnsw_debug_two_launch_count
    count.restype = C.c_uint64
    # the knobs of tests/test_gpu_labelset_walk.py; the last two cut the query list into chunks: the offsets of the sets and
    # the bounds follow the chunk, the offsets stay absolute
    settings = [dict(split, PHNSW_TINY_MAX="200"), dict(split, PHNSW_NO_TINY="1"), dict(PHNSW_NO_TINY="1"),
                dict(PHNSW_VISITED="global"), dict(PHNSW_NO_LAT="1"),
                dict(PHNSW_TINY_TABLE_BYTES=str(300 * 4 * N)),
                dict(PHNSW_HOST_CHUNKS="0,100,250", PHNSW_TINY_TABLE_BYTES=str(700 * 4 * N))]
    for kv in settings:
        with env(monkeypatch, **kv):
            before = count()
            same(hix.search_batch_labelset_ranged(**a), base)
            if "PHNSW_TWO_LAUNCH_MIN" in kv:
                assert count() > before  # the split descent ran
            if "PHNSW_TINY_TABLE_BYTES" in kv:  # the offsets and the bounds followed the chunks of the list
                assert lib().phnsw_debug_last_search_chunks(hix._h) > 1
            same(hix.search_batch_labelset_ranged(strict=True, **a), base_strict)


# ---------------------------------------------------------------- 4: one label per set is the walk by label and range
def test_one_label_sets_equal_the_label_range_walk():
    hix = world("f32", 100)[0]
    labels, keys, at = attr_of("f32", 100)
    sp = ph.SearchParameters(64, 24, 2)
    nq = 45
    want = np.array([(LABELS + (NONE, 5))[i % 9] for i in range(nq)], dtype=np.uint32)
    lo = np.array([RANGES[i % len(RANGES)][0] for i in range(nq)], dtype=np.uint32)
    hi = np.array([RANGES[i % len(RANGES)][1] for i in range(nq)], dtype=np.uint32)
    q = raw_queries("f32", 100, nq)
    ex = (np.arange(nq, dtype=np.uint64) * 31 + 2) % N
    for strict in (False, True):
        for upto in (0, 1):
            kw = dict(queries=q, sp=sp, attr=at, lo=values_of(lo), hi=values_of(hi), exclude=ex, strict=strict, upto=upto, stats=True)
            same(hix.search_batch_labelset_ranged(want=[[int(w)] for w in want], **kw),
                 hix.search_batch_label_ranged(want=want, **kw))  # stats included


# ---------------------------------------------------------------- 5: offsets the device form cannot trust
def test_unsound_offsets_end_their_queries_and_no_others():
    hix = world("f32", 100)[0]
    labels, keys, at = attr_of("f32", 100)
    sp = ph.SearchParameters(64, 24, 2)
    values = np.array((SETS[10] + SETS[10])[:24], dtype=np.uint32)
    nwant = len(values)
    # q4 runs backwards, q6 ends past nwant, q7 starts past nwant and runs backwards: status 8.  q5 overlaps q3: harmless
    # to a walk, every query reads its own range, and not detected
    first = np.array([0, 3, 5, 5, 9, 7, 12, nwant + 5, 14, 17, 20, 20, nwant], dtype=np.uint32)
    refused = [4, 6, 7]
    sound = [q for q in range(12) if q not in refused]
    sets12 = [values[first[q]:first[q + 1]].tolist() if q in sound else [] for q in range(12)]
    lo12 = np.array([RANGES[(q + 9) % 12][0] for q in range(12)], dtype=np.uint32)
    hi12 = np.array([RANGES[(q + 9) % 12][1] for q in range(12)], dtype=np.uint32)
    masks = sr.masks_of(labels, keys, sets12, lo12, hi12)
    assert masks[5].any() and masks[3].any()
    q = raw_queries("f32", 100, 12)
    for strict in (False, True):
        ref = hix.search_batch_filtered(queries=q, sp=sp, allow=masks, strict=strict, stats=True)
        dv = device_walk(hix, at, sp, first, values, lo12, hi12, queries=q, strict=strict, nwant=nwant)
        assert (dv[4][refused] == 8).all() and not dv[4][sound].any()
        assert not dv[2][refused].any() and (dv[0][refused] == EMPTY).all() and (bits(dv[1][refused]) == bits(fr.FMAX)).all()
        assert not dv[3][refused].any()  # stats 0
        same(tuple(x[sound] for x in dv[:4]), tuple(x[sound] for x in ref))                                          # B
    # the host form refuses offsets that run backwards, naming the query: the wrapper for a (first, values) pair, the
    # library for whoever calls it directly
    with pytest.raises(ValueError) as e:
        hix.search_batch_labelset_ranged(queries=q, sp=sp, attr=at, want=(np.minimum(first, nwant), values), lo=0, hi=5)
    assert "query 4" in str(e.value)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    back = np.minimum(first, nwant)
    l32, h32 = np.zeros(12, dtype=np.uint32), np.full(12, 5, dtype=np.uint32)
    ids, d, ln = np.zeros((12, 64), dtype=np.uint64), np.zeros((12, 64), dtype=np.float32), np.zeros(12, dtype=np.uint64)
    assert lib().phnsw_search_batch_labelset_ranged(hix._h, at._h, p(q), None, 12, C.byref(sp), 0, None, p(back), p(values), p(l32), p(h32),
                                                    0, 0, p(ids), p(d), p(ln), None) == E_INVALID
    assert lib().phnsw_last_error().decode().startswith("phnsw_search_batch_labelset_ranged: query 4: want_first must start at 0")


# ---------------------------------------------------------------- 6: unlisted vectors, a non-identity vec2node
def test_an_index_over_every_second_vector():
    w = ta.world("f32", 24, 2)
    hix = w["hix"]
    keys = column(ta.N, int(w["entry"]), seed=5, members=w["members"])  # odd rows carry labels and values too: unlisted
    labels = label_column(keys, int(w["entry"]))
    at = labeled_attribute(hix, labels, keys)
    sets, lo, hi = batch(ta.NQ, shift=2)
    vlo, vhi = values_of(lo), values_of(hi)
    listed = sr.masks_of(labels, keys, sets, lo, hi, w["members"])
    assert (sr.masks_of(labels, keys, sets, lo, hi).sum(1) > listed.sum(1)).any()
    sp = ph.SearchParameters(64, 24, 2)
    for kw in (dict(queries=w["q"]), dict(qids=w["qids"])):
        for strict in (False, True):
            got = hix.search_batch_labelset_ranged(sp=sp, attr=at, want=sets, lo=vlo, hi=vhi, strict=strict, stats=True, **kw)
            same(got, hix.search_batch_filtered(sp=sp, allow=listed, strict=strict, stats=True, **kw))                # B
        ids = got[0][got[0] != EMPTY].astype(np.int64)
        assert len(ids) and not (ids % 2).any()  # strict: listed vectors only


# ---------------------------------------------------------------- 7: the device form on a stream of its own, argument checks
def test_device_form_on_a_side_stream():
    import torch
    hix = world("f32", 100)[0]
    labels, keys, at = attr_of("f32", 100)
    sp = ph.SearchParameters(128, 32, 2)
    qids = (np.arange(70, dtype=np.uint64) * 29 + 3) % N
    sets, lo, hi = batch(70, shift=3)
    ex = (qids + 2) % N
    stream = torch.cuda.Stream()
    for strict in (False, True):
        host = hix.search_batch_labelset_ranged(qids=qids, sp=sp, attr=at, want=sets, lo=values_of(lo), hi=values_of(hi), exclude=ex,
                                                strict=strict, stats=True)
        dv = device_walk(hix, at, sp, *csr(sets), lo, hi, qids=qids, exclude=ex, strict=strict, stream=stream.cuda_stream)
        assert set(dv[4].tolist()) == {0}
        same(dv, host)
    one = device_walk(hix, at, sp, *csr(sets[:40]), lo[:40], hi[:40], qids=qids[:40], upto=1, stream=stream.cuda_stream)
    same(one, hix.search_batch_filtered(qids=qids[:40], sp=sp, allow=sr.masks_of(labels, keys, sets[:40], lo[:40], hi[:40]), upto=1,
                                        stats=True))                                                                  # B


def test_argument_checks():
    hix = world("f32", 100)[0]
    labels, keys, at = attr_of("f32", 100)
    sp = ph.SearchParameters(16, 16, 2)
    q = raw_queries("f32", 100, 4)
    sets = [[3], [3, 4], [], [5]]
    other = ph.Hnsw.from_layers(hix.store, ring(np.arange(N)))  # a handle of another index over the same store
    for call in (lambda: other.search_batch_labelset_ranged(queries=q, sp=sp, attr=at, want=sets, lo=0, hi=5),
                 lambda: other.search_batch_labelset_ranged_device(at, 4, 4, sp, 8, 8, 8, 8, qids=8, want_first=8, want_values=8, lo=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == E_INVALID and "are stale" in str(e.value) and "another index" in str(e.value)
        assert "phnsw_search_batch_labelset_ranged" in str(e.value)
    for bad in (dict(qids=8), dict(qids=8, want_values=8, lo=8, hi=8), dict(qids=8, want_first=8, lo=8, hi=8),
                dict(qids=8, want_first=8, want_values=8, lo=8), dict(qids=8, want_first=8, want_values=8, hi=8),
                dict(queries=16, ldq=hix.store.ld, qids=8, want_first=8, want_values=8, lo=8, hi=8), dict(want_first=8, want_values=8, lo=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_batch_labelset_ranged_device(at, 4, 4, sp, 8, 8, 8, 8, **bad)
        assert e.value.code == E_INVALID and "phnsw_search_batch_labelset_ranged_device: invalid argument" in str(e.value)
    qp = q.ctypes.data_as(C.c_void_p)
    for flags in (2, 0x80000000, 3):  # unknown flag bits, with and without the known one
        with pytest.raises(ph.PhnswError) as e:
            check(lib().phnsw_search_batch_labelset_ranged(hix._h, at._h, qp, None, 4, C.byref(sp), 0, None, C.c_void_p(8), C.c_void_p(8),
                                                           C.c_void_p(8), C.c_void_p(8), flags, 0, C.c_void_p(8), C.c_void_p(8),
                                                           C.c_void_p(8), None))
        assert e.value.code == E_INVALID and "unknown flag bits" in str(e.value)
        with pytest.raises(ph.PhnswError) as e:
            check(lib().phnsw_search_batch_labelset_ranged_device(hix._h, at._h, None, 0, C.c_void_p(8), 4, C.byref(sp), 0, None,
                                                                  C.c_void_p(8), C.c_void_p(8), 4, C.c_void_p(8), C.c_void_p(8), flags,
                                                                  C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None, C.c_void_p(8), None))
        assert e.value.code == E_INVALID and "unknown flag bits" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # k past the queue
        hix.search_batch_labelset_ranged(queries=q, sp=sp, attr=at, want=sets, lo=0, hi=5, k=17)
    assert e.value.code == E_INVALID and "k must be 0" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # the parameters come first
        hix.search_batch_labelset_ranged(queries=q, sp=ph.SearchParameters(1025, 16, 2), attr=at, want=sets, lo=0, hi=5)
    assert e.value.code == E_INVALID and "number_of_candidates" in str(e.value)
    ids, d, ln = hix.search_batch_labelset_ranged(queries=np.zeros((0, 100), dtype=np.float32), sp=sp, attr=at, want=[], lo=0, hi=5)
    assert ids.shape == (0, 16)  # nq == 0: a no-op
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses a Stored query id at or past n, naming the query
        hix.search_batch_labelset_ranged(qids=np.array([1, N], dtype=np.uint64), sp=sp, attr=at, want=[[3], [4]], lo=0, hi=5)
    assert e.value.code == E_INVALID and "query 1" in str(e.value) and "out of range" in str(e.value)
