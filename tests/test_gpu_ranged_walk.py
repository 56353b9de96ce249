"""phnsw_search_batch_ranged[_device]: the graph walk restricted by a numeric range, on the search kernels' range mode.
Every comparison is on ids, distance bits, lengths, stats and statuses; none has a tolerance.

Yardsticks, named per assertion below:
  * A -- tests/filter_reference.search, the restatement of search_layers / closest_vectors over the oracle's distances,
         with the masks tests/ranged_reference.masks_of makes of the key column: masks the code under test never saw.
  * B -- search_batch_filtered with those masks as per-query bitmaps: rows, lengths and stats must be equal bit for bit.

The worlds are those of tests/test_gpu_filter.py (N = 2000, built multi-layer graphs: the smallest at which the walk's
loops turn) and, for unlisted vectors, the every-second-vector index of tests/test_gpu_filter_auto.py (N = 5000).  The
key column is constructed, not drawn: 100 rows without a value, the others carry the distinct keys 10 * rank in a random
order, the entry vector at rank 1500; the ranges are cut by rank."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from parallel_hnsw_amd._lib import check, lib

import filter_reference as fr
import ranged_reference as rr
import test_gpu_filter_auto as ta
from test_gpu_exact_filter import ring
from test_gpu_filter import COS, EMPTY, KINDS, N, dist, raw_queries, same, world
from test_gpu_i8 import bits
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

NONE = rr.ATTR_NONE
NMISSING, ENTRY_RANK = 100, 1500
NQ = 20
E_INVALID = -1


def ranks(a, b):
    """the range that holds exactly the ranks [a, b)"""
    return 10 * a, 10 * (b - 1)


# (lo, hi) in u32 keys and the rows inside, for a column of 1900 values: half, a tenth, a hundredth, 1 / 64 / 65, empty
# ones, everything with and without an upper end, a range around the entry vector
RANGES = [ranks(0, 950) + (950,), ranks(1000, 1200) + (200,), ranks(1250, 1270) + (20,), ranks(1300, 1301) + (1,),
          ranks(300, 364) + (64,), ranks(400, 465) + (65,), (5, 9, 0), (9000, 3000, 0), (NONE, NONE, 0), (0, 0xFFFFFFFE, -1),
          (0, NONE, -1), ranks(1450, 1550) + (100,)]


def column(n, entry, seed=3, members=None):
    """u32 keys [n]: NONE for NMISSING rows, 10 * rank for the others in a random order, the entry vector at ENTRY_RANK"""
    keys = np.full(n, NONE, dtype=np.uint32)
    pool = np.arange(n) if members is None else np.nonzero(members)[0]
    rest = np.random.default_rng(seed).permutation(pool[pool != entry])[NMISSING:]
    order = np.concatenate([rest[:ENTRY_RANK], [entry], rest[ENTRY_RANK:]])
    keys[order] = 10 * np.arange(len(order))
    if members is not None:  # rows the index does not hold carry values too
        out = np.nonzero(~members)[0]
        keys[out] = 10 * (np.arange(len(out)) * 7 % len(order)) + 5
    return keys


def values_of(keys):
    return (np.asarray(keys, dtype=np.uint32) ^ np.uint32(0x80000000)).view(np.int32)


def attribute(hix, keys):
    return ph.Attribute(hix, values_of(np.where(keys == NONE, 0, keys)), missing=keys == NONE)


@functools.lru_cache(maxsize=None)
def attr_of(kind, dim):
    """(the column, an Attribute over world(kind, dim)'s index); made once, changed by no test"""
    hix, _, _, g = world(kind, dim)
    keys = column(N, int(g.entry_vector()))
    keys.setflags(write=False)
    return keys, attribute(hix, keys)


def bounds(nq, shift=0):
    lo = np.array([RANGES[(i + shift) % len(RANGES)][0] for i in range(nq)], dtype=np.uint32)
    hi = np.array([RANGES[(i + shift) % len(RANGES)][1] for i in range(nq)], dtype=np.uint32)
    return lo, hi


def test_the_column_is_what_the_docstring_says():
    hix, _, _, g = world("f32", 100)
    keys, at = attr_of("f32", 100)
    assert (keys == NONE).sum() == NMISSING and keys[int(g.entry_vector())] == 10 * ENTRY_RANK
    assert at.info() == (N, N - NMISSING, 0, 10 * (N - NMISSING - 1))
    lo, hi = bounds(len(RANGES))
    want = [r[2] if r[2] >= 0 else N - NMISSING for r in RANGES]
    assert rr.masks_of(keys, lo, hi).sum(1).tolist() == want
    np.testing.assert_array_equal(at.count(values_of(lo), values_of(hi)), want)
    assert (np.diff(np.argsort(keys, kind="stable")[:N - NMISSING]) < 0).sum() > 500  # span order is not id order


def device_walk(hix, at, sp, lo, hi, queries=None, qids=None, exclude=None, strict=False, upto=0, stream=0):
    """phnsw_search_batch_ranged_device with torch buffers -> ids u64, d, len u64, stats u64, status; 64 guard words
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
    lod = up(np.asarray(lo, dtype=np.uint32), np.int32).data_ptr()
    hid = up(np.asarray(hi, dtype=np.uint32), np.int32).data_ptr()
    G = 64
    ids = torch.full((nq * ef + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * ef + G,), -1.0, dtype=torch.float32, device=dev)
    ln, status = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(2))
    st = torch.full((2 * nq + G,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    hix.search_batch_ranged_device(at, nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd,
                                   ldq=ld, qids=qi, exclude=ex, lo=lod, hi=hid, strict=strict, out_stats=st.data_ptr(), upto=upto,
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
def test_the_range_walk_equals_the_restatement_and_the_bitmap_walk(kind, dim):
    hix, oix, layers, g = world(kind, dim)
    keys, at = attr_of(kind, dim)
    spt = (64, 24, 2)
    sp = ph.SearchParameters(*spt)
    lo, hi = bounds(NQ)
    vlo, vhi = values_of(lo), values_of(hi)
    masks = rr.masks_of(keys, lo, hi)
    q = raw_queries(kind, dim, NQ)
    qids = np.arange(11, N, N // NQ, dtype=np.uint64)[:NQ]
    # exclude: a vector inside the range where there is one (it matters), else any id
    ex = np.array([np.nonzero(masks[i])[0][i % 3 % max(int(masks[i].sum()), 1)] if masks[i].any() else i for i in range(NQ)],
                  dtype=np.uint64)
    seen_entry = False
    for kw in (dict(queries=q), dict(qids=qids)):
        D = None if oix is None else dist(oix, **kw)
        for upto in (0, 1, 2):
            for e in (None, ex):
                got = hix.search_batch_ranged(sp=sp, attr=at, lo=vlo, hi=vhi, exclude=e, upto=upto, stats=True, **kw)
                same(got, hix.search_batch_filtered(sp=sp, allow=masks, exclude=e, upto=upto, stats=True, **kw))       # B
                strict = hix.search_batch_ranged(sp=sp, attr=at, lo=vlo, hi=vhi, strict=True, exclude=e, upto=upto, stats=True, **kw)
                same(strict, hix.search_batch_filtered(sp=sp, allow=masks, strict=True, exclude=e, upto=upto, stats=True, **kw))  # B
                if oix is not None:
                    ref = fr.search(oix, D, spt, allow=masks, exclude=e, upto=upto, layers=layers)
                    same(got, ref)                                                                                     # A
                    same(strict, fr.strict(ref, masks), stats=False)                                                   # A
                    np.testing.assert_array_equal(strict[3], ref[3])  # strict drops ids after the walk: the same stats
                seen_entry |= bool(((got[0] == g.entry_vector()) & ~masks[:, int(g.entry_vector())][:, None]).any())
        cut = hix.search_batch_ranged(sp=sp, attr=at, lo=vlo, hi=vhi, exclude=ex, k=5, **kw)                           # the k cut
        same(cut, hix.search_batch_filtered(sp=sp, allow=masks, exclude=ex, k=5, **kw))
        dv = device_walk(hix, at, sp, lo, hi, exclude=ex, **kw)
        assert not dv[4].any()
        same(dv, hix.search_batch_ranged(sp=sp, attr=at, lo=vlo, hi=vhi, exclude=ex, stats=True, **kw))
    # the entry vector is outside most ranges: returned to their queries all the same, unless strict (asserted by B and A)
    assert seen_entry


# ---------------------------------------------------------------- 2: every queue capacity class
@pytest.mark.parametrize("ef", [64, 128, 256, 512])
def test_queue_capacity_classes(monkeypatch, ef):
    hix, oix, layers, _ = world("f32", 100)
    keys, at = attr_of("f32", 100)
    q = raw_queries("f32", 100, 12)
    lo, hi = bounds(12, shift=ef // 64)
    vlo, vhi = values_of(lo), values_of(hi)
    masks = rr.masks_of(keys, lo, hi)
    sp = ph.SearchParameters(ef, ef, 2)
    ref = hix.search_batch_filtered(queries=q, sp=sp, allow=masks, stats=True)                                        # B
    same(hix.search_batch_ranged(queries=q, sp=sp, attr=at, lo=vlo, hi=vhi, stats=True), ref)
    with env(monkeypatch, PHNSW_NO_LAT="1", PHNSW_NO_TINY="1"):  # the throughput kernel of pick_kernel_rows, rows gathered per hop
        same(hix.search_batch_ranged(queries=q, sp=sp, attr=at, lo=vlo, hi=vhi, stats=True), ref)
        same(hix.search_batch_ranged(queries=q, sp=sp, attr=at, lo=vlo, hi=vhi, strict=True, stats=True),
             hix.search_batch_filtered(queries=q, sp=sp, allow=masks, strict=True, stats=True))


# ---------------------------------------------------------------- 3: independence of the schedule
@pytest.mark.parametrize("kind,dim", [("f32", 100), ("i8q", 128)])
def test_ranged_results_do_not_depend_on_the_schedule(monkeypatch, kind, dim):
    hix, oix, layers, _ = world(kind, dim)
    keys, at = attr_of(kind, dim)
    spt = (64, 24, 2)
    sp = ph.SearchParameters(*spt)
    nq = 2100  # past the batch sizes of the small-batch kernels and of the dense-only launch of a split descent
    qids = (np.arange(nq, dtype=np.uint64) * 7) % N
    lo, hi = bounds(nq)
    vlo, vhi = values_of(lo), values_of(hi)
    masks = rr.masks_of(keys, lo, hi)
    ex = (qids + 1) % N
    base = hix.search_batch_ranged(qids=qids, sp=sp, attr=at, lo=vlo, hi=vhi, exclude=ex, stats=True)
    same(base, hix.search_batch_filtered(qids=qids, sp=sp, allow=masks, exclude=ex, stats=True))                      # B
    base_strict = hix.search_batch_ranged(qids=qids, sp=sp, attr=at, lo=vlo, hi=vhi, exclude=ex, strict=True, stats=True)
    same(base_strict, hix.search_batch_filtered(qids=qids, sp=sp, allow=masks, exclude=ex, strict=True, stats=True))  # B
    small = hix.search_batch_ranged(qids=qids[:300], sp=sp, attr=at, lo=vlo[:300], hi=vhi[:300], exclude=ex[:300], stats=True)
    same(small, tuple(x[:300] for x in base))  # a small batch: the latency kernels on f32
    split = dict(PHNSW_TWO_LAUNCH_MIN="1", PHNSW_SPLIT_BYTES="1")
    settings = [dict(PHNSW_NO_TINY="1"), dict(PHNSW_NO_LAT="1"),
                dict(PHNSW_TINY_TABLE_BYTES=str(300 * 4 * N)),  # the table holds ~300 queries: chunks of the list
                dict(split, PHNSW_TINY_MAX="200"), dict(split, PHNSW_NO_TINY="1")]
    for kv in settings:
        with env(monkeypatch, **kv):
            same(hix.search_batch_ranged(qids=qids, sp=sp, attr=at, lo=vlo, hi=vhi, exclude=ex, stats=True), base)
            if "PHNSW_TINY_TABLE_BYTES" in kv:  # the bounds followed the chunks of the list
                assert lib().phnsw_debug_last_search_chunks(hix._h) > 1
            same(hix.search_batch_ranged(qids=qids, sp=sp, attr=at, lo=vlo, hi=vhi, exclude=ex, strict=True, stats=True), base_strict)


# ---------------------------------------------------------------- 4: unlisted vectors, a non-identity vec2node
def test_an_index_over_every_second_vector():
    w = ta.world("f32", 24, 2)
    hix, n = w["hix"], ta.N
    keys = column(n, int(w["entry"]), seed=5, members=w["members"])  # odd rows carry values too: unlisted
    at = attribute(hix, keys)
    assert at.listed == int((keys[w["members"]] != NONE).sum()) < int((keys != NONE).sum())
    lo, hi = bounds(ta.NQ)
    vlo, vhi = values_of(lo), values_of(hi)
    listed = rr.masks_of(keys, lo, hi, w["members"])
    assert (rr.masks_of(keys, lo, hi).sum(1) > listed.sum(1)).any()
    sp = ph.SearchParameters(64, 24, 2)
    for kw in (dict(queries=w["q"]), dict(qids=w["qids"])):
        for strict in (False, True):
            got = hix.search_batch_ranged(sp=sp, attr=at, lo=vlo, hi=vhi, strict=strict, stats=True, **kw)
            same(got, hix.search_batch_filtered(sp=sp, allow=listed, strict=strict, stats=True, **kw))                # B
        ids = got[0][got[0] != EMPTY].astype(np.int64)
        assert len(ids) and not (ids % 2).any()  # strict: listed vectors only


# ---------------------------------------------------------------- 5: empty ranges
def test_empty_ranges_give_the_rows_of_an_all_zero_bitmap():
    hix, oix, layers, g = world("f32", 100)
    keys, at = attr_of("f32", 100)
    sp = ph.SearchParameters(64, 64, 2)
    q = raw_queries("f32", 100, NQ)
    zero = np.zeros((NQ, N), dtype=bool)
    for lo, hi in ((5, 9), (9000, 3000), (NONE, NONE), (NONE, 0)):
        lo, hi = np.full(NQ, lo, dtype=np.uint32), np.full(NQ, hi, dtype=np.uint32)
        for strict in (False, True):
            got = hix.search_batch_ranged(queries=q, sp=sp, attr=at, lo=values_of(lo), hi=values_of(hi), strict=strict, stats=True)
            same(got, hix.search_batch_filtered(queries=q, sp=sp, allow=zero, strict=strict, stats=True))             # B
            if strict:
                assert not got[2].any() and (got[0] == EMPTY).all() and (bits(got[1]) == bits(fr.FMAX)).all()
            else:  # the entry vector enters before any filter runs
                assert ((got[0] == g.entry_vector()).sum(axis=1) == got[2]).all()
        dv = device_walk(hix, at, sp, lo, hi, queries=q, strict=True)
        assert not dv[4].any() and not dv[2].any() and (dv[0] == EMPTY).all()


# ---------------------------------------------------------------- 6: the device form on a stream of its own
def test_device_form_on_a_side_stream():
    import torch
    hix = world("f32", 100)[0]
    keys, at = attr_of("f32", 100)
    sp = ph.SearchParameters(128, 32, 2)
    qids = (np.arange(70, dtype=np.uint64) * 29 + 3) % N
    lo, hi = bounds(70, shift=3)
    ex = (qids + 2) % N
    stream = torch.cuda.Stream()
    for strict in (False, True):
        host = hix.search_batch_ranged(qids=qids, sp=sp, attr=at, lo=values_of(lo), hi=values_of(hi), exclude=ex, strict=strict,
                                       stats=True)
        dv = device_walk(hix, at, sp, lo, hi, qids=qids, exclude=ex, strict=strict, stream=stream.cuda_stream)
        assert set(dv[4].tolist()) == {0}
        same(dv, host)
    one = device_walk(hix, at, sp, lo[:40], hi[:40], qids=qids[:40], upto=1, stream=stream.cuda_stream)
    same(one, hix.search_batch_filtered(qids=qids[:40], sp=sp, allow=rr.masks_of(keys, lo[:40], hi[:40]), upto=1, stats=True))  # B


# ---------------------------------------------------------------- 7: argument checks
def test_argument_checks():
    hix = world("f32", 100)[0]
    keys, at = attr_of("f32", 100)
    sp = ph.SearchParameters(16, 16, 2)
    q = raw_queries("f32", 100, 4)
    other = ph.Hnsw.from_layers(hix.store, ring(np.arange(N)))  # a handle of another index over the same store
    for call in (lambda: other.search_batch_ranged(queries=q, sp=sp, attr=at, lo=0, hi=5),
                 lambda: other.search_batch_ranged_device(at, 4, sp, 8, 8, 8, 8, qids=8, lo=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == E_INVALID and "are stale" in str(e.value) and "another index" in str(e.value)
        assert "phnsw_search_batch_ranged" in str(e.value)
    for bad in (dict(qids=8), dict(qids=8, lo=8), dict(queries=16, ldq=hix.store.ld, qids=8, lo=8, hi=8), dict(lo=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_batch_ranged_device(at, 4, sp, 8, 8, 8, 8, **bad)
        assert e.value.code == E_INVALID and "phnsw_search_batch_ranged_device: invalid argument" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # a null hi reaches the host form only past the wrapper
        check(lib().phnsw_search_batch_ranged(hix._h, at._h, q.ctypes.data_as(C.c_void_p), None, 4, C.byref(sp), 0, None,
                                              C.c_void_p(8), None, 0, 0, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None))
    assert "phnsw_search_batch_ranged: invalid argument" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # k past the queue
        hix.search_batch_ranged(queries=q, sp=sp, attr=at, lo=0, hi=5, k=17)
    assert e.value.code == E_INVALID and "k must be 0" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # the parameters come first
        hix.search_batch_ranged(queries=q, sp=ph.SearchParameters(1025, 16, 2), attr=at, lo=0, hi=5)
    assert e.value.code == E_INVALID and "number_of_candidates" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # an unknown flag
        check(lib().phnsw_search_batch_ranged(hix._h, at._h, q.ctypes.data_as(C.c_void_p), None, 4, C.byref(sp), 0, None,
                                              C.c_void_p(8), C.c_void_p(8), 2, 0, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None))
    assert "unknown flag bits" in str(e.value)
    ids, d, ln = hix.search_batch_ranged(queries=np.zeros((0, 100), dtype=np.float32), sp=sp, attr=at, lo=0, hi=5)
    assert ids.shape == (0, 16)  # nq == 0: a no-op
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses a Stored query id at or past n
        hix.search_batch_ranged(qids=np.array([N], dtype=np.uint64), sp=sp, attr=at, lo=0, hi=5)
    assert e.value.code == E_INVALID and "out of range" in str(e.value)
