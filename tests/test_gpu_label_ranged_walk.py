"""phnsw_search_batch_label_ranged[_device]: the graph walk restricted by a row label and a numeric range, on the search
kernels' label-range mode.  Every comparison is on ids, distance bits, lengths, stats and statuses; none has a tolerance.

Yardsticks, named per assertion below:
  * A -- tests/filter_reference.search, the restatement of search_layers / closest_vectors over the oracle's distances,
         with the masks tests/label_ranged_reference.masks_of makes of the two columns: masks the code under test never
         saw.
  * B -- search_batch_filtered with those masks as per-query bitmaps: rows, lengths and stats must be equal bit for bit.

The worlds are those of tests/test_gpu_ranged_walk.py (N = 2000, built multi-layer graphs, and the every-second-vector
index of tests/test_gpu_filter_auto.py, N = 5000) and so is the key column: 100 rows without a value, the others carry
the distinct keys 10 * rank in a random order, the entry vector at rank 1500.  Three labels -- 3, 0x80000001 and
0xFFFFFFFE -- are dealt over the ranks (rank r carries LABELS[r % 3], so the entry vector carries 3), except that every
37th row of the id range carries no label.  The queries go round the ranges of that test (period 12) and round the
wanted labels 3, 0x80000001, 0xFFFFFFFE, 3, NONE (period 5): the entry vector's label and range are both hit by some
queries, one of them by others, neither by the rest."""
import ctypes as C
import functools

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd._lib import check, lib

import filter_reference as fr
import label_ranged_reference as lr
import test_gpu_filter_auto as ta
from test_gpu_exact_filter import ring
from test_gpu_filter import EMPTY, KINDS, N, dist, raw_queries, same, world
from test_gpu_i8 import bits
from test_gpu_i8q import env
from test_gpu_ranged_walk import ENTRY_RANK, NMISSING, RANGES, column, values_of

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
LABELS = (3, 0x80000001, 0xFFFFFFFE)
WANTS = (3, 0x80000001, 0xFFFFFFFE, 3, NONE)
NQ = 20
E_INVALID = -1


def label_column(keys, entry):
    """u32 labels [n]: LABELS[rank % 3] by the rank of the key (rows without a value: by id), NONE for every 37th id but
    the entry vector"""
    n = len(keys)
    labels = np.array([LABELS[(int(k) // 10) % 3] if k != NONE else LABELS[v % 3] for v, k in enumerate(keys)], dtype=np.uint32)
    bare = np.arange(n) % 37 == 5
    bare[entry] = False
    labels[bare] = NONE
    return labels


def labeled_attribute(hix, labels, keys):
    return ph.LabeledAttribute(hix, labels, values_of(np.where(keys == NONE, 0, keys)), missing=keys == NONE)


@functools.lru_cache(maxsize=None)
def attr_of(kind, dim):
    """(labels, keys, a LabeledAttribute over world(kind, dim)'s index); made once, changed by no test"""
    hix, _, _, g = world(kind, dim)
    keys = column(N, int(g.entry_vector()))
    labels = label_column(keys, int(g.entry_vector()))
    keys.setflags(write=False), labels.setflags(write=False)
    return labels, keys, labeled_attribute(hix, labels, keys)


def pairs(nq, shift=0):
    want = np.array([WANTS[(i + shift) % len(WANTS)] for i in range(nq)], dtype=np.uint32)
    lo = np.array([RANGES[(i + shift) % len(RANGES)][0] for i in range(nq)], dtype=np.uint32)
    hi = np.array([RANGES[(i + shift) % len(RANGES)][1] for i in range(nq)], dtype=np.uint32)
    return want, lo, hi


def test_the_columns_are_what_the_docstring_says():
    hix, _, _, g = world("f32", 100)
    labels, keys, at = attr_of("f32", 100)
    entry = int(g.entry_vector())
    assert keys[entry] == 10 * ENTRY_RANK and labels[entry] == LABELS[0]
    listed = (labels != NONE) & (keys != NONE)
    per_label = [int((listed & (labels == x)).sum()) for x in LABELS]
    assert ((labels == NONE) & (keys != NONE)).sum() > 30 and ((labels != NONE) & (keys == NONE)).sum() > 60
    assert at.info() == (N, listed.sum(), 3, max(per_label)) and min(per_label) > 500
    want, lo, hi = pairs(60)  # every (label, range) combination
    m = lr.masks_of(labels, keys, want, lo, hi)
    np.testing.assert_array_equal(at.count(want, values_of(lo), values_of(hi)), m.sum(1))
    hit = m[:, entry]
    label_only = (want == LABELS[0]) & ~hit
    assert hit.any() and label_only.any() and ((want != LABELS[0]) & (lo <= keys[entry]) & (keys[entry] <= hi)).any()
    assert hit[:NQ].any() and not hit[:NQ].all()
    assert not m[want == NONE].any() and not m[lo > hi].any() and m[(hi == NONE) & (want != NONE) & (lo == 0)].any()


def device_walk(hix, at, sp, want, lo, hi, queries=None, qids=None, exclude=None, strict=False, upto=0, stream=0):
    """phnsw_search_batch_label_ranged_device with torch buffers -> ids u64, d, len u64, stats u64, status; 64 guard
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
    wd, lod, hid = (up(np.asarray(x, dtype=np.uint32), np.int32).data_ptr() for x in (want, lo, hi))
    G = 64
    ids = torch.full((nq * ef + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * ef + G,), -1.0, dtype=torch.float32, device=dev)
    ln, status = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(2))
    st = torch.full((2 * nq + G,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    hix.search_batch_label_ranged_device(at, nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd,
                                         ldq=ld, qids=qi, exclude=ex, want=wd, lo=lod, hi=hid, strict=strict,
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
    want, lo, hi = pairs(NQ)
    vlo, vhi = values_of(lo), values_of(hi)
    masks = lr.masks_of(labels, keys, want, lo, hi)
    q = raw_queries(kind, dim, NQ)
    qids = np.arange(11, N, N // NQ, dtype=np.uint64)[:NQ]
    # exclude: a vector inside the span where there is one (it matters), else any id
    ex = np.array([np.nonzero(masks[i])[0][i % 3 % max(int(masks[i].sum()), 1)] if masks[i].any() else i for i in range(NQ)],
                  dtype=np.uint64)
    seen_entry = False
    for kw in (dict(queries=q), dict(qids=qids)):
        D = None if oix is None else dist(oix, **kw)
        for upto in (0, 1, 2):
            for e in (None, ex):
                a = dict(sp=sp, attr=at, want=want, lo=vlo, hi=vhi, exclude=e, upto=upto, stats=True, **kw)
                b = dict(sp=sp, allow=masks, exclude=e, upto=upto, stats=True, **kw)
                got = hix.search_batch_label_ranged(**a)  # k = 0: the whole queue
                same(got, hix.search_batch_filtered(**b))                                                             # B
                strict = hix.search_batch_label_ranged(strict=True, **a)
                same(strict, hix.search_batch_filtered(strict=True, **b))                                             # B
                if oix is not None:
                    ref = fr.search(oix, D, spt, allow=masks, exclude=e, upto=upto, layers=layers)
                    same(got, ref)                                                                                    # A
                    same(strict, fr.strict(ref, masks), stats=False)                                                  # A
                    np.testing.assert_array_equal(strict[3], ref[3])  # strict drops ids after the walk: the same stats
                seen_entry |= bool(((got[0] == g.entry_vector()) & ~masks[:, int(g.entry_vector())][:, None]).any())
        cut = hix.search_batch_label_ranged(sp=sp, attr=at, want=want, lo=vlo, hi=vhi, exclude=ex, k=5, **kw)         # k < ef
        same(cut, hix.search_batch_filtered(sp=sp, allow=masks, exclude=ex, k=5, **kw))
        dv = device_walk(hix, at, sp, want, lo, hi, exclude=ex, **kw)
        assert not dv[4].any()
        same(dv, hix.search_batch_label_ranged(sp=sp, attr=at, want=want, lo=vlo, hi=vhi, exclude=ex, stats=True, **kw))
    # the entry vector is outside most spans: returned to their queries all the same, unless strict (asserted by B and A)
    assert seen_entry


# ---------------------------------------------------------------- 2: independence of the schedule
def test_results_do_not_depend_on_the_schedule(monkeypatch):
    hix, oix, layers, _ = world("f32", 100)
    labels, keys, at = attr_of("f32", 100)
    sp = ph.SearchParameters(64, 24, 2)
    nq = 2100  # past the batch sizes of the small-batch kernels and of the dense-only launch of a split descent
    qids = (np.arange(nq, dtype=np.uint64) * 7) % N
    want, lo, hi = pairs(nq)
    vlo, vhi = values_of(lo), values_of(hi)
    masks = lr.masks_of(labels, keys, want, lo, hi)
    ex = (qids + 1) % N
    a = dict(qids=qids, sp=sp, attr=at, want=want, lo=vlo, hi=vhi, exclude=ex, stats=True)
    base = hix.search_batch_label_ranged(**a)
    same(base, hix.search_batch_filtered(qids=qids, sp=sp, allow=masks, exclude=ex, stats=True))                      # B
    base_strict = hix.search_batch_label_ranged(strict=True, **a)
    same(base_strict, hix.search_batch_filtered(qids=qids, sp=sp, allow=masks, exclude=ex, strict=True, stats=True))  # B
    small = hix.search_batch_label_ranged(qids=qids[:300], sp=sp, attr=at, want=want[:300], lo=vlo[:300], hi=vhi[:300],
                                          exclude=ex[:300], stats=True)
    same(small, tuple(x[:300] for x in base))  # a small batch: the latency kernels on f32
    split = dict(PHNSW_TWO_LAUNCH_MIN="1", PHNSW_SPLIT_BYTES="1")
    settings = [dict(PHNSW_NO_TINY="1"), dict(PHNSW_NO_LAT="1"),
                dict(PHNSW_TINY_TABLE_BYTES=str(300 * 4 * N)),  # the table holds ~300 queries: chunks of the list
                dict(split, PHNSW_TINY_MAX="200"), dict(split, PHNSW_NO_TINY="1")]
    for kv in settings:
        with env(monkeypatch, **kv):
            same(hix.search_batch_label_ranged(**a), base)
            if "PHNSW_TINY_TABLE_BYTES" in kv:  # the labels and the bounds followed the chunks of the list
                assert lib().phnsw_debug_last_search_chunks(hix._h) > 1
            same(hix.search_batch_label_ranged(strict=True, **a), base_strict)


# ---------------------------------------------------------------- 3: unlisted vectors, a non-identity vec2node
def test_an_index_over_every_second_vector():
    w = ta.world("f32", 24, 2)
    hix = w["hix"]
    keys = column(ta.N, int(w["entry"]), seed=5, members=w["members"])  # odd rows carry labels and values too: unlisted
    labels = label_column(keys, int(w["entry"]))
    at = labeled_attribute(hix, labels, keys)
    carried = (labels != NONE) & (keys != NONE)
    assert at.listed == int(carried[w["members"]].sum()) < int(carried.sum())
    want, lo, hi = pairs(ta.NQ)
    vlo, vhi = values_of(lo), values_of(hi)
    listed = lr.masks_of(labels, keys, want, lo, hi, w["members"])
    assert (lr.masks_of(labels, keys, want, lo, hi).sum(1) > listed.sum(1)).any()
    sp = ph.SearchParameters(64, 24, 2)
    for kw in (dict(queries=w["q"]), dict(qids=w["qids"])):
        for strict in (False, True):
            got = hix.search_batch_label_ranged(sp=sp, attr=at, want=want, lo=vlo, hi=vhi, strict=strict, stats=True, **kw)
            same(got, hix.search_batch_filtered(sp=sp, allow=listed, strict=strict, stats=True, **kw))                # B
        ids = got[0][got[0] != EMPTY].astype(np.int64)
        assert len(ids) and not (ids % 2).any()  # strict: listed vectors only


# ---------------------------------------------------------------- 4: empty spans, an open upper end
def test_empty_spans_give_the_rows_of_an_all_zero_bitmap():
    hix, oix, layers, g = world("f32", 100)
    labels, keys, at = attr_of("f32", 100)
    sp = ph.SearchParameters(64, 64, 2)
    q = raw_queries("f32", 100, NQ)
    zero = np.zeros((NQ, N), dtype=bool)
    # want == NONE with every bound, lo > hi with keys between, a gap, a label nobody carries, NONE bounds
    for w_, lo, hi in ((NONE, 0, NONE), (NONE, NONE, NONE), (3, 9000, 3000), (3, 5, 9), (4, 0, NONE), (0x80000000, 0, NONE),
                       (0xFFFFFFFD, 0, NONE), (3, NONE, NONE), (3, NONE, 0)):
        want, lo, hi = (np.full(NQ, x, dtype=np.uint32) for x in (w_, lo, hi))
        assert not lr.masks_of(labels, keys, want, lo, hi).any()
        for strict in (False, True):
            got = hix.search_batch_label_ranged(queries=q, sp=sp, attr=at, want=want, lo=values_of(lo), hi=values_of(hi),
                                                strict=strict, stats=True)
            same(got, hix.search_batch_filtered(queries=q, sp=sp, allow=zero, strict=strict, stats=True))             # B
            if strict:
                assert not got[2].any() and (got[0] == EMPTY).all() and (bits(got[1]) == bits(fr.FMAX)).all()
            else:  # the entry vector enters before any filter runs
                assert ((got[0] == g.entry_vector()).sum(axis=1) == got[2]).all()
        dv = device_walk(hix, at, sp, want, lo, hi, queries=q, strict=True)
        assert not dv[4].any() and not dv[2].any() and (dv[0] == EMPTY).all()
    for w_ in LABELS:  # hi == 0xFFFFFFFF: no upper end within the label, and nothing of the next label
        want, lo, hi = np.full(NQ, w_, dtype=np.uint32), np.full(NQ, 5000, dtype=np.uint32), np.full(NQ, NONE, dtype=np.uint32)
        m = lr.masks_of(labels, keys, want, lo, hi)
        assert m.any() and (labels[m[0]] == w_).all()
        same(hix.search_batch_label_ranged(queries=q, sp=sp, attr=at, want=want, lo=values_of(lo), hi=None, strict=True, stats=True),
             hix.search_batch_filtered(queries=q, sp=sp, allow=m, strict=True, stats=True))                           # B


# ---------------------------------------------------------------- 5: the device form on a stream of its own
def test_device_form_on_a_side_stream():
    import torch
    hix = world("f32", 100)[0]
    labels, keys, at = attr_of("f32", 100)
    sp = ph.SearchParameters(128, 32, 2)
    qids = (np.arange(70, dtype=np.uint64) * 29 + 3) % N
    want, lo, hi = pairs(70, shift=3)
    ex = (qids + 2) % N
    stream = torch.cuda.Stream()
    for strict in (False, True):
        host = hix.search_batch_label_ranged(qids=qids, sp=sp, attr=at, want=want, lo=values_of(lo), hi=values_of(hi), exclude=ex,
                                             strict=strict, stats=True)
        dv = device_walk(hix, at, sp, want, lo, hi, qids=qids, exclude=ex, strict=strict, stream=stream.cuda_stream)
        assert set(dv[4].tolist()) == {0}
        same(dv, host)
    one = device_walk(hix, at, sp, want[:40], lo[:40], hi[:40], qids=qids[:40], upto=1, stream=stream.cuda_stream)
    same(one, hix.search_batch_filtered(qids=qids[:40], sp=sp, allow=lr.masks_of(labels, keys, want[:40], lo[:40], hi[:40]), upto=1,
                                        stats=True))                                                                  # B


# ---------------------------------------------------------------- 6: argument checks
def test_argument_checks():
    hix = world("f32", 100)[0]
    labels, keys, at = attr_of("f32", 100)
    sp = ph.SearchParameters(16, 16, 2)
    q = raw_queries("f32", 100, 4)
    other = ph.Hnsw.from_layers(hix.store, ring(np.arange(N)))  # a handle of another index over the same store
    for call in (lambda: other.search_batch_label_ranged(queries=q, sp=sp, attr=at, want=3, lo=0, hi=5),
                 lambda: other.search_batch_label_ranged_device(at, 4, sp, 8, 8, 8, 8, qids=8, want=8, lo=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == E_INVALID and "are stale" in str(e.value) and "another index" in str(e.value)
        assert "phnsw_search_batch_label_ranged" in str(e.value)
    for bad in (dict(qids=8), dict(qids=8, lo=8, hi=8), dict(qids=8, want=8, lo=8), dict(queries=16, ldq=hix.store.ld, qids=8, want=8, lo=8, hi=8),
                dict(want=8, lo=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_batch_label_ranged_device(at, 4, sp, 8, 8, 8, 8, **bad)
        assert e.value.code == E_INVALID and "phnsw_search_batch_label_ranged_device: invalid argument" in str(e.value)
    qp = q.ctypes.data_as(C.c_void_p)
    with pytest.raises(ph.PhnswError) as e:  # a null want reaches the host form only past the wrapper
        check(lib().phnsw_search_batch_label_ranged(hix._h, at._h, qp, None, 4, C.byref(sp), 0, None, None, C.c_void_p(8), C.c_void_p(8),
                                                    0, 0, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None))
    assert "phnsw_search_batch_label_ranged: invalid argument" in str(e.value)
    for flags in (2, 0x80000000, 3):  # unknown flag bits, with and without the known one
        with pytest.raises(ph.PhnswError) as e:
            check(lib().phnsw_search_batch_label_ranged(hix._h, at._h, qp, None, 4, C.byref(sp), 0, None, C.c_void_p(8), C.c_void_p(8),
                                                        C.c_void_p(8), flags, 0, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None))
        assert e.value.code == E_INVALID and "unknown flag bits" in str(e.value)
        with pytest.raises(ph.PhnswError) as e:
            check(lib().phnsw_search_batch_label_ranged_device(hix._h, at._h, None, 0, C.c_void_p(8), 4, C.byref(sp), 0, None,
                                                               C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), flags, C.c_void_p(8),
                                                               C.c_void_p(8), C.c_void_p(8), None, C.c_void_p(8), None))
        assert e.value.code == E_INVALID and "unknown flag bits" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # k past the queue
        hix.search_batch_label_ranged(queries=q, sp=sp, attr=at, want=3, lo=0, hi=5, k=17)
    assert e.value.code == E_INVALID and "k must be 0" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # the parameters come first
        hix.search_batch_label_ranged(queries=q, sp=ph.SearchParameters(1025, 16, 2), attr=at, want=3, lo=0, hi=5)
    assert e.value.code == E_INVALID and "number_of_candidates" in str(e.value)
    ids, d, ln = hix.search_batch_label_ranged(queries=np.zeros((0, 100), dtype=np.float32), sp=sp, attr=at, want=3, lo=0, hi=5)
    assert ids.shape == (0, 16)  # nq == 0: a no-op
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses a Stored query id at or past n
        hix.search_batch_label_ranged(qids=np.array([N], dtype=np.uint64), sp=sp, attr=at, want=3, lo=0, hi=5)
    assert e.value.code == E_INVALID and "out of range" in str(e.value)
