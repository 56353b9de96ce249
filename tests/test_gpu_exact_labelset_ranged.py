"""The exact top-k by a SET of row labels AND a numeric range (phnsw_label_attr_count_set_device,
phnsw_search_exact_labelset_ranged[_device], filter_label_ranged.hip): one span of the column sorted by
(label << 32) | key per wanted label instead of a bitmap per query.  Every comparison is on ids, distance bits, lengths
and statuses, no tolerance anywhere.

The yardstick is the EXISTING scan, search_exact_filtered, over the per-query bitmaps
tests/labelset_ranged_reference.masks_of makes of the two columns and the sets -- masks the code under test never saw.

The worlds are those of tests/test_gpu_filter.py (N = 2000, built multi-layer graphs) and the every-second-vector index of
tests/test_gpu_filter_auto.py (N = 5000).  The key column is that of tests/test_gpu_ranged_walk.py: 100 rows without a
value, the others carry the distinct keys 10 * rank in a random order, the entry vector at rank 1500; the 12 ranges are
that test's.  The label column deals SEVEN labels over the ranks (rank r carries LABELS[r % 7], so the entry vector
carries 4): 0, 3, 4, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE -- the neighbours 3 | 4 and 0x7FFFFFFF | 0x80000000
put a span without an upper end directly against the next label's first row and the composite's top bit on a label
boundary -- except that every 37th id carries no label.  The sets go round with period 11 (SETS below), the ranges with
period 12: 132 queries meet every (set, range) combination.  The sets of all seven labels hold about 1850 rows under an
open range, more than the 1024 entries a row can have: k = 1024 is the largest k there is, and above every other count."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import labelset_ranged_reference as sr
import test_gpu_filter_auto as ta
from test_gpu_exact_filter import ring
from test_gpu_filter import EMPTY, N, raw_queries, same
from test_gpu_filter import world as filter_world
from test_gpu_i8 import adopt, bits
from test_gpu_i8q import env
from test_gpu_ranged_walk import ENTRY_RANK, RANGES, column, values_of

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
FMAX_BITS = 0x7F7FFFFF
LABELS = (0, 3, 4, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE)
LONG = [int(x) for x in np.random.default_rng(70).permutation(np.repeat(np.array(LABELS, dtype=np.int64), 10))]
SETS = [[], [3], [3, 4], [4, 3], [3, 3, 4], [NONE], [NONE, 0x80000000], [5], [0, 0xFFFFFFFE], list(LABELS), LONG]
NQ = len(SETS) * len(RANGES)  # 132
KINDS = [("f32", 24), ("f16", 24), ("i8", 24), ("i8q", 24), ("pq", 24), ("f32", 100), ("f32", 768)]
E_INVALID = -1


@functools.lru_cache(maxsize=None)
def world(kind, dim):
    """test_gpu_filter.world; a PQ store over 24 dimensions cannot have that world's dim / 4 = 6 sub-spaces (a multiple of
    4 is needed), so it gets 12 of them over the f32 world's rows, with the f32 world's graph adopted"""
    if (kind, dim) != ("pq", 24):
        return filter_world(kind, dim)
    g = filter_world("f32", 24)[3]
    return adopt(ph.PqStore(g.store, 12), g), None, None, g


def label_column(keys, entry):
    """u32 labels [n]: LABELS[rank % 7] by the rank of the key (rows without a value: by id), NONE for every 37th id but
    the entry vector"""
    n = len(keys)
    labels = np.array([LABELS[(int(k) // 10) % 7] if k != NONE else LABELS[v % 7] for v, k in enumerate(keys)], dtype=np.uint32)
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


def batch(nq=NQ, shift=0):
    """(sets, lo, hi): query i wants SETS[(i + shift) % 11] inside RANGES[(i + shift) % 12]"""
    sets = [SETS[(i + shift) % len(SETS)] for i in range(nq)]
    lo = np.array([RANGES[(i + shift) % len(RANGES)][0] for i in range(nq)], dtype=np.uint32)
    hi = np.array([RANGES[(i + shift) % len(RANGES)][1] for i in range(nq)], dtype=np.uint32)
    return sets, lo, hi


def csr(sets):
    first = np.zeros(len(sets) + 1, dtype=np.uint32)
    first[1:] = np.cumsum([len(s) for s in sets])
    values = np.array([x for s in sets for x in s], dtype=np.uint64).astype(np.uint32)
    return first, values


def stored_ids(nq):
    return (np.arange(nq, dtype=np.uint64) * 13 + 11) % N


def test_the_columns_and_the_sets_are_what_the_docstring_says():
    hix, _, _, g = world("f32", 100)
    labels, keys, at = attr_of("f32", 100)
    entry = int(g.entry_vector())
    assert keys[entry] == 10 * ENTRY_RANK and labels[entry] == LABELS[ENTRY_RANK % 7] == 4
    listed = (labels != NONE) & (keys != NONE)
    per_label = [int((listed & (labels == x)).sum()) for x in LABELS]
    assert ((labels == NONE) & (keys != NONE)).sum() > 30 and ((labels != NONE) & (keys == NONE)).sum() > 60
    assert at.info() == (N, listed.sum(), 7, max(per_label)) and min(per_label) > 200
    assert len(LONG) == 70 > 64 and sorted(set(LONG)) == sorted(LABELS) and NQ == 132
    sets, lo, hi = batch()
    assert len({(tuple(s), int(a), int(b)) for s, a, b in zip(sets, lo, hi)}) == NQ  # every (set, range) combination
    m = sr.masks_of(labels, keys, sets, lo, hi)
    counts = at.count_sets(sets, values_of(lo), values_of(hi))
    np.testing.assert_array_equal(counts, m.sum(1))
    np.testing.assert_array_equal(counts, hix.filter_count(m))
    i10 = [i for i in range(NQ) if sets[i] is SETS[9]]
    i11 = [i for i in range(NQ) if sets[i] is SETS[10]]
    by_range = lambda idx: {(int(lo[i]), int(hi[i])): int(counts[i]) for i in idx}
    assert by_range(i10) == by_range(i11) and max(by_range(i10).values()) == listed.sum() > 1024
    # a (first, values) pair is taken as the list of sequences is
    np.testing.assert_array_equal(at.count_sets(csr(sets), values_of(lo), values_of(hi)), counts)
    # the entry vector: its label and its range are both hit by some queries, one of them by others, neither by the rest
    has_label = np.array([4 in s for s in sets])
    in_range = (lo <= keys[entry]) & (keys[entry] <= hi)
    np.testing.assert_array_equal(m[:, entry], has_label & in_range)
    for a in (has_label & in_range, has_label & ~in_range, ~has_label & in_range, ~has_label & ~in_range):
        assert a.any()
    # NONE in a set, labels nobody carries, empty sets and empty ranges hold nothing; no upper end stays inside the labels
    assert not m[np.array([s in ([], [NONE], [5]) for s in sets])].any() and not m[lo > hi].any()
    open_34 = [i for i in range(NQ) if sets[i] == [3, 4] and hi[i] == NONE and lo[i] == 0]
    assert len(open_34) == 1 and set(labels[m[open_34[0]]].tolist()) == {3, 4} and counts[open_34[0]] == per_label[1] + per_label[2]
    seven = [i for i in range(NQ) if sets[i] == [NONE, 0x80000000] and hi[i] == NONE and lo[i] == 0]
    assert set(labels[m[seven[0]]].tolist()) == {0x80000000}


def device_exact(hix, at, k, first, values, lo, hi, queries=None, qids=None, exclude=None, nwant=None, stream=0):
    """phnsw_search_exact_labelset_ranged_device with torch buffers -> ids u64, d, len u64, status; 64 guard words behind
    every output must come back as they went in"""
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
    fd, lod, hid = (up(np.asarray(x, dtype=np.uint32), np.int32).data_ptr() for x in (first, lo, hi))
    vd = up(np.asarray(values, dtype=np.uint32), np.int32).data_ptr() if len(values) else 0
    G = 64
    ids = torch.full((nq * k + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * k + G,), -1.0, dtype=torch.float32, device=dev)
    ln, status = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    hix.search_exact_labelset_ranged_device(at, nq, len(values) if nwant is None else nwant, k, ids.data_ptr(), d.data_ptr(),
                                            ln.data_ptr(), status.data_ptr(), queries=qd, ldq=ld, qids=qi, exclude=ex,
                                            want_first=fd, want_values=vd, lo=lod, hi=hid, stream=stream)
    torch.cuda.synchronize()
    assert (ids[nq * k:] == 7).all() and (d[nq * k:] == -1.0).all() and (ln[nq:] == -1).all() and (status[nq:] == -1).all()
    i64 = ids[:nq * k].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, k)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return (i64, d[:nq * k].cpu().numpy().reshape(nq, k), ln[:nq].cpu().numpy().view(np.uint32).astype(np.uint64),
            status[:nq].cpu().numpy())


def check(hix, cols, at, sets, lo, hi, queries=None, qids=None, exclude=None, k=10, members=None, device=False):
    """the host form (and the device form) against search_exact_filtered over the masks -> the host result"""
    masks = sr.masks_of(cols[0], cols[1], sets, lo, hi, members)
    kw = dict(queries=queries) if queries is not None else dict(qids=qids)
    got = hix.search_exact_labelset_ranged(attr=at, want=sets, lo=values_of(lo), hi=values_of(hi), exclude=exclude, k=k, **kw)
    same(got, hix.search_exact_filtered(allow=masks, exclude=exclude, k=k, **kw))
    pad = np.arange(k)[None, :] >= got[2][:, None]
    assert (got[0][pad] == EMPTY).all() and (bits(got[1])[pad] == FMAX_BITS).all()
    if device:
        dv = device_exact(hix, at, k, *csr(sets), lo, hi, exclude=exclude, **kw)
        assert not dv[3].any()
        same(dv, got)
    return got


# ---------------------------------------------------------------- 1: kinds x dimensions, k, exclude
@pytest.mark.parametrize("kind,dim", KINDS)
def test_rows_equal_the_bitmap_scan(kind, dim):
    hix = world(kind, dim)[0]
    labels, keys, at = attr_of(kind, dim)
    sets, lo, hi = batch()
    counts = sr.masks_of(labels, keys, sets, lo, hi).sum(1)
    for kw in (dict(queries=raw_queries(kind, dim, NQ)), dict(qids=stored_ids(NQ))):
        first = check(hix, (labels, keys), at, sets, lo, hi, k=10, device=True, **kw)
        np.testing.assert_array_equal(first[2], np.minimum(counts, 10))
        check(hix, (labels, keys), at, sets, lo, hi, k=1, **kw)
        # exclude: each query's best hit where it has one -- inside its spans, it matters --, else any id
        ex = np.where(first[0][:, 0] == EMPTY, np.uint64(5), first[0][:, 0])
        got = check(hix, (labels, keys), at, sets, lo, hi, exclude=ex, k=64, device=True, **kw)
        has = first[0][:, 0] != EMPTY
        assert has.any() and not (got[0][has] == ex[has, None]).any()
        np.testing.assert_array_equal(got[2][has], np.minimum(64, counts[has] - 1))
        big = check(hix, (labels, keys), at, sets, lo, hi, k=1024, **kw)  # the whole spans of every query but the widest
        np.testing.assert_array_equal(big[2], np.minimum(counts, 1024))
        assert (counts < 1024).sum() > 100 and (counts > 1024).any()


@functools.lru_cache(maxsize=None)
def metric_world(metric):
    """an f32 store of the rows of world("f32", 24) under another metric, with a one-layer ring over every vector"""
    rows = oracle.synth_rows(0, N, 24)[:, :24].copy()
    store = ph.VectorStore(rows, metric=metric)
    hix = ph.Hnsw.from_layers(store, ring(np.arange(N)))
    keys = column(N, 0)
    labels = label_column(keys, 0)
    return hix, labels, keys, labeled_attribute(hix, labels, keys)


@pytest.mark.parametrize("metric", [oracle.METRIC_COSINE_HALF, oracle.METRIC_L2, oracle.METRIC_ONE_MINUS_DOT])
def test_three_metrics_on_f32(metric):
    hix, labels, keys, at = metric_world(metric)
    sets, lo, hi = batch()
    check(hix, (labels, keys), at, sets, lo, hi, queries=raw_queries("f32", 24, NQ), k=100, device=True)
    check(hix, (labels, keys), at, sets, lo, hi, qids=stored_ids(NQ), exclude=stored_ids(NQ), k=100)


# ---------------------------------------------------------------- 2: slices, the order of the batch and of a set
def test_rows_do_not_depend_on_the_slices(monkeypatch):
    hix = world("f32", 100)[0]
    labels, keys, at = attr_of("f32", 100)
    sets, lo, hi = batch()
    q = raw_queries("f32", 100, NQ)
    base = check(hix, (labels, keys), at, sets, lo, hi, queries=q, k=100)
    for slices in ("1", "2", "5"):
        with env(monkeypatch, PHNSW_LABELSET_RANGE_SLICES=slices):
            same(hix.search_exact_labelset_ranged(queries=q, attr=at, want=sets, lo=values_of(lo), hi=values_of(hi), k=100), base)
            dv = device_exact(hix, at, 100, *csr(sets), lo, hi, queries=q)
        assert not dv[3].any()
        same(dv, base)


def test_permuting_the_batch_permutes_the_rows_and_the_order_inside_a_set_does_not_matter():
    hix = world("f32", 100)[0]
    labels, keys, at = attr_of("f32", 100)
    sets, lo, hi = batch()
    q = raw_queries("f32", 100, NQ)
    a = dict(attr=at, k=20)
    base = hix.search_exact_labelset_ranged(queries=q, want=sets, lo=values_of(lo), hi=values_of(hi), **a)
    perm = np.random.default_rng(11).permutation(NQ)
    got = hix.search_exact_labelset_ranged(queries=q[perm], want=[sets[i] for i in perm], lo=values_of(lo[perm]),
                                           hi=values_of(hi[perm]), **a)
    same(got, tuple(x[perm] for x in base))
    rev = [list(reversed(s)) for s in sets]
    same(hix.search_exact_labelset_ranged(queries=q, want=rev, lo=values_of(lo), hi=values_of(hi), **a), base)
    srt = [sorted(s) for s in sets]
    same(hix.search_exact_labelset_ranged(queries=q, want=srt, lo=values_of(lo), hi=values_of(hi), **a), base)


def test_one_label_sets_equal_the_label_range_scan():
    hix = world("f32", 100)[0]
    labels, keys, at = attr_of("f32", 100)
    nq = 7 * len(RANGES) + 12
    want = np.array([(LABELS + (NONE, 5))[i % 9] for i in range(nq)], dtype=np.uint32)
    lo = np.array([RANGES[i % len(RANGES)][0] for i in range(nq)], dtype=np.uint32)
    hi = np.array([RANGES[i % len(RANGES)][1] for i in range(nq)], dtype=np.uint32)
    q = raw_queries("f32", 100, NQ)[:nq]
    ex = stored_ids(nq)
    for k in (1, 10, 300):
        same(hix.search_exact_labelset_ranged(queries=q, attr=at, want=[[int(w)] for w in want], lo=values_of(lo), hi=values_of(hi),
                                              exclude=ex, k=k),
             hix.search_exact_label_ranged(queries=q, attr=at, want=want, lo=values_of(lo), hi=values_of(hi), exclude=ex, k=k))


# ---------------------------------------------------------------- 3: an index over part of its store
def test_an_index_over_every_second_vector():
    w = ta.world("f32", 24, 2)
    hix = w["hix"]
    keys = column(ta.N, int(w["entry"]), seed=5, members=w["members"])  # odd rows carry labels and values too: unlisted
    labels = label_column(keys, int(w["entry"]))
    at = labeled_attribute(hix, labels, keys)
    carried = (labels != NONE) & (keys != NONE)
    assert at.listed == int(carried[w["members"]].sum()) < int(carried.sum())
    sets, lo, hi = batch(ta.NQ, shift=1)
    listed = sr.masks_of(labels, keys, sets, lo, hi, w["members"])
    assert (sr.masks_of(labels, keys, sets, lo, hi).sum(1) > listed.sum(1)).any()
    np.testing.assert_array_equal(at.count_sets(sets, values_of(lo), values_of(hi)), listed.sum(1))
    for kw in (dict(queries=w["q"]), dict(qids=w["qids"])):
        got = check(hix, (labels, keys), at, sets, lo, hi, k=100, members=w["members"], device=True, **kw)
        ids = got[0][got[0] != EMPTY].astype(np.int64)
        assert len(ids) and not (ids % 2).any()


# ---------------------------------------------------------------- 4: more work items than a resident grid holds
def test_more_work_items_than_a_grid_of_resident_waves(monkeypatch):
    """600 queries x the set of all seven labels x 5 forced slices = 21 000 (pair, slice) items of one wave each, more than
    the 256 CUs x 32 waves the part holds resident: the scan kernel's stride over what is left runs"""
    hix = world("f32", 24)[0]
    labels, keys, at = attr_of("f32", 24)
    nq = 600
    sets = [SETS[9]] * nq
    lo = np.array([RANGES[i % len(RANGES)][0] for i in range(nq)], dtype=np.uint32)
    hi = np.array([RANGES[i % len(RANGES)][1] for i in range(nq)], dtype=np.uint32)
    assert nq * len(SETS[9]) * 5 == 21000 > 256 * 32
    qids = (np.arange(nq, dtype=np.uint64) * 3 + 1) % N
    with env(monkeypatch, PHNSW_LABELSET_RANGE_SLICES="5"):
        check(hix, (labels, keys), at, sets, lo, hi, qids=qids, exclude=qids, k=10, device=True)


# ---------------------------------------------------------------- 5: the device form
def test_device_form_on_a_side_stream_with_offsets_it_cannot_trust(monkeypatch):
    import torch
    hix = world("f32", 100)[0]
    labels, keys, at = attr_of("f32", 100)
    stream = torch.cuda.Stream()
    sets, lo, hi = batch(70, shift=4)
    qids = stored_ids(70)
    host = hix.search_exact_labelset_ranged(qids=qids, attr=at, want=sets, lo=values_of(lo), hi=values_of(hi), exclude=qids, k=33)
    dv = device_exact(hix, at, 33, *csr(sets), lo, hi, qids=qids, exclude=qids, stream=stream.cuda_stream)
    assert set(dv[3].tolist()) == {0}
    same(dv, host)
    # offsets: q4 runs backwards, q5 overlaps the lower q3, q6 ends past nwant, q7 starts past nwant and runs backwards; the
    # others are sound and own their ranges.  Twelve queries, an open range for all
    values = np.array((LONG + LONG)[:24], dtype=np.uint32)
    nwant = len(values)
    first = np.array([0, 3, 5, 5, 9, 7, 12, nwant + 5, 14, 17, 20, 20, nwant], dtype=np.uint32)
    refused = [4, 5, 6, 7]
    sound = [q for q in range(12) if q not in refused]
    sets12 = [values[first[q]:first[q + 1]].tolist() if q in sound else [] for q in range(12)]
    lo12, hi12 = np.array([RANGES[q][0] for q in range(12)], dtype=np.uint32), np.array([RANGES[q][1] for q in range(12)], dtype=np.uint32)
    lo12[[3, 5]], hi12[[3, 5]] = 0, NONE  # the two that overlap have candidates
    q = raw_queries("f32", 100, NQ)[:12]
    ref = hix.search_exact_filtered(queries=q, allow=sr.masks_of(labels, keys, sets12, lo12, hi12), k=10)
    assert ref[2][sound].any() and ref[2][3] == 10
    for kw in (dict(), dict(PHNSW_LABELSET_RANGE_SLICES="3")):
        with env(monkeypatch, **kw):
            dv = device_exact(hix, at, 10, first, values, lo12, hi12, queries=q, nwant=nwant, stream=stream.cuda_stream)
        assert (dv[3][refused] == 8).all() and not dv[3][sound].any()
        assert not dv[2][refused].any() and (dv[0][refused] == EMPTY).all() and (bits(dv[1][refused]) == FMAX_BITS).all()
        same(tuple(x[sound] for x in dv[:3]), tuple(x[sound] for x in ref))
    # the count call writes 0 exactly where the scan refuses
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev) for x in (first, values, lo12, hi12)]
    out = torch.full((12 + 64,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    at.count_set_device(12, nwant, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), out.data_ptr(),
                        stream=stream.cuda_stream)
    torch.cuda.synchronize()
    counts = out.cpu().numpy()
    assert (counts[12:] == -1).all() and not counts[refused].any()
    np.testing.assert_array_equal(counts[sound], sr.masks_of(labels, keys, sets12, lo12, hi12).sum(1)[sound])
    # a Stored id at or past n: status 4, an empty row; status 8 wins where both hold; the others are unaffected
    bad = stored_ids(12)
    bad[[1, 5, 11]] = [N, N + 3, 0xFFFFFFF0]
    ref = hix.search_exact_filtered(qids=stored_ids(12), allow=sr.masks_of(labels, keys, sets12, lo12, hi12), k=10)
    dv = device_exact(hix, at, 10, first, values, lo12, hi12, qids=bad, nwant=nwant)
    assert dv[3].tolist() == [0, 4, 0, 0, 8, 8, 8, 8, 0, 0, 0, 4]
    empty = [1, 4, 5, 6, 7, 11]
    assert not dv[2][empty].any() and (dv[0][empty] == EMPTY).all() and (bits(dv[1][empty]) == FMAX_BITS).all()
    good = [0, 2, 3, 8, 9, 10]
    same(tuple(x[good] for x in dv[:3]), tuple(x[good] for x in ref))


# ---------------------------------------------------------------- 6: refusals
def test_argument_checks_in_the_documented_order():
    import ctypes as C
    hix = world("f32", 100)[0]
    labels, keys, at = attr_of("f32", 100)
    q = raw_queries("f32", 100, NQ)[:4]
    sets = [[3], [3, 4], [], [5]]
    other = ph.Hnsw.from_layers(hix.store, ring(np.arange(N)))  # a handle of another index over the same store
    for k in (0, 1025):  # k comes before the handle
        with pytest.raises(ph.PhnswError) as e:
            other.search_exact_labelset_ranged(queries=q, attr=at, want=sets, lo=0, hi=5, k=k)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_labelset_ranged: k must be 1..1024 (got %d)" % k
        with pytest.raises(ph.PhnswError) as e:
            other.search_exact_labelset_ranged_device(at, 4, 4, k, 8, 8, 8, 8, qids=8, want_first=8, want_values=8, lo=8, hi=8)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_labelset_ranged_device: k must be 1..1024 (got %d)" % k
    for call in (lambda: other.search_exact_labelset_ranged(queries=q, attr=at, want=sets, lo=0, hi=5, k=3),
                 lambda: other.search_exact_labelset_ranged_device(at, 4, 4, 3, 8, 8, 8, 8)):  # the handle before the pointers
        with pytest.raises(ph.PhnswError) as e:
            call()
        msg = str(e.value)
        assert e.value.code == E_INVALID and "are stale: made for another index" in msg and "phnsw_search_exact_labelset_ranged" in msg
    for bad in (dict(queries=16, ldq=hix.store.ld, qids=8, want_first=8, want_values=8, lo=8, hi=8), dict(want_first=8, want_values=8, lo=8, hi=8),
                dict(qids=8, want_values=8, lo=8, hi=8), dict(qids=8, want_first=8, lo=8, hi=8), dict(qids=8, want_first=8, want_values=8, hi=8),
                dict(qids=8, want_first=8, want_values=8, lo=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_labelset_ranged_device(at, 4, 4, 3, 8, 8, 8, 8, **bad)
        assert e.value.code == E_INVALID and "phnsw_search_exact_labelset_ranged_device: invalid argument" in str(e.value)
    hix.search_exact_labelset_ranged_device(at, 0, 0, 3, 0, 0, 0, 0)  # nq == 0: a no-op before any pointer is looked at
    with pytest.raises(ph.PhnswError) as e:
        hix.search_exact_labelset_ranged_device(at, 4, 2 ** 31, 3, 8, 8, 8, 8, qids=8, want_first=8, want_values=8, lo=8, hi=8)
    assert "nq and nwant must be below 2^31 - 1" in str(e.value)
    ids, d, ln = hix.search_exact_labelset_ranged(queries=np.zeros((0, 100), dtype=np.float32), attr=at, want=[], lo=0, hi=1, k=3)
    assert ids.shape == (0, 3)  # nq == 0: a no-op
    # the host form past the wrapper: null arguments, then want_values against want_first[nq], then the Stored ids, then
    # the offsets -- each names the call, the last two the query
    lib = ph.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    first, lo, hi = np.array([0, 1, 3, 3, 4], dtype=np.uint32), np.zeros(4, dtype=np.uint32), np.full(4, 50, dtype=np.uint32)
    values = np.array([3, 3, 4, 5], dtype=np.uint32)
    ids, d, ln = np.zeros((4, 3), dtype=np.uint64), np.zeros((4, 3), dtype=np.float32), np.zeros(4, dtype=np.uint64)
    qids = np.array([1, 2, N + 5, N + 6], dtype=np.uint64)
    call = lambda qq, qi, f, v, l, h: lib.phnsw_search_exact_labelset_ranged(hix._h, at._h, qq, qi, 4, None, f, v, l, h, 3, p(ids), p(d), p(ln))
    assert call(p(q), p(qids), p(first), p(values), p(lo), p(hi)) == E_INVALID and "exactly one" in lib.phnsw_last_error().decode()
    assert call(p(q), None, None, p(values), p(lo), p(hi)) == E_INVALID
    assert "phnsw_search_exact_labelset_ranged: invalid argument (outputs; want_first, lo and hi" in lib.phnsw_last_error().decode()
    assert call(None, p(qids), p(first), None, p(lo), p(hi)) == E_INVALID  # want_values comes before the Stored ids
    assert "want_values unless want_first[nq] is 0" in lib.phnsw_last_error().decode()
    back = np.array([0, 3, 1, 3, 4], dtype=np.uint32)
    assert call(None, p(qids), p(back), p(values), p(lo), p(hi)) == E_INVALID  # the Stored ids come before the offsets
    assert lib.phnsw_last_error().decode() == ("phnsw_search_exact_labelset_ranged: query 2: stored query id %d out of range" % (N + 5))
    assert call(p(q), None, p(back), p(values), p(lo), p(hi)) == E_INVALID
    assert lib.phnsw_last_error().decode().startswith("phnsw_search_exact_labelset_ranged: query 1: want_first must start at 0 and never run backwards")
    off = np.array([1, 1, 3, 3, 4], dtype=np.uint32)
    assert call(p(q), None, p(off), p(values), p(lo), p(hi)) == E_INVALID and "query 0: want_first must start at 0" in lib.phnsw_last_error().decode()
    assert call(p(q), None, p(first), p(values), p(lo), p(hi)) == 0  # sound: the keys 0 .. 50 under {3}, {3, 4}, {} and {5}
    np.testing.assert_array_equal(ln, np.minimum(sr.masks_of(labels, keys, [[3], [3, 4], [], [5]], lo, hi).sum(1), 3))
    # a null handle: PHNSW_E_INVALID, before the other arguments are looked at
    assert lib.phnsw_search_exact_labelset_ranged(hix._h, None, None, None, 4, None, None, None, None, None, 3, None, None, None) == E_INVALID
    assert "phnsw_search_exact_labelset_ranged" in lib.phnsw_last_error().decode()
    assert lib.phnsw_label_attr_count_set_device(None, None, None, None, None, 4, 0, None, None) == E_INVALID
    assert "phnsw_label_attr_count_set_device: null label and attribute keys" in lib.phnsw_last_error().decode()
    assert lib.phnsw_label_attr_count_set_device(at._h, C.c_void_p(8), None, C.c_void_p(8), C.c_void_p(8), 4, 3, C.c_void_p(8), None) == E_INVALID
    assert "null want_values with nwant > 0" in lib.phnsw_last_error().decode()


def test_a_handle_is_stale_after_the_store_has_grown():
    rows = oracle.synth_rows(0, 300, 24)[:, :24].copy()
    store = ph.VectorStore(rows[:200], metric=oracle.METRIC_COSINE_HALF)
    hix = ph.Hnsw.from_layers(store, ring(np.arange(200)))
    val = (np.arange(200) * 7 % 50).astype(np.int32) - 25
    lab = (np.arange(200) % 3).astype(np.uint32)
    at = ph.LabeledAttribute(hix, lab, val)
    sets = [[0, 1], [1], [2, 0, 2]]
    lo, hi = np.array([-25, 0, 10], dtype=np.int32), np.array([-20, 0, 24], dtype=np.int32)
    allow = np.array([np.isin(lab, s) for s in sets]) & (val[None, :] >= lo[:, None]) & (val[None, :] <= hi[:, None])
    same(hix.search_exact_labelset_ranged(queries=rows[:3], attr=at, want=sets, lo=lo, hi=hi, k=5),
         hix.search_exact_filtered(queries=rows[:3], allow=allow, k=5))
    store.append(rows[200:])
    with pytest.raises(ph.PhnswError) as e:
        hix.search_exact_labelset_ranged(queries=rows[:3], attr=at, want=sets, lo=lo, hi=hi, k=5)
    assert e.value.code == E_INVALID and "are stale: made for this index before it changed" in str(e.value)
    at2 = ph.LabeledAttribute(hix, np.concatenate([lab, np.zeros(100, dtype=np.uint32)]),
                              np.concatenate([val, np.zeros(100, dtype=np.int32)]))
    assert at2.listed == 200  # the appended vectors are not in the index, so they are not listed
    allow2 = np.concatenate([allow, np.ones((3, 100), dtype=bool)], axis=1)
    same(hix.search_exact_labelset_ranged(queries=rows[:3], attr=at2, want=sets, lo=lo, hi=hi, k=5),
         hix.search_exact_filtered(queries=rows[:3], allow=allow2, k=5))
