"""The exact top-k by a row label AND a numeric range (phnsw_label_attr_*, phnsw_search_exact_label_ranged[_device],
filter_label_ranged.hip): one span of a column sorted once by (label << 32) | key instead of a bitmap per query.  Every
comparison is on ids, distance bits, lengths and status, no tolerance anywhere.

Two yardsticks, both for every case: tests/exact_filter_reference.py over the oracle's distances with the bitmaps
label_ranged_reference.masks_of makes of the two columns, which the code under test did not make, and the existing scan,
search_exact_filtered with those masks as per-query bitmaps, whose rows the new call promises bit for bit.

The worlds are those of tests/test_gpu_exact_ranged.py (N = 5000, 40 copies of row 0 spread over the id range, 65 raw and
65 stored queries, one-layer ring indexes, its KINDS).  The columns are constructed, not drawn; the rows take their
places in a random order, so the ids of a span are not ascending.  Four labels:

  MAIN 0x80000005  4001 rows: one with key 0; 1500 with the distinct keys 1000, 1010, ... (spans of exactly 1, 64 and 65
                   rows are cut from them); a plateau of 300 rows with ONE key, 100000; a run of 2200 rows with the
                   distinct keys 200000, 200010, ... that holds the 40 copies, 55 ranks apart (35 batches of 64: the
                   ties cross batch and slice borders)
  TWIN 7            350 rows: 300 with the keys 1000, 1010, ... 3990 -- the keys MAIN's first 300 distinct rows carry, so
                   the range alone cannot tell the two labels apart -- and 50 with the plateau's key, 100000
  TOPL 0xFFFFFFFE   200 rows: 199 with the keys 1000, 1010, ... and one with key 0xFFFFFFFE
  ZERO 0            249 rows with the keys 0, 5, 10, ...

100 rows carry the label MAIN but no value, 100 rows carry a value (1000, 1010, ...) but no label: none of them is
listed.  The values are held as int32, whose map covers all of the u32 keys a bound can be.

The spans of PAIRS, as (label, lo, hi) -> rows: (MAIN, the big run) 2200; (MAIN, 1000, 1000) 1; (MAIN, 2000, 2630) 64;
(MAIN, 2000, 2640) 65; (MAIN, plateau) 300; (TWIN, plateau) 50; (TWIN, 1000, 3990) 300; (MAIN, 1000, 3990) 300; (TWIN,
0, open) 350; (TOPL, 0, open) 200; (TOPL, 0xFFFFFFFE, open) 1; (ZERO, 0, 0) 1; (ZERO, 0, open) 249; (MAIN, 0, open)
4001; (MAIN, 5000, 2000) 0; (NONE, 0, open) 0; the labels 5, 0x80000006, 0x7FFFFFFF and 0xFFFFFFFD, which nobody
carries, 0 each; (MAIN, 5, 900) 0; (MAIN, 15990, 100000) 301; (MAIN, 100000, 200000) 301; (TOPL, 0, 0xFFFFFFFE) 200."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import label_ranged_reference as lr
from test_gpu_exact_filter import COS, DUPS, EMPTY, N, ring, same
from test_gpu_exact_labeled import world_of
from test_gpu_exact_ranged import KINDS, values_of
from test_gpu_exact_shared import NQX, fetch, sworld
from test_gpu_i8 import bits
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
TOP = 0xFFFFFFFE
MAIN, TWIN, TOPL, ZERO = 0x80000005, 7, 0xFFFFFFFE, 0
A0, PLATEAU, BIG0 = 1000, 100000, 200000
NA, NP, NBIG, NTWIN, NTWINP, NTOPL, NZERO, NHALF = 1500, 300, 2200, 300, 50, 200, 249, 100
NMAIN = 1 + NA + NP + NBIG
LISTED = NMAIN + NTWIN + NTWINP + NTOPL + NZERO


@functools.lru_cache(maxsize=None)
def columns():
    """(labels, keys) of every vector, u32 [N] each"""
    labels = np.full(N, NONE, dtype=np.uint32)
    keys = np.full(N, NONE, dtype=np.uint32)
    o = list(np.random.default_rng(2026).permutation(np.setdiff1d(np.arange(N), DUPS)))

    def take(count):
        got = np.array(o[:count], dtype=np.int64)
        del o[:count]
        return got

    def put(rows, label, k):
        labels[rows], keys[rows] = label, k

    put(take(1), MAIN, 0)
    put(take(NA), MAIN, A0 + 10 * np.arange(NA))
    put(take(NP), MAIN, PLATEAU)
    run = list(take(NBIG - len(DUPS)))
    for i, v in enumerate(DUPS):  # the copies, 55 ranks apart
        run.insert(i * 55, v)
    put(np.array(run), MAIN, BIG0 + 10 * np.arange(NBIG))
    put(take(NTWIN), TWIN, A0 + 10 * np.arange(NTWIN))
    put(take(NTWINP), TWIN, PLATEAU)
    put(take(NTOPL - 1), TOPL, A0 + 10 * np.arange(NTOPL - 1))
    put(take(1), TOPL, TOP)
    put(take(NZERO), ZERO, 5 * np.arange(NZERO))
    put(take(NHALF), MAIN, NONE)                         # a label, no value
    put(take(NHALF), NONE, A0 + 10 * np.arange(NHALF))   # a value, no label
    assert not o
    # what the docstring says of it
    listed = (labels != NONE) & (keys != NONE)
    assert listed.sum() == LISTED == N - 2 * NHALF and ((labels != NONE) & ~listed).sum() == NHALF == ((keys != NONE) & ~listed).sum()
    assert [(listed & (labels == x)).sum() for x in (MAIN, TWIN, TOPL, ZERO)] == [NMAIN, NTWIN + NTWINP, NTOPL, NZERO]
    assert ((labels == MAIN) & (keys == PLATEAU)).sum() == NP and ((labels == TWIN) & (keys == PLATEAU)).sum() == NTWINP
    big = (labels == MAIN) & (keys >= BIG0) & (keys != NONE)
    assert big.sum() == NBIG > 2048 and big[DUPS].all()
    ranks = np.sort((keys[DUPS].astype(np.int64) - BIG0) // 10)
    assert ranks[0] == 0 and ranks[-1] == 39 * 55 > 2048 and len(set((ranks // 64).tolist())) > 30
    comp = (labels.astype(np.uint64) << np.uint64(32)) | keys.astype(np.uint64)
    order = np.argsort(comp, kind="stable")[:LISTED]
    assert (np.diff(order) < 0).sum() > 1000  # span order is not id order
    labels.setflags(write=False), keys.setflags(write=False)
    return labels, keys


# (want, lo, hi, rows) in u32 labels and keys: every span the docstring names
PAIRS = [
    (MAIN, BIG0, BIG0 + 10 * (NBIG - 1), NBIG),  # more than 2048 rows, all 40 copies
    (MAIN, A0, A0, 1),
    (MAIN, A0 + 1000, A0 + 1630, 64),
    (MAIN, A0 + 1000, A0 + 1640, 65),
    (MAIN, PLATEAU, PLATEAU, NP),
    (TWIN, PLATEAU, PLATEAU, NTWINP),            # the plateau's key under another label
    (TWIN, A0, A0 + 10 * (NTWIN - 1), NTWIN),    # one range ...
    (MAIN, A0, A0 + 10 * (NTWIN - 1), NTWIN),    # ... two labels
    (TWIN, 0, NONE, NTWIN + NTWINP),             # no upper end at a middle label
    (TOPL, 0, NONE, NTOPL),                      # ... and at the last one
    (TOPL, TOP, NONE, 1),
    (ZERO, 0, 0, 1),
    (ZERO, 0, NONE, NZERO),
    (MAIN, 0, NONE, NMAIN),                      # rows with the label but no value are in no span
    (MAIN, 5000, 2000, 0),                       # lo > hi, with keys between
    (NONE, 0, NONE, 0),                          # the NONE label: rows without a label are in no span
    (5, 0, NONE, 0),                             # labels nobody carries: between ...
    (MAIN + 1, 0, NONE, 0),
    (0x7FFFFFFF, 0, NONE, 0),
    (0xFFFFFFFD, 0, NONE, 0),
    (MAIN, 5, 900, 0),                           # a gap
    (MAIN, A0 + 10 * (NA - 1), PLATEAU, NP + 1),  # the plateau and the row before it
    (MAIN, PLATEAU, BIG0, NP + 1),               # ... and the row after it
    (TOPL, 0, TOP, NTOPL),
]


def cycle_pairs(nq=NQX):
    """(want, lo, hi) u32 [nq]: query 0 (the duplicated row) gets the big run, the others go round every pair"""
    return tuple(np.array([PAIRS[i % len(PAIRS)][j] for i in range(nq)], dtype=np.uint32) for j in range(3))


def masks(want, lo, hi, members=None, cols=None):
    labels, keys = cols or columns()
    return lr.masks_of(labels, keys, want, lo, hi, members)


def test_the_pairs_hold_the_rows_they_are_named_for():
    assert masks(*cycle_pairs(len(PAIRS))).sum(1).tolist() == [p[3] for p in PAIRS]


def make_handle(hix):
    labels, keys = columns()
    return ph.LabeledAttribute(hix, labels, values_of(np.where(keys == NONE, 0, keys)), missing=keys == NONE)


@functools.lru_cache(maxsize=None)
def handle(kind, dim, metric=COS):
    return make_handle(world_of(kind, dim, metric)["hix"])


def staged(hix, at, k, want, lo, hi, queries=None, qids=None, exclude=None):
    """the inputs and outputs of one phnsw_search_exact_label_ranged_device call, uploaded; no synchronisation here.
    Returns (launch, out): launch(stream) enqueues the call and nothing else, out is what fetch takes"""
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
    wd, lod, hid = (up(np.asarray(x, dtype=np.uint32), np.int32).data_ptr() for x in (want, lo, hi))
    ids = torch.full((nq, k), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev)
    ln = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    status = torch.full((nq,), -1, dtype=torch.int32, device=dev)

    def launch(stream=None):
        hix.search_exact_label_ranged_device(at, nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(),
                                             queries=qd, ldq=ld, qids=qi, exclude=ex, want=wd, lo=lod, hi=hid,
                                             stream=0 if stream is None else stream.cuda_stream)

    return launch, (ids, d, ln, status, keep)


def device_call(hix, at, k, want, lo, hi, queries=None, qids=None, exclude=None):
    """the device form between two events on a side stream, with no host synchronisation between staging's one and the
    fetch: the call enqueues and returns"""
    import torch
    launch, out = staged(hix, at, k, want, lo, hi, queries=queries, qids=qids, exclude=exclude)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    before, after = torch.cuda.Event(), torch.cuda.Event()
    before.record(stream)
    launch(stream)
    after.record(stream)
    return fetch(out)


def check(w, at, want, lo, hi, nq=NQX, exclude=None, k=10, members=None, hix=None, device=True, forms=(0, 1), scan=True):
    """raw (0) and stored (1) queries, host and device form, against both yardsticks -> the host results by form"""
    hix = hix or w["hix"]
    want, lo, hi = (np.asarray(x, dtype=np.uint32)[:nq] for x in (want, lo, hi))
    allow = masks(want, lo, hi)
    out = {}
    for form in forms:
        kw, D = (dict(queries=w["q"][:nq]), w["Dq"][:nq]) if form == 0 else (dict(qids=w["qids"][:nq]), w["Ds"][:nq])
        e = None if exclude is None else exclude[:nq]
        ref = xr.exact_topk(D, allow, e, members, k)
        got = hix.search_exact_label_ranged(attr=at, want=want, lo=values_of(lo), hi=values_of(hi), exclude=e, k=k, **kw)
        same(got, ref)
        if scan:
            same(got, hix.search_exact_filtered(allow=allow, exclude=e, k=k, **kw))
        assert (got[0][np.arange(k)[None, :] >= got[2][:, None]] == EMPTY).all()
        assert (bits(got[1])[np.arange(k)[None, :] >= got[2][:, None]] == bits(xr.FMAX)).all()
        if device:
            dv = device_call(hix, at, k, want, lo, hi, exclude=e, **kw)
            assert not dv[3].any()
            same(dv, ref)
        out[form] = got
    return out


# ---------------------------------------------------------------- the handle
def test_the_handle_describes_the_columns():
    at = handle("f32", 24)
    assert at.info() == (N, LISTED, 4, NMAIN) and at.listed == LISTED and at.dtype == np.int32
    want, lo, hi = cycle_pairs()
    m = masks(want, lo, hi)
    got = at.count(want, values_of(lo), values_of(hi))
    np.testing.assert_array_equal(got, m.sum(1))
    np.testing.assert_array_equal(got, world_of("f32", 24)["hix"].filter_count(m))
    assert at.count(np.array([TWIN, MAIN]), values_of(np.array([PLATEAU], dtype=np.uint32))[0], None).tolist() == [NTWINP, NP + NBIG]


def test_a_handle_from_device_columns_gives_the_same_rows():
    import torch
    w = sworld("f32", 24)
    labels, keys = columns()
    tl = torch.from_numpy(labels.copy().view(np.int32)).to(torch.device("cuda", 0))
    tk = torch.from_numpy(keys.copy().view(np.int32)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    at = ph.LabeledAttribute.from_device(w["hix"], tl.data_ptr(), tk.data_ptr(), dtype=np.int32)
    assert at.info() == handle("f32", 24).info()
    check(w, at, *cycle_pairs(), k=10)
    at.close()
    at.close()  # twice: a no-op


# ---------------------------------------------------------------- 1: kinds x dimensions, k, exclude
@pytest.mark.parametrize("kind,dim", KINDS)
def test_kinds_and_dimensions(kind, dim):
    w, at = world_of(kind, dim), handle(kind, dim)
    want, lo, hi = cycle_pairs()
    got = check(w, at, want, lo, hi, k=10)
    if kind not in ("i8q", "pq"):  # normalised rows: nothing is nearer to a row than its copies
        for form in (0, 1):  # query 0 is the duplicated row: the copies tie, ids decide, whatever order the span has them in
            np.testing.assert_array_equal(got[form][0][0], DUPS[:10].astype(np.uint64))
    check(w, at, want, lo, hi, k=1, device=False)
    first = check(w, at, want, lo, hi, k=64)
    counts = masks(want, lo, hi).sum(1)
    for form in (0, 1):
        best = first[form][0][:, 0]  # each query's best hit, where it has one: inside its span, and it matters
        inside = np.where(best == EMPTY, np.uint64(5), best)
        got = check(w, at, want, lo, hi, exclude=inside, k=64, forms=(form,))[form]
        has = best != EMPTY
        assert not (got[0][has] == best[has, None]).any()
        np.testing.assert_array_equal(got[2][has], np.minimum(64, counts[has] - 1))
    # an exclude outside the span (a row with a label but no value, one with a value but no label, an id past n,
    # PHNSW_EMPTY) changes nothing
    labels, keys = columns()
    outside = np.full(NQX, EMPTY, dtype=np.uint64)
    outside[0::4] = int(np.nonzero((labels == MAIN) & (keys == NONE))[0][0])
    outside[1::4] = int(np.nonzero((labels == NONE) & (keys != NONE))[0][0])
    outside[2::4] = N + 7
    got = check(w, at, want, lo, hi, exclude=outside, k=64, device=False)
    for form in (0, 1):
        same(got[form], first[form])


def test_k_1024_returns_whole_spans_with_their_ties():
    w, at = sworld("f32", 256), handle("f32", 256)
    want, lo, hi = cycle_pairs()
    got = check(w, at, want, lo, hi, k=1024)
    counts = masks(want, lo, hi).sum(1)
    for form in (0, 1):
        np.testing.assert_array_equal(got[form][2], np.minimum(counts, 1024))
        np.testing.assert_array_equal(got[form][0][0, :40], DUPS.astype(np.uint64))
        assert len(set(bits(got[form][1][0, :40]).tolist())) == 1


@pytest.mark.parametrize("metric", [oracle.METRIC_COSINE_HALF, oracle.METRIC_L2, oracle.METRIC_ONE_MINUS_DOT])
def test_three_metrics_on_f32(metric):
    w = world_of("f32", 256, metric)  # (the handle's index: world_of keys its cache on the call's form)
    check(w, handle("f32", 256, metric), *cycle_pairs(), k=100)


# ---------------------------------------------------------------- 2: slices
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("f16", 24), ("i8q", 256), ("pq", 24)])
def test_rows_do_not_depend_on_the_slices(monkeypatch, kind, dim):
    w, at = world_of(kind, dim), handle(kind, dim)
    cyc = cycle_pairs()
    big = tuple(np.full(NQX, PAIRS[0][j], dtype=np.uint32) for j in range(3))
    base = [check(w, at, *r, k=100) for r in (cyc, big)]
    for slices in ("1", "2", "7"):
        with env(monkeypatch, PHNSW_LABEL_RANGE_SLICES=slices):
            for r, b in zip((cyc, big), base):
                now = check(w, at, *r, k=100, scan=False)
                for form in (0, 1):
                    same(now[form], b[form])


# ---------------------------------------------------------------- 3: the device form
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("i8q", 24)])
def test_a_stored_query_id_past_n_is_reported_and_harms_nobody(monkeypatch, kind, dim):
    w, at = world_of(kind, dim), handle(kind, dim)
    want, lo, hi = cycle_pairs(40)
    qids = w["qids"][:40].copy()
    bad = [0, 17, 39]
    qids[bad] = [N, N + 12345, 0xFFFFFFFE]
    ref = xr.exact_topk(w["Ds"][:40], masks(want, lo, hi), None, None, 10)
    good = np.setdiff1d(np.arange(40), bad)
    for kw in (dict(), dict(PHNSW_LABEL_RANGE_SLICES="3")):
        with env(monkeypatch, **kw):
            dv = device_call(w["hix"], at, 10, want, lo, hi, qids=qids)
        same(tuple(x[good] for x in dv[:3]), tuple(x[good] for x in ref))
        assert (dv[3][bad] == 4).all() and not dv[3][good].any()
        assert (dv[0][bad] == EMPTY).all() and (bits(dv[1][bad]) == bits(xr.FMAX)).all() and not dv[2][bad].any()
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses such an id, as the other exact calls do
        w["hix"].search_exact_label_ranged(qids=qids, attr=at, want=want, lo=values_of(lo), hi=values_of(hi), k=10)
    assert e.value.code == -1 and "phnsw_search_exact_label_ranged:" in str(e.value) and "out of range" in str(e.value)


# ---------------------------------------------------------------- 4: an index over part of its store
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("i8q", 256)])
def test_vectors_outside_the_index_are_never_listed(kind, dim):
    w = world_of(kind, dim)
    labels, keys = columns()
    even = np.arange(N) % 2 == 0
    hix = ph.Hnsw.from_layers(w["store"], ring(np.arange(0, N, 2)))  # every second vector: vec2node is not the identity
    at = make_handle(hix)  # the odd rows carry labels and values too
    listed = even & (labels != NONE) & (keys != NONE)
    per_label = [int((listed & (labels == x)).sum()) for x in (MAIN, TWIN, TOPL, ZERO)]
    assert at.info() == (N, listed.sum(), 4, max(per_label))
    want, lo, hi = cycle_pairs()
    m = masks(want, lo, hi)
    np.testing.assert_array_equal(at.count(want, values_of(lo), values_of(hi)), hix.filter_count(m))
    np.testing.assert_array_equal(at.count(want, values_of(lo), values_of(hi)), masks(want, lo, hi, even).sum(1))
    got = check(w, at, want, lo, hi, members=even, hix=hix, k=100)
    for form in (0, 1):
        assert not (got[form][0][got[form][0] != EMPTY] % 2).any()


# ---------------------------------------------------------------- 5: refusals
def test_refusals():
    w, at = sworld("f32", 24), handle("f32", 24)
    hix, q = w["hix"], w["q"][:4]
    for k in (0, 1025):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_label_ranged(queries=q, attr=at, want=7, lo=0, hi=5, k=k)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_label_ranged: k must be 1..1024 (got %d)" % k
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_label_ranged_device(at, 4, k, 8, 8, 8, 8, qids=8, want=8, lo=8, hi=8)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_label_ranged_device: k must be 1..1024 (got %d)" % k
    # a handle made for another index over the same store: the wording of the labels
    other = ph.Hnsw.from_layers(w["store"], ring(np.arange(N)))
    for call in (lambda: other.search_exact_label_ranged(queries=q, attr=at, want=7, lo=0, hi=5, k=3),
                 lambda: other.search_exact_label_ranged_device(at, 4, 3, 8, 8, 8, 8, qids=8, want=8, lo=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        msg = str(e.value)
        assert e.value.code == -1 and "are stale: made for another index" in msg and "phnsw_search_exact_label_ranged" in msg
        assert "make a new handle" in msg
    with pytest.raises(ph.PhnswError) as e:  # the handle is looked at before the other arguments, k before the handle
        other.search_exact_label_ranged_device(at, 4, 0, 8, 8, 8, 8, qids=8, want=8, lo=8, hi=8)
    assert "k must be" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:
        other.search_exact_label_ranged_device(at, 4, 3, 8, 8, 8, 8)
    assert "stale" in str(e.value)
    for bad in (dict(queries=16, ldq=24, qids=8, want=8, lo=8, hi=8), dict(want=8, lo=8, hi=8), dict(qids=8, lo=8, hi=8),
                dict(qids=8, want=8, lo=8), dict(qids=8, want=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_label_ranged_device(at, 4, 3, 8, 8, 8, 8, **bad)
        assert e.value.code == -1 and "phnsw_search_exact_label_ranged_device: invalid argument" in str(e.value)
    ids, d, ln = hix.search_exact_label_ranged(queries=np.zeros((0, 24), dtype=np.float32), attr=at, want=7, lo=0, hi=1, k=3)
    assert ids.shape == (0, 3)  # nq == 0: a no-op
    import ctypes as C
    lib = ph.lib()
    # a null handle: PHNSW_E_INVALID, before the other arguments are looked at
    assert lib.phnsw_search_exact_label_ranged(hix._h, None, None, None, 4, None, None, None, None, 3, None, None, None) == -1
    assert "phnsw_search_exact_label_ranged" in lib.phnsw_last_error().decode()
    out = C.c_void_p()
    labels, keys = columns()
    assert lib.phnsw_label_attr_create(hix._h, labels.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p), N - 1,
                                       C.byref(out)) == -1
    msg = lib.phnsw_last_error().decode()
    assert msg.startswith("phnsw_label_attr_create: %d labels and keys for a store of %d vectors" % (N - 1, N)) and not out.value


def test_a_handle_is_stale_after_the_store_has_grown():
    rows = oracle.synth_rows(0, 300, 24)[:, :24].copy()
    store = ph.VectorStore(rows[:200], metric=COS)
    hix = ph.Hnsw.from_layers(store, ring(np.arange(200)))
    val = (np.arange(200) * 7 % 50).astype(np.int32) - 25
    lab = (np.arange(200) % 3).astype(np.uint32)
    at = ph.LabeledAttribute(hix, lab, val)
    want = np.array([0, 1, 2], dtype=np.uint32)
    lo, hi = np.array([-25, 0, 10], dtype=np.int32), np.array([-20, 0, 24], dtype=np.int32)
    allow = (lab[None, :] == want[:, None]) & (val[None, :] >= lo[:, None]) & (val[None, :] <= hi[:, None])
    same(hix.search_exact_label_ranged(queries=rows[:3], attr=at, want=want, lo=lo, hi=hi, k=5),
         hix.search_exact_filtered(queries=rows[:3], allow=allow, k=5))
    store.append(rows[200:])
    with pytest.raises(ph.PhnswError) as e:
        hix.search_exact_label_ranged(queries=rows[:3], attr=at, want=want, lo=lo, hi=hi, k=5)
    assert e.value.code == -1 and "are stale: made for this index before it changed" in str(e.value)
    at2 = ph.LabeledAttribute(hix, np.concatenate([lab, np.zeros(100, dtype=np.uint32)]),
                              np.concatenate([val, np.zeros(100, dtype=np.int32)]))
    assert at2.listed == 200  # the appended vectors are not in the index, so they are not listed
    allow2 = np.concatenate([allow, np.ones((3, 100), dtype=bool)], axis=1)
    same(hix.search_exact_label_ranged(queries=rows[:3], attr=at2, want=want, lo=lo, hi=hi, k=5),
         hix.search_exact_filtered(queries=rows[:3], allow=allow2, k=5))
