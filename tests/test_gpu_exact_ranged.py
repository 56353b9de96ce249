"""The exact top-k by a numeric range (phnsw_attr_*, phnsw_search_exact_ranged[_device], filter_ranged.hip): one span of
a column sorted once instead of a bitmap per query.  Every comparison is on ids, distance bits, lengths and status, no
tolerance anywhere.

Two yardsticks, both for every case: tests/exact_filter_reference.py over the oracle's distances with the bitmaps
ranged_reference.masks_of makes of the key column, which the code under test did not make, and the existing scan,
search_exact_filtered with those masks as per-query bitmaps, whose rows the new call promises bit for bit.

The worlds are those of tests/test_gpu_exact_shared.py (N = 5000, 40 copies of row 0 spread over the id range, 65 raw and
65 stored queries, one-layer ring indexes).  The key column is constructed, not drawn.  In key order: one row with key
0; 1500 rows with distinct keys (spans of exactly 1, 64 and 65 rows are cut from them); a plateau of 300 rows with ONE
key; a run of 2200 rows with distinct keys that holds the 40 copies, 55 ranks apart (35 batches of 64: the ties cross
batch and slice borders); 898 more rows; one row with key 0xFFFFFFFE; 100 rows without a value.  The rows take their
ranks in a random order, so the ids of a span are not ascending.  The column is held as int32 values, whose map covers
all of the u32 keys a bound can be (INT32_MAX is the key 0xFFFFFFFF, "no upper end")."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import ranged_reference as rr
from test_gpu_exact_filter import COS, DUPS, EMPTY, N, ring, same, stores
from test_gpu_exact_labeled import world_of
from test_gpu_exact_shared import NQX, fetch, sworld
from test_gpu_i8 import bits
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

NONE = rr.ATTR_NONE
TOP = 0xFFFFFFFE
A0, PLATEAU, BIG0, TAIL0 = 1000, 100000, 200000, 400000  # first key of the distinct run, the plateau, the big run, the tail
NA, NP, NBIG, NTAIL, NMISSING = 1500, 300, 2200, 898, 100
KINDS = [(k, d) for k in ("f32", "f16", "i8", "i8q") for d in (24, 256)] + [("f32", 768), ("pq", 24)]


@functools.lru_cache(maxsize=None)
def column():
    """the key of every vector, u32 [N]"""
    keys = np.full(N, NONE, dtype=np.uint32)
    o = np.random.default_rng(2025).permutation(np.setdiff1d(np.arange(N), DUPS))
    keys[o[0]] = 0
    keys[o[1:1 + NA]] = A0 + 10 * np.arange(NA)
    keys[o[1 + NA:1 + NA + NP]] = PLATEAU
    run = list(o[1 + NA + NP:1 + NA + NP + NBIG - len(DUPS)])
    for i, v in enumerate(DUPS):  # the copies, 55 ranks apart
        run.insert(i * 55, v)
    keys[np.array(run)] = BIG0 + 10 * np.arange(NBIG)
    at = 1 + NA + NP + NBIG - len(DUPS)
    keys[o[at:at + NTAIL]] = TAIL0 + 10 * np.arange(NTAIL)
    keys[o[at + NTAIL]] = TOP
    assert at + NTAIL + 1 + NMISSING == len(o)
    # what the docstring says of it
    assert (keys == NONE).sum() == NMISSING and (keys == 0).sum() == 1 and (keys == TOP).sum() == 1
    assert (keys == PLATEAU).sum() == NP
    big = (keys >= BIG0) & (keys < TAIL0)
    assert big.sum() == NBIG > 2048 and big[DUPS].all()
    ranks = np.sort((keys[DUPS].astype(np.int64) - BIG0) // 10)
    assert ranks[0] == 0 and ranks[-1] == 39 * 55 > 2048 and len(set((ranks // 64).tolist())) > 30
    order = np.argsort(keys, kind="stable")[:N - NMISSING]
    assert (np.diff(order) < 0).sum() > 1000  # span order is not id order
    keys.setflags(write=False)
    return keys


def values_of(keys):
    """the int32 values whose keys these are"""
    return (np.asarray(keys, dtype=np.uint32) ^ np.uint32(0x80000000)).view(np.int32)


# (lo, hi, rows) in u32 keys: every span the issue names
RANGES = [
    (BIG0, BIG0 + 10 * (NBIG - 1), NBIG),  # more than 2048 rows, all 40 copies
    (5, 900, 0),                           # a gap
    (5000, 2000, 0),                       # lo > hi, with keys between
    (NONE, NONE, 0),                       # above the maximum: rows without a value are in no span
    (A0, A0, 1),
    (A0 + 1000, A0 + 1630, 64),
    (A0 + 1000, A0 + 1640, 65),
    (PLATEAU, PLATEAU, NP),                # lo == hi on the plateau
    (A0 + 10 * (NA - 1), PLATEAU, NP + 1),  # the plateau and the row before it
    (PLATEAU, BIG0, NP + 1),               # ... and the row after it
    (PLATEAU + 1, BIG0, 1),                # just past the plateau
    (A0 + 10 * (NA - 1), PLATEAU - 1, 1),  # just before it
    (0, TOP, N - NMISSING),                # everything
    (0, NONE, N - NMISSING),               # everything, no upper end
    (0, 0, 1),
    (TOP, NONE, 1),
    (TAIL0 - 5, TAIL0 + 10 * 99 + 5, 100),  # bounds in gaps
]


def cycle_ranges(nq=NQX):
    """(lo, hi) u32 [nq]: query 0 (the duplicated row) gets the big run, the others go round every range"""
    lo = np.array([RANGES[i % len(RANGES)][0] for i in range(nq)], dtype=np.uint32)
    hi = np.array([RANGES[i % len(RANGES)][1] for i in range(nq)], dtype=np.uint32)
    return lo, hi


def test_the_ranges_hold_the_rows_they_are_named_for():
    lo, hi = cycle_ranges(len(RANGES))
    assert rr.masks_of(column(), lo, hi).sum(1).tolist() == [r[2] for r in RANGES]


@functools.lru_cache(maxsize=None)
def handle(kind, dim, metric=COS):
    keys = column()
    return ph.Attribute(world_of(kind, dim, metric)["hix"], values_of(np.where(keys == NONE, 0, keys)), missing=keys == NONE)


def staged_ranged(hix, at, k, lo, hi, queries=None, qids=None, exclude=None):
    """the inputs and outputs of one phnsw_search_exact_ranged_device call, uploaded; no synchronisation here.  Returns
    (launch, out): launch(stream) enqueues the call and nothing else, out is what fetch takes"""
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
    lod = up(np.asarray(lo, dtype=np.uint32), np.int32).data_ptr()
    hid = up(np.asarray(hi, dtype=np.uint32), np.int32).data_ptr()
    ids = torch.full((nq, k), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev)
    ln = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    status = torch.full((nq,), -1, dtype=torch.int32, device=dev)

    def launch(stream=None):
        hix.search_exact_ranged_device(at, nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd,
                                       ldq=ld, qids=qi, exclude=ex, lo=lod, hi=hid,
                                       stream=0 if stream is None else stream.cuda_stream)

    return launch, (ids, d, ln, status, keep)


def device_ranged(hix, at, k, lo, hi, queries=None, qids=None, exclude=None, stream=None):
    import torch
    launch, out = staged_ranged(hix, at, k, lo, hi, queries=queries, qids=qids, exclude=exclude)
    torch.cuda.synchronize()
    launch(stream)
    return fetch(out)


def check(w, at, lo, hi, nq=NQX, exclude=None, k=10, members=None, hix=None, device=True, forms=(0, 1), scan=True, keys=None):
    """raw (0) and stored (1) queries, host and device form, against both yardsticks -> the host results by form"""
    hix = hix or w["hix"]
    lo, hi = np.asarray(lo, dtype=np.uint32)[:nq], np.asarray(hi, dtype=np.uint32)[:nq]
    allow = rr.masks_of(column() if keys is None else keys, lo, hi)
    out = {}
    for form in forms:
        kw, D = (dict(queries=w["q"][:nq]), w["Dq"][:nq]) if form == 0 else (dict(qids=w["qids"][:nq]), w["Ds"][:nq])
        e = None if exclude is None else exclude[:nq]
        ref = xr.exact_topk(D, allow, e, members, k)
        got = hix.search_exact_ranged(attr=at, lo=values_of(lo), hi=values_of(hi), exclude=e, k=k, **kw)
        same(got, ref)
        if scan:
            same(got, hix.search_exact_filtered(allow=allow, exclude=e, k=k, **kw))
        assert (got[0][np.arange(k)[None, :] >= got[2][:, None]] == EMPTY).all()
        assert (bits(got[1])[np.arange(k)[None, :] >= got[2][:, None]] == bits(xr.FMAX)).all()
        if device:
            dv = device_ranged(hix, at, k, lo, hi, exclude=e, **kw)
            assert not dv[3].any()
            same(dv, ref)
        out[form] = got
    return out


# ---------------------------------------------------------------- the handle
def test_the_handle_describes_the_column():
    at, keys = handle("f32", 24), column()
    assert at.info() == (N, N - NMISSING, 0, TOP) and at.listed == N - NMISSING and at.dtype == np.int32
    lo, hi = cycle_ranges()
    masks = rr.masks_of(keys, lo, hi)
    got = at.count(values_of(lo), values_of(hi))
    np.testing.assert_array_equal(got, masks.sum(1))
    np.testing.assert_array_equal(got, world_of("f32", 24)["hix"].filter_count(masks))
    assert at.count(values_of(np.array([PLATEAU], dtype=np.uint32)), None).tolist() == [N - NMISSING - 1 - NA]
    assert at.count(None, values_of(np.array([PLATEAU], dtype=np.uint32))).tolist() == [1 + NA + NP]


def test_a_handle_from_device_keys_gives_the_same_rows():
    import torch
    w = sworld("f32", 24)
    t = torch.from_numpy(column().copy().view(np.int32)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    at = ph.Attribute.from_device(w["hix"], t.data_ptr(), dtype=np.int32)
    assert at.info() == handle("f32", 24).info()
    check(w, at, *cycle_ranges(), k=10)
    at.close()
    at.close()  # twice: a no-op


def test_float_and_unsigned_columns_go_through_their_maps():
    w = sworld("f32", 24)
    rng = np.random.default_rng(8)
    f = rng.standard_normal(N).astype(np.float32)
    f[:6] = [-0.0, 0.0, np.inf, -np.inf, 1e-45, -1e-45]
    missing = np.zeros(N, dtype=bool)
    missing[10:60] = True
    f[10:20] = np.nan  # a missing row may hold anything
    at = ph.Attribute(w["hix"], f, missing=missing)
    keys = rr.keys_of(np.where(missing, np.float32(0), f))
    keys[missing] = NONE
    lo = np.array([-0.5, 0.0, -np.inf, 0.25, 1.0, -0.0], dtype=np.float32)
    hi = np.array([0.5, 0.0, np.inf, 0.25, -1.0, 1e-45], dtype=np.float32)
    allow = rr.masks_of(keys, rr.keys_of(lo), rr.keys_of(hi))
    plain = ~missing[None, :] & (f[None, :] >= lo[:, None]) & (f[None, :] <= hi[:, None])  # the range as numpy reads it
    np.testing.assert_array_equal(allow, plain)
    assert allow[1].sum() == 2 and allow[2].sum() == N - 50 and not allow[4].any() and allow[5].sum() == 3
    got = w["hix"].search_exact_ranged(queries=w["q"][:6], attr=at, lo=lo, hi=hi, k=100)
    same(got, w["hix"].search_exact_filtered(queries=w["q"][:6], allow=allow, k=100))
    same(w["hix"].search_exact_ranged(queries=w["q"][:6], attr=at, lo=-0.5, hi=None, k=10),
         w["hix"].search_exact_filtered(queries=w["q"][:6], allow=np.tile(~missing & (f >= -0.5), (6, 1)), k=10))
    with pytest.raises(ValueError, match="index 3: NaN"):
        ph.Attribute(w["hix"], np.where(np.arange(N) >= 3, np.float32(np.nan), f))
    u = rng.integers(0, 1000, N).astype(np.uint32)
    au = ph.Attribute(w["hix"], u)
    assert au.info() == (N, N, int(u.min()), int(u.max()))
    got = w["hix"].search_exact_ranged(qids=w["qids"][:4], attr=au, lo=np.array([0, 10, 999, 500], dtype=np.uint32), hi=20, k=64)
    allow = (u[None, :] >= np.array([0, 10, 999, 500])[:, None]) & (u[None, :] <= 20)
    same(got, w["hix"].search_exact_filtered(qids=w["qids"][:4], allow=allow, k=64))
    with pytest.raises(ValueError, match="index 7: 0xFFFFFFFF"):
        ph.Attribute(w["hix"], np.where(np.arange(N) == 7, np.uint32(0xFFFFFFFF), u))


# ---------------------------------------------------------------- 1: kinds x dimensions, k, exclude
@pytest.mark.parametrize("kind,dim", KINDS)
def test_kinds_and_dimensions(kind, dim):
    w, at = world_of(kind, dim), handle(kind, dim)
    lo, hi = cycle_ranges()
    got = check(w, at, lo, hi, k=10)
    if kind not in ("i8q", "pq"):  # normalised rows: nothing is nearer to a row than its copies
        for form in (0, 1):  # query 0 is the duplicated row: the copies tie, ids decide, whatever order the span has them in
            np.testing.assert_array_equal(got[form][0][0], DUPS[:10].astype(np.uint64))
    check(w, at, lo, hi, k=1, device=False)
    first = check(w, at, lo, hi, k=64)
    counts = rr.masks_of(column(), lo, hi).sum(1)
    for form in (0, 1):
        best = first[form][0][:, 0]  # each query's best hit, where it has one: inside its range, and it matters
        inside = np.where(best == EMPTY, np.uint64(5), best)
        got = check(w, at, lo, hi, exclude=inside, k=64, forms=(form,))[form]
        has = best != EMPTY
        assert not (got[0][has] == best[has, None]).any()
        np.testing.assert_array_equal(got[2][has], np.minimum(64, counts[has] - 1))
    # an exclude outside the range (a row without a value, an id past n, PHNSW_EMPTY) changes nothing
    outside = np.full(NQX, EMPTY, dtype=np.uint64)
    outside[0::3] = int(np.nonzero(column() == NONE)[0][0])
    outside[1::3] = N + 7
    got = check(w, at, lo, hi, exclude=outside, k=64, device=False)
    for form in (0, 1):
        same(got[form], first[form])


def test_k_1024_returns_whole_spans_with_their_ties():
    w, at = sworld("f32", 256), handle("f32", 256)
    lo, hi = cycle_ranges()
    got = check(w, at, lo, hi, k=1024)
    counts = rr.masks_of(column(), lo, hi).sum(1)
    for form in (0, 1):
        np.testing.assert_array_equal(got[form][2], np.minimum(counts, 1024))
        np.testing.assert_array_equal(got[form][0][0, :40], DUPS.astype(np.uint64))
        assert len(set(bits(got[form][1][0, :40]).tolist())) == 1


# ---------------------------------------------------------------- 2: slices
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("f16", 24), ("i8q", 256), ("pq", 24)])
def test_rows_do_not_depend_on_the_slices(monkeypatch, kind, dim):
    w, at = world_of(kind, dim), handle(kind, dim)
    lo, hi = cycle_ranges()
    big = (np.full(NQX, RANGES[0][0], dtype=np.uint32), np.full(NQX, RANGES[0][1], dtype=np.uint32))
    base = [check(w, at, *r, k=100) for r in ((lo, hi), big)]
    for slices in ("1", "3", "7"):
        with env(monkeypatch, PHNSW_RANGE_SLICES=slices):
            for r, b in zip(((lo, hi), big), base):
                now = check(w, at, *r, k=100, scan=False)
                for form in (0, 1):
                    same(now[form], b[form])


# ---------------------------------------------------------------- 3: the device form
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("i8q", 24)])
def test_a_stored_query_id_past_n_is_reported_and_harms_nobody(monkeypatch, kind, dim):
    w, at = world_of(kind, dim), handle(kind, dim)
    lo, hi = cycle_ranges(40)
    qids = w["qids"][:40].copy()
    bad = [0, 17, 39]
    qids[bad] = [N, N + 12345, 0xFFFFFFFE]
    ref = xr.exact_topk(w["Ds"][:40], rr.masks_of(column(), lo, hi), None, None, 10)
    good = np.setdiff1d(np.arange(40), bad)
    for kw in (dict(), dict(PHNSW_RANGE_SLICES="3")):
        with env(monkeypatch, **kw):
            dv = device_ranged(w["hix"], at, 10, lo, hi, qids=qids)
        same(tuple(x[good] for x in dv[:3]), tuple(x[good] for x in ref))
        assert (dv[3][bad] == 4).all() and not dv[3][good].any()
        assert (dv[0][bad] == EMPTY).all() and (bits(dv[1][bad]) == bits(xr.FMAX)).all() and not dv[2][bad].any()
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses such an id, as the other exact calls do
        w["hix"].search_exact_ranged(qids=qids, attr=at, lo=values_of(lo), hi=values_of(hi), k=10)
    assert e.value.code == -1 and "phnsw_search_exact_ranged:" in str(e.value) and "out of range" in str(e.value)


def test_calls_in_flight_on_several_streams_with_no_synchronisation_between_them(monkeypatch):
    """Everything is uploaded first and the device is synchronised ONCE; then 18 calls are enqueued back to back on five
    streams (more than the four scratch sets a handle makes before calls share one) and on the default stream, with
    nothing between them that waits; only then are the rows fetched.  The calls differ in ranges, form, k, batch size and
    slice count, so a set is handed on while its last call may still run and its blocks grow behind unfinished work: a
    call that synchronised would be no error here, but one that read another's scratch would return another's rows."""
    import torch
    w = sworld("f32", 256)
    keys = column()
    at = ph.Attribute(w["hix"], values_of(np.where(keys == NONE, 0, keys)), missing=keys == NONE)  # no scratch set exists yet
    lo, hi = cycle_ranges()
    big = (np.full(NQX, RANGES[0][0], dtype=np.uint32), np.full(NQX, RANGES[0][1], dtype=np.uint32))
    shapes = [((lo, hi), 0, 16, 10, None), ((lo, hi), 1, 65, 100, "7"), (big, 0, 65, 64, "3"), ((lo, hi), 0, 40, 1, None),
              (big, 1, 33, 1024, "3"), ((lo, hi), 1, 65, 10, "1")]

    def kwargs(form, nq):
        return dict(queries=w["q"][:nq]) if form == 0 else dict(qids=w["qids"][:nq])

    expect = [xr.exact_topk((w["Dq"], w["Ds"])[form][:nq], rr.masks_of(keys, r[0][:nq], r[1][:nq]), None, None, k)
              for r, form, nq, k, _ in shapes]
    streams = [torch.cuda.Stream() for _ in range(5)] + [None]
    plan = [((j + r) % 6, streams[(j * (r + 1) + r) % 6]) for r in range(3) for j in range(6)]
    staged = [staged_ranged(w["hix"], at, shapes[i][3], shapes[i][0][0][:shapes[i][2]], shapes[i][0][1][:shapes[i][2]],
                            **kwargs(shapes[i][1], shapes[i][2])) for i, _ in plan]
    torch.cuda.synchronize()  # the one synchronisation: inputs and outputs are there
    for (i, stream), (launch, _) in zip(plan, staged):
        slices = shapes[i][4]
        with env(monkeypatch, **({} if slices is None else {"PHNSW_RANGE_SLICES": slices})):
            launch(stream)  # enqueues and returns; nothing waits for the device
    for (i, _), (_, out) in zip(plan, staged):
        got = fetch(out)
        assert not got[3].any()
        same(got, expect[i])
    at.close()


# ---------------------------------------------------------------- 4: an index over part of its store
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("i8q", 256)])
def test_vectors_outside_the_index_are_never_listed(kind, dim):
    w, keys = world_of(kind, dim), column()
    even = np.arange(N) % 2 == 0
    hix = ph.Hnsw.from_layers(w["store"], ring(np.arange(0, N, 2)))  # every second vector: vec2node is not the identity
    at = ph.Attribute(hix, values_of(np.where(keys == NONE, 0, keys)), missing=keys == NONE)
    listed = even & (keys != NONE)
    assert at.info() == (N, listed.sum(), keys[listed].min(), keys[listed].max())
    lo, hi = cycle_ranges()
    masks = rr.masks_of(keys, lo, hi)
    np.testing.assert_array_equal(at.count(values_of(lo), values_of(hi)), hix.filter_count(masks))
    np.testing.assert_array_equal(at.count(values_of(lo), values_of(hi)), rr.masks_of(keys, lo, hi, even).sum(1))
    got = check(w, at, lo, hi, members=even, hix=hix, k=100)
    for form in (0, 1):
        assert not (got[form][0][got[form][0] != EMPTY] % 2).any()
    head = np.arange(N) < N - 100
    hix2 = ph.Hnsw.from_layers(w["store"], ring(np.arange(N - 100)))  # the first N - 100: identity, shorter than the store
    at2 = ph.Attribute(hix2, values_of(np.where(keys == NONE, 0, keys)), missing=keys == NONE)
    assert at2.listed == (head & (keys != NONE)).sum()
    got = check(w, at2, lo, hi, members=head, hix=hix2, k=1024, device=False)
    assert (got[0][0][got[0][0] != EMPTY] < N - 100).all()


# ---------------------------------------------------------------- 5: refusals
def test_refusals():
    w, at = sworld("f32", 24), handle("f32", 24)
    hix, q = w["hix"], w["q"][:4]
    for k in (0, 1025):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_ranged(queries=q, attr=at, lo=0, hi=5, k=k)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_ranged: k must be 1..1024 (got %d)" % k
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_ranged_device(at, 4, k, 8, 8, 8, 8, qids=8, lo=8, hi=8)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_ranged_device: k must be 1..1024 (got %d)" % k
    # a handle made for another index over the same store: the wording of the labels
    other = ph.Hnsw.from_layers(w["store"], ring(np.arange(N)))
    for call in (lambda: other.search_exact_ranged(queries=q, attr=at, lo=0, hi=5, k=3),
                 lambda: other.search_exact_ranged_device(at, 4, 3, 8, 8, 8, 8, qids=8, lo=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        msg = str(e.value)
        assert e.value.code == -1 and "are stale: made for another index" in msg and "phnsw_search_exact_ranged" in msg
        assert "make a new handle" in msg
    with pytest.raises(ph.PhnswError) as e:  # the handle is looked at before the other arguments, k before the handle
        other.search_exact_ranged_device(at, 4, 0, 8, 8, 8, 8, qids=8, lo=8, hi=8)
    assert "k must be" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:
        other.search_exact_ranged_device(at, 4, 3, 8, 8, 8, 8)
    assert "stale" in str(e.value)
    for bad in (dict(queries=16, ldq=24, qids=8, lo=8, hi=8), dict(lo=8, hi=8), dict(qids=8, lo=8), dict(qids=8, hi=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_ranged_device(at, 4, 3, 8, 8, 8, 8, **bad)
        assert e.value.code == -1 and "phnsw_search_exact_ranged_device: invalid argument" in str(e.value)
    ids, d, ln = hix.search_exact_ranged(queries=np.zeros((0, 24), dtype=np.float32), attr=at, lo=0, hi=1, k=3)
    assert ids.shape == (0, 3)  # nq == 0: a no-op
    import ctypes as C
    out = C.c_void_p()
    col = column()
    assert ph.lib().phnsw_attr_create(hix._h, col.ctypes.data_as(C.c_void_p), N - 1, C.byref(out)) == -1
    msg = ph.lib().phnsw_last_error().decode()
    assert msg.startswith("phnsw_attr_create: %d keys for a store of %d vectors" % (N - 1, N)) and not out.value
    assert ph.lib().phnsw_attr_info(None, None, None, None, None) == -1
    ph.lib().phnsw_attr_destroy(None)  # a no-op


def test_a_handle_is_stale_after_the_store_has_grown():
    rows = oracle.synth_rows(0, 300, 24)[:, :24].copy()
    store = ph.VectorStore(rows[:200], metric=COS)
    hix = ph.Hnsw.from_layers(store, ring(np.arange(200)))
    val = (np.arange(200) * 7 % 50).astype(np.int32) - 25
    at = ph.Attribute(hix, val)
    lo, hi = np.array([-25, 0, 10], dtype=np.int32), np.array([-20, 0, 24], dtype=np.int32)
    allow = (val[None, :] >= lo[:, None]) & (val[None, :] <= hi[:, None])
    same(hix.search_exact_ranged(queries=rows[:3], attr=at, lo=lo, hi=hi, k=5), hix.search_exact_filtered(queries=rows[:3], allow=allow, k=5))
    store.append(rows[200:])
    with pytest.raises(ph.PhnswError) as e:
        hix.search_exact_ranged(queries=rows[:3], attr=at, lo=lo, hi=hi, k=5)
    assert e.value.code == -1 and "are stale: made for this index before it changed" in str(e.value)
    val2 = np.concatenate([val, np.zeros(100, dtype=np.int32)])
    at2 = ph.Attribute(hix, val2)  # a new handle: the appended vectors are not in the index, so they are not listed
    assert at2.listed == 200
    allow2 = np.concatenate([allow, np.ones((3, 100), dtype=bool)], axis=1)
    same(hix.search_exact_ranged(queries=rows[:3], attr=at2, lo=lo, hi=hi, k=5),
         hix.search_exact_filtered(queries=rows[:3], allow=allow2, k=5))


# ---------------------------------------------------------------- 6: value edges
VALUE_WORLDS = [("lattice", 0, 256, "f32"), ("lattice", 1, 256, "f32"), ("lattice", 2, 256, "f32"), ("l2_overflow", 2, 768, "f32"),
                ("tiny", 0, 100, "f16")]


@pytest.mark.parametrize("key", VALUE_WORLDS, ids=lambda k: "%s-m%d-d%d-%s" % k)
def test_value_edges_against_the_scan(monkeypatch, key):
    """ties (lattice, all three metrics), infinite distances (l2_overflow) and one tie over everything (tiny): the rows
    of search_exact_filtered for the equivalent bitmaps, and of the restatement over yardstick 1"""
    import filter_value_worlds as fw
    from test_gpu_filter_value_edges import queries_of, ring_index
    w, hix = fw.world(*key), ring_index(key)
    val = ((np.arange(fw.N) * 37) % fw.N).astype(np.float32) - 1000.0  # a permutation: spans are not in id order
    missing = np.arange(fw.N) % 50 == 0
    at = ph.Attribute(hix, val, missing=missing)
    for form in (0, 1):
        kw = queries_of(w, form)
        nq = len(next(iter(kw.values())))
        lo = (np.arange(nq) % 3 * 350.0 - 1000.0).astype(np.float32)  # spans of about 700 rows: eleven batches each
        hi = lo + np.float32(699.0)
        allow = ~missing[None, :] & (val[None, :] >= lo[:, None]) & (val[None, :] <= hi[:, None])
        for k in (10, 1024):
            ref = hix.search_exact_filtered(allow=allow, k=k, **kw)
            same(ref, xr.exact_topk((w["Dq"], w["Ds"])[form][:nq], allow, None, None, k))
            for env_kw in (dict(), dict(PHNSW_RANGE_SLICES="3")):
                with env(monkeypatch, **env_kw):
                    same(hix.search_exact_ranged(attr=at, lo=lo, hi=hi, k=k, **kw), ref)
