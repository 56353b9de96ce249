"""The exact radius search by a numeric range (phnsw_search_exact_radius_ranged[_device], filter_list_radius.hip): per
query the listed rows with lo[q] <= key <= hi[q] and d < radius[q], as CSR.  Every comparison is on offsets, ids and
distance bits, no tolerance anywhere.  World, yardsticks and the check: tests/list_radius_gpu.py.

The key column has ties (runs of 2 to 5 rows per key) and 50 rows without a value; the windows select spans of 0, 1, 63,
64, 65, 1000 rows and every listed row -- the last batch of a span empty, partial and full -- plus lo > hi,
hi = 0xFFFFFFFF and a window that could select only rows without a value.  The 40 copies of row 0 are in the span of 1000."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import list_radius_gpu as g
import list_radius_reference as lrr
import radius_reference as rr
from list_radius_gpu import DUPS, EMPTY, MS, N, NQX, UP, ByRange, check, radii_at
from test_gpu_exact_filter import COS, ring
from test_gpu_exact_labeled import world_of
from test_gpu_i8q import env
from test_gpu_radius_exact import same

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
KINDS = [("f32", 24, COS), ("f32", 256, COS), ("f16", 24, COS), ("i8", 24, COS), ("i8q", 24, COS), ("pq", 24, COS),
         ("f32", 24, oracle.METRIC_L2), ("f32", 24, oracle.METRIC_ONE_MINUS_DOT)]
# (lo, hi, rows): the windows, by what they select
WINDOWS = [(1000, 1249, 1000), (10, 10, 1), (20, 40, 63), (100, 131, 64), (200, 212, 65), (0, NONE, N - 50), (5000, NONE, N - 1243),
           (50, 40, 0), (NONE - 1, NONE, 0), (41, 99, 0), (0, 9, 0), (20, 131, 127), (1249, 5000, 4 + 3)]


@functools.lru_cache(maxsize=None)
def column():
    """the key of every vector, u32 [N]; NONE = no value"""
    keys = np.full(N, NONE, dtype=np.uint32)
    others = np.random.default_rng(2026).permutation(np.setdiff1d(np.arange(N), DUPS))
    at = 0
    for base, count, run in ((10, 1, 1), (20, 63, 3), (100, 64, 2), (200, 65, 5), (1000, 1000 - len(DUPS), 4)):
        keys[others[at:at + count]] = base + np.arange(count) // run
        at += count
    keys[DUPS] = 1000 + (1000 - len(DUPS) + np.arange(len(DUPS))) // 4  # the last ten keys of the span of 1000
    at += 50  # fifty rows without a value
    rest = others[at:]
    keys[rest] = 5000 + np.arange(len(rest)) // 3
    assert (keys == NONE).sum() == 50 and keys[DUPS].max() == 1249
    keys.setflags(write=False)
    return keys


BY = ByRange(column())


@functools.lru_cache(maxsize=None)
def handle(kind, dim, metric=COS):
    keys = column()
    return ph.Attribute(world_of(kind, dim, metric)["hix"], keys, missing=keys == NONE)


def cycle_windows(nq=NQX):
    """query 0 (the duplicated row) takes the span of 1000 with the copies; the others go round every window"""
    w = [WINDOWS[i % len(WINDOWS)] for i in range(nq)]
    return np.array([x[0] for x in w], dtype=np.uint32), np.array([x[1] for x in w], dtype=np.uint32)


def test_the_windows_hold_the_rows_they_are_named_for():
    at = handle("f32", 24)
    lo, hi = np.array([x[0] for x in WINDOWS], dtype=np.uint32), np.array([x[1] for x in WINDOWS], dtype=np.uint32)
    assert at.count(**{k: v for k, v in BY.kw(at, (lo, hi)).items() if k != "attr"}).tolist() == [x[2] for x in WINDOWS] == BY.masks((lo, hi)).sum(axis=1).tolist()
    assert at.listed == N - 50


# ---------------------------------------------------------------- 1: stores, radii, strictness
@pytest.mark.parametrize("kind,dim,metric", KINDS)
def test_radii_at_the_mth_smallest_distance_and_the_next_float_up(kind, dim, metric):
    w, at = world_of(kind, dim, metric), handle(kind, dim, metric)
    filt = cycle_windows()
    masks = BY.masks(filt)
    for shift in ((0, 1, 2, 3, 4, 5) if (kind, dim, metric) == KINDS[0] else (0, 3)):
        m = np.array([MS[(q // len(WINDOWS) + q + shift) % len(MS)] for q in range(NQX)])
        r_at = lambda D, masks: radii_at(D, masks, m)
        above = lambda D, masks: np.nextafter(radii_at(D, masks, m), UP)
        lo = check(BY, w, at, filt, r_at, bitmap=kind != "pq", device=shift == 0, topk=shift in (0, 3))
        hi = check(BY, w, at, filt, above, bitmap=kind != "pq" and shift == 0, device=shift == 3, topk=False)
        for form in (0, 1):
            D = g.forms(w, NQX)[form][1]
            n_lo, n_hi = np.diff(lo[form][0].astype(np.int64)), np.diff(hi[form][0].astype(np.int64))
            have = masks.sum(axis=1) > 0
            pos = have & (r_at(D, masks) > 0)
            assert (n_lo[pos] <= m[pos]).all() and (n_hi[pos] > np.minimum(m, masks.sum(axis=1) - 1)[pos]).all()  # strict
            assert not n_lo[~have].any() and not n_hi[~have].any()


@pytest.mark.parametrize("kind,dim", [("f32", 24), ("i8q", 24)])
def test_zero_negative_nan_and_infinite_radii_and_the_edge_windows(kind, dim):
    w, at = world_of(kind, dim), handle(kind, dim)
    filt = cycle_windows(39)
    counts = BY.masks(filt).sum(axis=1)
    assert counts.tolist() == [WINDOWS[i % len(WINDOWS)][2] for i in range(39)]
    for value in (0.0, -1.0, np.nan, -np.inf, -0.0):
        got = check(BY, w, at, filt, np.float32(value), nq=39, device=value == 0.0, topk=value == 0.0)
        for form in (0, 1):
            assert not got[form][0].any() and len(got[form][1]) == 0
    got = check(BY, w, at, filt, np.float32(np.inf), nq=39)
    for form in (0, 1):  # lo > hi, a window of rows without a value and gaps: empty; hi = 0xFFFFFFFF: no such row passes
        np.testing.assert_array_equal(np.diff(got[form][0].astype(np.int64)), counts)
        assert not np.isin(got[form][1], np.nonzero(column() == NONE)[0].astype(np.uint64)).any()
    # lo = hi = 0xFFFFFFFF, which only the C calls take: the key of a row without a value selects nothing
    none = (np.full(4, NONE, dtype=np.uint32), np.full(4, NONE, dtype=np.uint32))
    first, total, _, _ = BY.raw(w["hix"], at, none, np.inf, 16, queries=w["q"][:4])
    dv, status, dtotal, _, _ = BY.device(w["hix"], at, none, np.inf, 16, qids=w["qids"][:4])
    assert total == dtotal == 0 and not first.any() and not dv[0].any() and not status.any()
    mixed = np.tile(np.array([np.inf, 0.0, 0.3, np.nan, -1.0, 0.6, np.inf], dtype=np.float32), 6)[:39]
    got = check(BY, w, at, filt, mixed, nq=39)
    n = np.diff(got[0][0].astype(np.int64))
    assert (n[0::7] == counts[0::7]).all() and not n[1::7].any() and not n[3::7].any() and not n[4::7].any()


# ---------------------------------------------------------------- 2: slices
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("pq", 24)])
def test_the_result_does_not_depend_on_the_slices(monkeypatch, kind, dim):
    w, at = world_of(kind, dim), handle(kind, dim)
    filt = cycle_windows()
    m = np.array([MS[(q // len(WINDOWS) + q + 1) % len(MS)] for q in range(NQX)])
    r = lambda D, masks: radii_at(D, masks, m)
    runs = {}
    for slices in ("1", "3", "16"):
        with env(monkeypatch, PHNSW_RANGE_SLICES=slices):
            runs[slices] = check(BY, w, at, filt, r, bitmap=False, topk=False, device=slices != "3")
            counts = {f: BY.count(w["hix"], at, filt, radius=r(D, BY.masks(filt)), **kw) for f, (kw, D) in enumerate(g.forms(w, NQX))}
        for form in (0, 1):  # byte for byte across the slice counts, the atomic counts of the slices included
            for a, b in zip(runs[slices][form], runs["1"][form]):
                assert a.tobytes() == b.tobytes()
            assert counts[form].tobytes() == runs["1"][form][0].tobytes()


# ---------------------------------------------------------------- 3: capacity
def test_size_negotiation():
    w, at = world_of("f32", 24), handle("f32", 24)
    hix = w["hix"]
    filt = cycle_windows(39)
    masks = BY.masks(filt)
    for form in (0, 1):
        kw, D = g.forms(w, 39)[form]
        r = radii_at(D, masks, 30 + np.arange(39))
        ref = lrr.by_masks(D, r, masks)
        total = len(ref[1])
        assert total > 400
        first, t, ids, d = BY.raw(hix, at, filt, r, total, **kw)  # cap == total: filled
        assert t == total
        same((first, ids, d), ref)
        for cap in (total - 1, 1):  # too small: exact offsets and total, the arrays not touched
            first, t, ids, d = BY.raw(hix, at, filt, r, cap, **kw)
            assert t == total and (ids == 7).all() and (d == -1.0).all()
            np.testing.assert_array_equal(first, ref[0])
            dv, status, t, i_all, d_all = BY.device(hix, at, filt, r, cap, **kw)
            assert t == total and (i_all == 7).all() and (d_all == -1.0).all() and not status.any()
            np.testing.assert_array_equal(dv[0], ref[0])
        first, t, ids, d = BY.raw(hix, at, filt, r, total + 100000, **kw)  # room to spare: the tail untouched
        same((first, ids[:total], d[:total]), ref)
        assert (ids[total:] == 7).all() and (d[total:] == -1.0).all()
        first, t, _, _ = BY.raw(hix, at, filt, r, 0, null_arrays=True, **kw)  # counts only
        assert t == total
        np.testing.assert_array_equal(first, ref[0])
        dv, status, t, i_all, d_all = BY.device(hix, at, filt, r, 0, **kw)  # count only, arrays given: not touched
        assert t == total and (i_all == 7).all() and (d_all == -1.0).all() and not status.any()
        np.testing.assert_array_equal(dv[0], ref[0])
        same(BY.search(hix, at, filt, radius=r, cap=5, **kw), ref)  # the method asks again, once


# ---------------------------------------------------------------- 4: exclude, copies, a bad stored id
def test_exclude_and_the_forty_copies():
    w, at = world_of("f32", 24, oracle.METRIC_L2), handle("f32", 24, oracle.METRIC_L2)
    filt = cycle_windows()
    masks = BY.masks(filt)
    inf = np.float32(np.inf)
    for form in (0, 1):
        got = check(BY, w, at, filt, inf, which=(form,))[form]
        si, sd = rr.segment(got, 0)  # equal rows are at exactly 0.0 under L2: the copies lead, in id order
        assert len(si) == 1000
        np.testing.assert_array_equal(si[:40], DUPS.astype(np.uint64))
        assert len(set(sd[:40].view(np.uint32).tolist())) == 1
        best = np.array([rr.segment(got, q)[0][0] if len(rr.segment(got, q)[0]) else EMPTY for q in range(NQX)], dtype=np.uint64)
        outside = np.array([np.nonzero(~masks[q])[0][5] for q in range(NQX)], dtype=np.uint64)
        ex = np.array([(best[q], outside[q], N + 7, EMPTY)[q % 4] for q in range(NQX)], dtype=np.uint64)
        now = check(BY, w, at, filt, inf, exclude=ex, which=(form,))[form]
        for q in range(NQX):
            a, b = rr.segment(got, q), rr.segment(now, q)
            np.testing.assert_array_equal(b[0], a[0][1:] if q % 4 == 0 and len(a[0]) else a[0])


def test_a_stored_query_id_past_n_is_reported_and_harms_nobody():
    w, at = world_of("f32", 24), handle("f32", 24)
    filt = cycle_windows(40)
    masks = BY.masks(filt)
    qids = w["qids"][:40].copy()
    bad = [3, 17, 39]
    qids[bad] = [N, N + 12345, 0xFFFFFFFE]
    r = radii_at(w["Ds"][:40], masks, 25)
    dv, status, total, _, _ = BY.device(w["hix"], at, filt, r, 40 * 26, qids=qids)
    rz = r.copy()
    rz[bad] = 0.0  # the reference: those three match nothing
    ref = lrr.by_masks(w["Ds"][:40], rz, masks)
    same(dv, ref)
    good = np.setdiff1d(np.arange(40), bad)
    assert total == len(ref[1]) > 0 and (status[bad] == 4).all() and not status[good].any()
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses it, by name
        w["hix"].search_exact_radius_ranged(qids=qids.astype(np.uint64), radius=r, **BY.kw(at, filt))
    assert e.value.code == -1 and str(e.value).startswith("phnsw error -1: phnsw_search_exact_radius_ranged: stored query id")


# ---------------------------------------------------------------- 5: refusals, in the documented order
def test_refusals_in_the_documented_order():
    w, at = world_of("f32", 24), handle("f32", 24)
    hix, q = w["hix"], w["q"][:4]
    lo, hi = np.array([0, 10, 50, 1000], dtype=np.uint32), np.array([NONE - 1, 10, 40, 1249], dtype=np.uint32)
    host = "phnsw_search_exact_radius_ranged"
    other = ph.Hnsw.from_layers(w["store"], ring(np.arange(N)))  # the handle was made for another index
    with pytest.raises(ph.PhnswError) as e:  # cap before the handle
        BY.raw(other, at, (lo, hi), 1.0, 1 << 31, queries=q)
    assert str(e.value) == "phnsw error -1: %s: cap must be at most 2^31 - 1 (got 2147483648)" % host
    with pytest.raises(ph.PhnswError) as e:
        other.search_exact_radius_ranged_device(at, 4, 8, 1 << 31, 8, 8, 8, 8, 8, qids=8, lo=8, hi=8)
    assert str(e.value) == "phnsw error -1: %s_device: cap must be at most 2^31 - 1 (got 2147483648)" % host
    for call in (lambda: other.search_exact_radius_ranged(queries=q, attr=at, lo=lo, hi=hi, radius=1.0),
                 lambda: other.search_exact_radius_ranged(queries=q[:0], attr=at, lo=lo[:0], hi=hi[:0], radius=1.0),  # before nq == 0
                 lambda: other.search_exact_radius_ranged_device(at, 4, 8, 3, 8, 8, 8, 8, 8)):                         # before the pointers
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == -1 and "the attribute keys are stale" in str(e.value) and host in str(e.value)
    first, ids, d = hix.search_exact_radius_ranged(queries=q[:0], attr=at, lo=lo[:0], hi=hi[:0], radius=1.0)  # nq == 0
    assert first.tolist() == [0] and len(ids) == 0 and len(d) == 0
    hix.search_exact_radius_ranged_device(at, 0, 0, 0, 0, 0, 0, 0, 0)
    for bad in (dict(queries=16, ldq=24, qids=8, lo=8, hi=8), dict(lo=8, hi=8), dict(qids=8, hi=8), dict(qids=8, lo=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_radius_ranged_device(at, 4, 8, 3, 8, 8, 8, 8, 8, **bad)
        assert e.value.code == -1 and "%s_device: invalid argument" % host in str(e.value)
    for args in ((4, 0, 3, 8, 8, 8, 8, 8), (4, 8, 3, 0, 8, 8, 8, 8), (4, 8, 3, 8, 0, 0, 8, 8), (4, 8, 3, 8, 8, 8, 0, 8), (4, 8, 3, 8, 8, 8, 8, 0)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_radius_ranged_device(at, *args, qids=8, lo=8, hi=8)
        assert e.value.code == -1 and "%s_device: invalid argument" % host in str(e.value)
    rows = oracle.synth_rows(0, 300, 24)[:, :24].copy()  # a stale handle: the store has grown
    store = ph.VectorStore(rows[:200], metric=COS)
    six = ph.Hnsw.from_layers(store, ring(np.arange(200)))
    sat = ph.Attribute(six, (np.arange(200) % 4).astype(np.uint32))
    first, ids, d = six.search_exact_radius_ranged(queries=rows[:3], attr=sat, lo=np.uint32(1), hi=np.uint32(2), radius=np.inf)
    assert np.diff(first.astype(np.int64)).tolist() == [100, 100, 100]
    store.append(rows[200:])
    with pytest.raises(ph.PhnswError) as e:
        six.search_exact_radius_ranged(queries=rows[:3], attr=sat, lo=np.uint32(1), hi=np.uint32(2), radius=np.inf)
    assert e.value.code == -1 and "stale" in str(e.value) and "before it changed" in str(e.value)
    r32 = oracle.synth_rows(0, 400, 32)[:, :32].copy()  # unsupported stores, after the handle
    f2 = ph.VectorStore(r32, metric=ph.METRIC_L2)
    shared = ph.SharedPqStore(f2, 16, 100, seed=3, centroid_bp=ph.BuildParameters(seed=2), quantized_search=ph.SearchParameters(32, 32, 2))
    long_rows = ph.VectorStore(oracle.synth_rows(0, 64, 1540)[:, :1540].copy(), metric=ph.METRIC_L2)
    for store, n, dim in ((shared, 400, 32), (long_rows, 64, 1540)):
        pix = ph.Hnsw.from_layers(store, ring(np.arange(n)))
        pat = ph.Attribute(pix, (np.arange(n) % 3).astype(np.uint32))
        with pytest.raises(ph.PhnswError) as e:
            pix.search_exact_radius_ranged(queries=np.zeros((2, dim), dtype=np.float32), attr=pat, lo=np.uint32(0), hi=np.uint32(1), radius=1.0)
        assert e.value.code == -7 and host + ":" in str(e.value)  # PHNSW_E_UNSUPPORTED
        with pytest.raises(ph.PhnswError) as e:
            pix.search_exact_radius_ranged_device(pat, 2, 8, 3, 8, 8, 8, 8, 8, qids=8, lo=8, hi=8)
        assert e.value.code == -7 and host + "_device:" in str(e.value)
        with pytest.raises(ph.PhnswError) as e:  # the handle before the store
            pix.search_exact_radius_ranged_device(at, 2, 8, 3, 8, 8, 8, 8, 8, qids=8, lo=8, hi=8)
        assert e.value.code == -1 and "stale" in str(e.value)


# ---------------------------------------------------------------- 6: two streams, one handle
def test_two_calls_on_two_streams_with_one_handle():
    import torch
    w, at = world_of("f32", 256), handle("f32", 256)
    hix = w["hix"]
    filt = cycle_windows()
    masks = BY.masks(filt)
    calls = []
    for i, (kw, D) in enumerate(g.forms(w, NQX)):
        r = radii_at(D, masks, 40 + 300 * i)
        ref = lrr.by_masks(D, r, masks)
        same(BY.device(hix, at, filt, r, len(ref[1]), **kw)[0], ref)
        calls.append((kw, r, ref))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(3):  # in flight together, nothing between them
        fetch = [BY.device(hix, at, filt, r, len(ref[1]), stream=s, sync=False, **kw) for (kw, r, ref), s in zip(calls, streams)]
        for f, (kw, r, ref) in zip(fetch, calls):
            dv, status, total, _, _ = f()
            assert not status.any() and total == len(ref[1])
            same(dv, ref)
