"""The exact radius search by row label (phnsw_search_exact_radius_labeled[_device], filter_list_radius.hip): per query
the listed rows of want[q] with d < radius[q], as CSR.  Every comparison is on offsets, ids and distance bits, no
tolerance anywhere.  World, yardsticks and the check: tests/list_radius_gpu.py.

The column gives lists of 0 (an absent label, NONE), 1, 63, 64, 65 and 1000 rows -- the last batch of a list empty,
partial and full -- and one of every other row; a second column lists every row under one label.  The 40 copies of row 0
are all in the list of 1000."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import filter_reference as fr
import list_radius_gpu as g
import list_radius_reference as lrr
import radius_reference as rr
from list_radius_gpu import DUPS, EMPTY, MS, N, NQX, STAGE, UP, ByLabel, check, radii_at
from test_gpu_exact_filter import COS, ring
from test_gpu_exact_labeled import world_of
from test_gpu_i8 import bits, oracle_over
from test_gpu_i8q import env
from test_gpu_radius_exact import same

pytestmark = pytest.mark.gpu

NONE, ABSENT = 0xFFFFFFFF, 77
L1, L63, L64, L65, L1000, REST, EVERY = 1, 2, 3, 4, 0x80000005, 9, 8
SIZES = ((L1, 1), (L63, 63), (L64, 64), (L65, 65), (L1000, 1000 - len(DUPS)), (NONE, 50))
KINDS = [("f32", 24, COS), ("f32", 256, COS), ("f16", 24, COS), ("i8", 24, COS), ("i8q", 24, COS), ("pq", 24, COS),
         ("f32", 24, oracle.METRIC_L2), ("f32", 24, oracle.METRIC_ONE_MINUS_DOT)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def column(name="lists"):
    """the label of every vector, u32 [N]"""
    if name == "every":
        lab = np.full(N, EVERY, dtype=np.uint32)
    else:
        lab = np.full(N, REST, dtype=np.uint32)
        others = np.random.default_rng(2025).permutation(np.setdiff1d(np.arange(N), DUPS))
        lab[DUPS] = L1000
        at = 0
        for value, count in SIZES:
            lab[others[at:at + count]] = value
            at += count
        assert (lab == L1000).sum() == 1000 and (lab == NONE).sum() == 50 and not (lab == ABSENT).any()
    lab.setflags(write=False)
    return lab


BY = {"lists": ByLabel(column()), "every": ByLabel(column("every"))}


@functools.lru_cache(maxsize=None)
def handle(kind, dim, metric=COS, name="lists"):
    return ph.Labels(world_of(kind, dim, metric)["hix"], column(name))


def cycle_want(nq=NQX):
    """query 0 (the duplicated row) wants the list of 1000 with the copies; the others go round every list"""
    values = [L1000, L1, L63, L64, L65, REST, ABSENT, NONE]
    return (np.array([values[i % len(values)] for i in range(nq)], dtype=np.int64),)


def test_the_lists_have_the_lengths_they_are_named_for():
    lb = handle("f32", 24)
    counts = lb.count(np.array([L1000, L1, L63, L64, L65, REST, ABSENT, -1]))
    assert counts.tolist() == [1000, 1, 63, 64, 65, N - 1243, 0, 0] and lb.longest == N - 1243
    assert handle("f32", 24, COS, "every").longest == N


# ---------------------------------------------------------------- 1: stores, radii, strictness
@pytest.mark.parametrize("kind,dim,metric", KINDS)
def test_radii_at_the_mth_smallest_distance_and_the_next_float_up(kind, dim, metric):
    w, lb, by = world_of(kind, dim, metric), handle(kind, dim, metric), BY["lists"]
    filt = cycle_want()
    first_kind = (kind, dim, metric) == KINDS[0]
    for shift in ((0, 1, 2, 3, 4, 5) if first_kind else (0, 3)):  # query q takes m = MS[(q // 8 + shift) % 6]: every list meets every m
        m = np.array([MS[(q // 8 + shift) % len(MS)] for q in range(NQX)])
        at = lambda D, masks: radii_at(D, masks, m)
        above = lambda D, masks: np.nextafter(radii_at(D, masks, m), UP)
        lo = check(by, w, lb, filt, at, bitmap=kind != "pq", device=shift == 0, topk=shift in (0, 3))
        hi = check(by, w, lb, filt, above, bitmap=kind != "pq" and shift == 0, device=shift == 3, topk=False)
        masks = by.masks(filt)
        for form in (0, 1):
            D = g.forms(w, NQX)[form][1]
            n_lo, n_hi = np.diff(lo[form][0].astype(np.int64)), np.diff(hi[form][0].astype(np.int64))
            have = masks.sum(axis=1) > 0
            r = at(D, masks)
            pos = have & (r > 0)
            assert (n_lo[pos] <= m[pos]).all() and (n_hi[pos] > np.minimum(m, masks.sum(axis=1) - 1)[pos]).all()  # strict
            assert not n_lo[~have].any() and not n_hi[~have].any() and not n_lo[have & ~(r > 0)].any()


@pytest.mark.parametrize("kind,dim", [("f32", 24), ("i8q", 24), ("pq", 24)])
def test_zero_negative_nan_and_infinite_radii(kind, dim):
    w, lb, by = world_of(kind, dim), handle(kind, dim), BY["lists"]
    filt = cycle_want(40)
    counts = by.masks(filt).sum(axis=1)
    for value in (0.0, -1.0, np.nan, -np.inf, -0.0):
        got = check(by, w, lb, filt, np.float32(value), nq=40, bitmap=kind != "pq", device=value == 0.0, topk=value == 0.0)
        for form in (0, 1):
            assert not got[form][0].any() and len(got[form][1]) == 0
    got = check(by, w, lb, filt, np.float32(np.inf), nq=40, bitmap=kind != "pq")
    for form in (0, 1):
        np.testing.assert_array_equal(np.diff(got[form][0].astype(np.int64)), counts)  # every listed row: all distances are finite
    mixed = np.tile(np.array([np.inf, 0.0, 0.3, np.nan, -1.0, 0.6, np.inf], dtype=np.float32), 6)[:40]  # all of them in one batch
    got = check(by, w, lb, filt, mixed, nq=40, bitmap=kind != "pq")
    n = np.diff(got[0][0].astype(np.int64))
    assert (n[0::7] == counts[0::7]).all() and not n[1::7].any() and not n[3::7].any() and not n[4::7].any()


def test_every_row_under_one_label_is_the_unfiltered_radius_call():
    w, lb, by = world_of("f32", 24), handle("f32", 24, COS, "every"), BY["every"]
    filt = (np.full(NQX, EVERY, dtype=np.int64),)
    m = np.array([MS[q % len(MS)] for q in range(NQX)])
    got = check(by, w, lb, filt, lambda D, masks: radii_at(D, masks, m))
    for form, (kw, D) in enumerate(g.forms(w, NQX)):
        same(got[form], w["hix"].search_exact_radius(radius=radii_at(D, np.ones((NQX, N), dtype=bool), m), **kw))


# ---------------------------------------------------------------- 2: slices
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("f32", 256), ("pq", 24)])
def test_the_result_does_not_depend_on_the_slices(monkeypatch, kind, dim):
    w, by = world_of(kind, dim), BY["lists"]
    for name, filt in (("lists", cycle_want()), ("every", (np.full(NQX, EVERY, dtype=np.int64),))):
        lb, by = handle(kind, dim, COS, name), BY[name]
        m = np.array([MS[(q // 8 + 1) % len(MS)] for q in range(NQX)])
        r = lambda D, masks: radii_at(D, masks, m)
        runs = {}
        for slices in ("1", "3", "16"):
            with env(monkeypatch, **{by.slices_knob: slices}):
                runs[slices] = check(by, w, lb, filt, r, bitmap=False, topk=False, device=slices != "3")
                counts = {f: by.count(w["hix"], lb, filt, radius=r(D, by.masks(filt)), **kw) for f, (kw, D) in enumerate(g.forms(w, NQX))}
            for form in (0, 1):  # byte for byte across the slice counts, the atomic counts of the slices included
                for a, b in zip(runs[slices][form], runs["1"][form]):
                    assert a.tobytes() == b.tobytes()
                assert counts[form].tobytes() == runs["1"][form][0].tobytes()


# ---------------------------------------------------------------- 3: the staging buffer
def test_lists_with_more_hits_than_the_staging_buffer_holds(monkeypatch):
    """one wave per query (one slice): 256 hits fill the buffer exactly and leave in the one flush at the end; 257 flush
    twice; 512, 1000 and every row at several multiples"""
    w, lb, by = world_of("f32", 24), handle("f32", 24, COS, "every"), BY["every"]
    filt = (np.full(16, EVERY, dtype=np.int64),)
    hits = np.array([STAGE, STAGE + 1, STAGE - 1, 2 * STAGE, 2 * STAGE + 1, 1000, 3 * STAGE + 64, N, 1, 0, STAGE, 4 * STAGE, 63, 64, 65, N])
    exact = 0
    for slices in ("1", "3"):
        with env(monkeypatch, PHNSW_LABEL_SLICES=slices):
            got = check(by, w, lb, filt, lambda D, masks: radii_at(D, masks, hits), nq=16, topk=slices == "1")
        for form in (0, 1):
            n = np.diff(got[form][0].astype(np.int64))
            D = g.forms(w, 16)[form][1]
            distinct = np.array([np.sort(D[q])[min(hits[q], N - 1) - 1] < np.sort(D[q])[min(hits[q], N - 1)] if 0 < hits[q] < N else True
                                 for q in range(16)])
            assert (n[distinct & (hits < N)] == hits[distinct & (hits < N)]).all()  # no tie at the cut: exactly m rows inside
            exact += int((n == STAGE).sum())
    assert exact >= 4  # a query with exactly one buffer's worth of hits, in each form and slice count


# ---------------------------------------------------------------- 4: capacity
def test_size_negotiation():
    w, lb, by = world_of("f32", 24), handle("f32", 24), BY["lists"]
    hix = w["hix"]
    filt = cycle_want(40)
    masks = by.masks(filt)
    for form in (0, 1):
        kw, D = g.forms(w, 40)[form]
        r = radii_at(D, masks, 30 + np.arange(40))
        ref = lrr.by_masks(D, r, masks)
        total = len(ref[1])
        assert total > 400
        first, t, ids, d = by.raw(hix, lb, filt, r, total, **kw)  # cap == total: filled
        assert t == total
        same((first, ids, d), ref)
        for cap in (total - 1, 1):  # too small: exact offsets and total, the arrays not touched
            first, t, ids, d = by.raw(hix, lb, filt, r, cap, **kw)
            assert t == total and (ids == 7).all() and (d == -1.0).all()
            np.testing.assert_array_equal(first, ref[0])
            dv, status, t, i_all, d_all = by.device(hix, lb, filt, r, cap, **kw)
            assert t == total and (i_all == 7).all() and (d_all == -1.0).all() and not status.any()
            np.testing.assert_array_equal(dv[0], ref[0])
        first, t, ids, d = by.raw(hix, lb, filt, r, total + 100000, **kw)  # room to spare: the tail untouched
        same((first, ids[:total], d[:total]), ref)
        assert (ids[total:] == 7).all() and (d[total:] == -1.0).all()
        first, t, _, _ = by.raw(hix, lb, filt, r, 0, null_arrays=True, **kw)  # counts only
        assert t == total
        np.testing.assert_array_equal(first, ref[0])
        dv, status, t, _, _ = by.device(hix, lb, filt, r, 0, null_arrays=True, **kw)
        assert t == total and not status.any()
        np.testing.assert_array_equal(dv[0], ref[0])
        dv, status, t, i_all, d_all = by.device(hix, lb, filt, r, 0, **kw)  # count only, arrays given: not touched
        assert t == total and (i_all == 7).all() and (d_all == -1.0).all()
        same(by.search(hix, lb, filt, radius=r, cap=5, **kw), ref)  # the method asks again, once


# ---------------------------------------------------------------- 5: exclude, copies, a bad stored id
def test_exclude_and_the_forty_copies():
    w, lb, by = world_of("f32", 24, oracle.METRIC_L2), handle("f32", 24, oracle.METRIC_L2), BY["lists"]
    filt = cycle_want()
    masks = by.masks(filt)
    inf = np.float32(np.inf)
    for form, (kw, D) in enumerate(g.forms(w, NQX)):
        got = check(by, w, lb, filt, inf, which=(form,))[form]
        si, sd = rr.segment(got, 0)  # equal rows are at exactly 0.0 under L2: the copies lead, in id order
        assert len(si) == 1000
        np.testing.assert_array_equal(si[:40], DUPS.astype(np.uint64))  # (stored query 0 is one of them: it finds itself too)
        assert len(set(bits(sd[:40]).tolist())) == 1
        # in turn: the query's best hit (inside the radius), a row outside its list, an id past n, EMPTY
        best = np.array([rr.segment(got, q)[0][0] if len(rr.segment(got, q)[0]) else EMPTY for q in range(NQX)], dtype=np.uint64)
        outside = np.array([np.nonzero(~masks[q])[0][5] for q in range(NQX)], dtype=np.uint64)
        ex = np.array([(best[q], outside[q], N + 7, EMPTY)[q % 4] for q in range(NQX)], dtype=np.uint64)
        now = check(by, w, lb, filt, inf, exclude=ex, which=(form,))[form]
        for q in range(NQX):
            a, b = rr.segment(got, q), rr.segment(now, q)
            if q % 4 == 0 and len(a[0]):
                np.testing.assert_array_equal(b[0], a[0][1:])
            else:
                np.testing.assert_array_equal(b[0], a[0])


@pytest.mark.parametrize("kind,dim", [("f32", 24), ("pq", 24)])
def test_a_stored_query_id_past_n_is_reported_and_harms_nobody(kind, dim):
    w, lb, by = world_of(kind, dim), handle(kind, dim), BY["lists"]
    nq = min(40, len(w["qids"]))
    filt = cycle_want(nq)
    masks = by.masks(filt)
    qids = w["qids"][:nq].copy()
    bad = [3, 17, nq - 1]
    qids[bad] = [N, N + 12345, 0xFFFFFFFE]
    r = radii_at(w["Ds"][:nq], masks, 25)
    dv, status, total, _, _ = by.device(w["hix"], lb, filt, r, nq * 26, qids=qids)
    rz = r.copy()
    rz[bad] = 0.0  # the reference: those three match nothing
    ref = lrr.by_masks(w["Ds"][:nq], rz, masks)
    same(dv, ref)
    good = np.setdiff1d(np.arange(nq), bad)
    assert total == len(ref[1]) > 0 and (status[bad] == 4).all() and not status[good].any()
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses it, by name
        w["hix"].search_exact_radius_labeled(qids=qids.astype(np.uint64), labels=lb, want=filt[0], radius=r)
    assert e.value.code == -1 and str(e.value).startswith("phnsw error -1: phnsw_search_exact_radius_labeled: stored query id")


# ---------------------------------------------------------------- 6: refusals, in the documented order
def test_refusals_in_the_documented_order():
    w, lb, by = world_of("f32", 24), handle("f32", 24), BY["lists"]
    hix, q = w["hix"], w["q"][:4]
    want = np.array([L1000, L1, ABSENT, NONE])
    host = "phnsw_search_exact_radius_labeled"
    other = ph.Hnsw.from_layers(w["store"], ring(np.arange(N)))  # the handle was made for another index
    # cap before the handle, the handle before the store, the pointers and nq
    with pytest.raises(ph.PhnswError) as e:
        by.raw(other, lb, (want,), 1.0, 1 << 31, queries=q)
    assert str(e.value) == "phnsw error -1: %s: cap must be at most 2^31 - 1 (got 2147483648)" % host
    with pytest.raises(ph.PhnswError) as e:
        other.search_exact_radius_labeled_device(lb, 4, 8, 1 << 31, 8, 8, 8, 8, 8, qids=8, want=8)
    assert str(e.value) == "phnsw error -1: %s_device: cap must be at most 2^31 - 1 (got 2147483648)" % host
    for call in (lambda: other.search_exact_radius_labeled(queries=q, labels=lb, want=want, radius=1.0),
                 lambda: other.search_exact_radius_labeled(queries=q[:0], labels=lb, want=want[:0], radius=1.0),  # before nq == 0
                 lambda: other.search_exact_radius_labeled_device(lb, 4, 8, 3, 8, 8, 8, 8, 8),                     # before the pointers
                 lambda: other.search_exact_radius_labeled_device(lb, 0, 0, 0, 0, 0, 0, 0, 0)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == -1 and "the labels are stale" in str(e.value) and "made for another index" in str(e.value)
        assert host in str(e.value)
    # nq == 0: the host form writes the empty result, the device form enqueues nothing and looks at no pointer
    first, ids, d = hix.search_exact_radius_labeled(queries=q[:0], labels=lb, want=want[:0], radius=1.0)
    assert first.tolist() == [0] and len(ids) == 0 and len(d) == 0
    hix.search_exact_radius_labeled_device(lb, 0, 0, 0, 0, 0, 0, 0, 0)
    # the pointers: both and neither of queries / qids, no want, no radius, no out_first, cap without arrays
    for bad in (dict(queries=16, ldq=24, qids=8, want=8), dict(want=8), dict(qids=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_radius_labeled_device(lb, 4, 8, 3, 8, 8, 8, 8, 8, **bad)
        assert e.value.code == -1 and "%s_device: invalid argument" % host in str(e.value)
    for args in ((4, 0, 3, 8, 8, 8, 8, 8), (4, 8, 3, 0, 8, 8, 8, 8), (4, 8, 3, 8, 0, 0, 8, 8), (4, 8, 3, 8, 8, 8, 0, 8), (4, 8, 3, 8, 8, 8, 8, 0)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_radius_labeled_device(lb, *args, qids=8, want=8)
        assert e.value.code == -1 and "%s_device: invalid argument" % host in str(e.value)
    with pytest.raises(ValueError):
        hix.search_exact_radius_labeled(queries=q, qids=w["qids"][:4], labels=lb, want=want, radius=1.0)
    with pytest.raises(ValueError):
        hix.search_exact_radius_labeled(queries=q, labels=lb, want=want)
    # a stale handle: the store has grown
    rows = oracle.synth_rows(0, 300, 24)[:, :24].copy()
    store = ph.VectorStore(rows[:200], metric=COS)
    six = ph.Hnsw.from_layers(store, ring(np.arange(200)))
    slb = ph.Labels(six, np.arange(200) % 4)
    first, ids, d = six.search_exact_radius_labeled(queries=rows[:3], labels=slb, want=np.array([0, 1, 2]), radius=np.inf)
    assert np.diff(first.astype(np.int64)).tolist() == [50, 50, 50]
    store.append(rows[200:])
    with pytest.raises(ph.PhnswError) as e:
        six.search_exact_radius_labeled(queries=rows[:3], labels=slb, want=np.array([0, 1, 2]), radius=np.inf)
    assert e.value.code == -1 and "the labels are stale" in str(e.value) and "before it changed" in str(e.value)
    # a shared-codebook PQ store and rows above 1536 floats: unsupported, after the handle
    r32 = oracle.synth_rows(0, 400, 32)[:, :32].copy()
    f2 = ph.VectorStore(r32, metric=ph.METRIC_L2)
    shared = ph.SharedPqStore(f2, 16, 100, seed=3, centroid_bp=ph.BuildParameters(seed=2), quantized_search=ph.SearchParameters(32, 32, 2))
    long_rows = ph.VectorStore(oracle.synth_rows(0, 64, 1540)[:, :1540].copy(), metric=ph.METRIC_L2)
    for store, n, dim in ((shared, 400, 32), (long_rows, 64, 1540)):
        pix = ph.Hnsw.from_layers(store, ring(np.arange(n)))
        plb = ph.Labels(pix, np.arange(n) % 3)
        with pytest.raises(ph.PhnswError) as e:
            pix.search_exact_radius_labeled(queries=np.zeros((2, dim), dtype=np.float32), labels=plb, want=np.array([0, 1]), radius=1.0)
        assert e.value.code == -7 and host + ":" in str(e.value)  # PHNSW_E_UNSUPPORTED
        with pytest.raises(ph.PhnswError) as e:
            pix.search_exact_radius_labeled_device(plb, 2, 8, 3, 8, 8, 8, 8, 8, qids=8, want=8)
        assert e.value.code == -7 and host + "_device:" in str(e.value)
        with pytest.raises(ph.PhnswError) as e:  # the handle before the store
            pix.search_exact_radius_labeled_device(lb, 2, 8, 3, 8, 8, 8, 8, 8, qids=8, want=8)
        assert e.value.code == -1 and "stale" in str(e.value)


# ---------------------------------------------------------------- 7: two streams, one handle
def test_two_calls_on_two_streams_with_one_handle():
    import torch
    w, lb, by = world_of("f32", 256), handle("f32", 256), BY["lists"]
    hix = w["hix"]
    filt = cycle_want()
    masks = by.masks(filt)
    calls = []
    for i, (kw, D) in enumerate(g.forms(w, NQX)):
        r = radii_at(D, masks, 40 + 300 * i)
        ref = lrr.by_masks(D, r, masks)
        alone = by.device(hix, lb, filt, r, len(ref[1]), **kw)
        same(alone[0], ref)
        calls.append((kw, r, ref))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(3):  # in flight together, nothing between them
        fetch = [by.device(hix, lb, filt, r, len(ref[1]), stream=s, sync=False, **kw) for (kw, r, ref), s in zip(calls, streams)]
        for f, (kw, r, ref) in zip(fetch, calls):
            dv, status, total, _, _ = f()
            assert not status.any() and total == len(ref[1])
            same(dv, ref)


def test_calls_from_two_threads_whose_scratch_grows():
    """two host threads, a stream each, one handle: every thread's calls alternate between a small batch with a cap of 1
    and the whole batch with room for everything, so the blocks of its scratch set grow again and again while the other
    thread's calls are queued.  A block is sized once per call, before anything of the call is enqueued; a block that went
    back to the pool under a queued sort would give another call's bytes to it"""
    import threading
    import torch
    w, by = world_of("f32", 24), BY["lists"]
    hix, lb = w["hix"], ph.Labels(w["hix"], column())  # a fresh handle: no scratch set yet
    filt = cycle_want()
    masks = by.masks(filt)
    jobs = []
    for i, (kw, D) in enumerate(g.forms(w, NQX)):
        r = radii_at(D, masks, 900)
        jobs.append((kw, r, lrr.by_masks(D, r, masks), lrr.by_masks(D[:3], r[:3], masks[:3])))
    errors = []

    def work(job, stream):
        try:
            kw, r, ref, ref3 = job
            for n in range(6):
                small = {k: v[:3] for k, v in kw.items()}
                dv, status, total, i_all, _ = by.device(hix, lb, by.take(filt, np.arange(3)), r[:3], 1, stream=stream, **small)
                assert total == len(ref3[1]) > 1 and (i_all == 7).all() and not status.any()
                np.testing.assert_array_equal(dv[0], ref3[0])
                dv, status, total, _, _ = by.device(hix, lb, filt, r, len(ref[1]) + 1000 * n, stream=stream, **kw)
                assert total == len(ref[1]) and not status.any()
                same(dv, ref)
        except BaseException as e:  # noqa: B902 -- handed to the test's thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(job, torch.cuda.Stream())) for job in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    lb.close()
    if errors:
        raise errors[0]


# ---------------------------------------------------------------- 8: more work items than the grid has blocks
def test_more_items_than_blocks_at_70_001_rows(monkeypatch):
    """the world of tests/test_gpu_labeled_scale.py: 70 001 rows; every row a Stored query, 16 forced slices: 1 120 016
    items > 2^20 blocks, so 71 440 blocks take a second item.  Rows of a small list want their own label, the rows of the
    list of 25 040 want an absent one (so the lists are short and the test runs in seconds) but for 200 of them, which
    scan all 16 slices of it.  Counts for every query, whole segments for a sample, against the restatement"""
    import test_gpu_labeled_scale as ts
    w, lab, lb = ts.world("f32", 24), ts.col("mix"), ts.handle("f32", "mix")
    hix, n = w["hix"], ts.N
    big = ts.mix()[1]["big"]
    qids = np.arange(n, dtype=np.uint64)
    want = lab.astype(np.int64).copy()
    in_big = np.nonzero(lab == big)[0]
    want[in_big[200:]] = 5_000_000_00  # nobody carries it
    assert lb.count([5_000_000_00])[0] == 0 and lb.longest == 25040 and n * 16 > 2 ** 20
    sizes = lb.count(want).astype(np.int64)
    assert (sizes[in_big[:200]] == 25040).all() and sizes.sum() < 12_000_000
    by = ByLabel(lab)
    with env(monkeypatch, PHNSW_LABEL_SLICES="16"):
        first, ids, d = by.search(hix, lb, (want,), qids=qids, radius=np.float32(np.inf), cap=int(sizes.sum()))
        counts = by.count(hix, lb, (want,), qids=qids, radius=np.float32(np.inf))
    np.testing.assert_array_equal(first, counts)
    np.testing.assert_array_equal(np.diff(first.astype(np.int64)), sizes)  # every listed row is at a finite distance
    rng = np.random.default_rng(8)
    sample = np.unique(np.concatenate([in_big[:3], rng.integers(0, n, 60), np.arange(n - 5, n), ts.DUPS[:3]]))
    D = fr.distance_rows(oracle_over(w["store"], COS), qids=sample.astype(np.uint64), mode=oracle.SUM_BLOCKED64)
    ref = lrr.exact_radius_labeled(D, np.float32(np.inf), lab.astype(np.int64) & 0xFFFFFFFF, want[sample])
    for j, q in enumerate(sample):
        a, b = rr.segment((first, ids, d), int(q)), rr.segment(ref, j)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(bits(a[1]), bits(b[1]))


# ---------------------------------------------------------------- 9: the C++ mirror
def test_cpp_mirror_compiles_and_runs(tmp_path):
    exe = str(tmp_path / "test_radius_labeled_shim")
    libdir = os.path.join(ROOT, "parallel_hnsw_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_radius_labeled_shim.cpp"), "-o", exe, "-L", libdir, "-lphnsw",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
