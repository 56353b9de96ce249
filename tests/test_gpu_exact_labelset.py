"""The exact top-k by a SET of row labels (phnsw_labels_count_set_device, phnsw_search_exact_labelset[_device]): the
machinery of the label scan over (query, wanted label) pairs.  Every comparison is on ids, distance bits, lengths and
status, no tolerance anywhere.

Two yardsticks, both for every case: tests/exact_filter_reference.py over the oracle's distances with the bitmaps
labelset_reference.masks_of_sets makes of the label column, and the existing scan, search_exact_filtered with those masks
as per-query bitmaps, whose rows the new call promises bit for bit.

The worlds, the label column (lists of exactly 1, 64 and 65 rows, BIG with 2140 rows in 34 batches and the 40 copies of
row 0, 100 unlabelled rows) and the helpers are those of tests/test_gpu_exact_labeled.py."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import filter_reference as fr
import labeled_reference as lr
import labeled_scale_reference as ls
import labelset_reference as sr
from test_gpu_exact_filter import COS, DUPS, EMPTY, N, ring, same
from test_gpu_exact_labeled import (ABSENT, BIG, HALF, KINDS, L64, L65, NONE, ONE, REST, TOP, column, device_labeled, handle,
                                    world_of)
from test_gpu_exact_shared import NQX, fetch, sworld
from test_gpu_i8 import bits, oracle_over
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

ALL13 = [BIG, ONE, L64, L65, HALF, TOP, ABSENT, NONE] + list(REST)
SHAPES = [[], [ONE], [L64, L65], [L64, L64, ONE], [ABSENT, NONE], [BIG, ABSENT, L65, NONE, BIG], ALL13, list(REST)]
ST_RANGE = 8  # status of a query whose range of want_first is not sound


def cycle_sets(nq=NQX):
    """query 0 (the duplicated row) wants [BIG, L65]; the others go round every shape of a set"""
    sets = [list(SHAPES[i % len(SHAPES)]) for i in range(nq)]
    sets[0] = [BIG, L65]
    return sets


def staged_labelset(hix, lb, k, first, values, nwant=None, queries=None, qids=None, exclude=None):
    """the inputs and outputs of one phnsw_search_exact_labelset_device call, uploaded; no synchronisation here.  first
    and values go up as they are (u32), so a test can send offsets the host form would refuse.  Returns (launch, out):
    launch(stream) enqueues the call and nothing else, out is what fetch takes"""
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
    first = np.asarray(first, dtype=np.uint32)
    values = np.asarray(values, dtype=np.uint32)
    nwant = len(values) if nwant is None else nwant
    assert len(first) == nq + 1 and nwant <= len(values)
    fd = up(first, np.int32).data_ptr()
    vd = up(values, np.int32).data_ptr() if len(values) else 0
    ids = torch.full((nq, k), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev)
    ln = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    status = torch.full((nq,), -1, dtype=torch.int32, device=dev)

    def launch(stream=None):
        hix.search_exact_labelset_device(lb, nq, nwant, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(),
                                         queries=qd, ldq=ld, qids=qi, exclude=ex, want_first=fd, want_values=vd,
                                         stream=0 if stream is None else stream.cuda_stream)

    return launch, (ids, d, ln, status, keep)


def device_labelset(hix, lb, k, sets, queries=None, qids=None, exclude=None, stream=None):
    """phnsw_search_exact_labelset_device with torch buffers -> ids u64, d, len u64, status"""
    import torch
    first, values = ph.hnsw.pack_label_sets(sets, len(sets))
    launch, out = staged_labelset(hix, lb, k, first, values, queries=queries, qids=qids, exclude=exclude)
    torch.cuda.synchronize()
    launch(stream)
    return fetch(out)


def masks(sets, labels=None):
    first, values = sr.csr(sets)
    return sr.masks_of_sets(column() if labels is None else labels, first, values)


def check(w, lb, sets, exclude=None, k=10, members=None, hix=None, device=True, forms=(0, 1), scan=True, labels=None):
    """raw (0) and stored (1) queries, host and device form, against both yardsticks -> the host results by form"""
    hix = hix or w["hix"]
    nq = len(sets)
    allow = masks(sets, labels)
    out = {}
    for form in forms:
        kw, D = (dict(queries=w["q"][:nq]), w["Dq"][:nq]) if form == 0 else (dict(qids=w["qids"][:nq]), w["Ds"][:nq])
        e = None if exclude is None else exclude[:nq]
        ref = xr.exact_topk(D, allow, e, members, k)
        got = hix.search_exact_labelset(labels=lb, want=sets, exclude=e, k=k, **kw)
        same(got, ref)
        if scan:
            same(got, hix.search_exact_filtered(allow=allow, exclude=e, k=k, **kw))
        assert (got[0][np.arange(k)[None, :] >= got[2][:, None]] == EMPTY).all()
        assert (bits(got[1])[np.arange(k)[None, :] >= got[2][:, None]] == bits(xr.FMAX)).all()
        if device:
            dv = device_labelset(hix, lb, k, sets, exclude=e, **kw)
            assert not dv[3].any()
            same(dv, ref)
        out[form] = got
    return out


# ---------------------------------------------------------------- 1: the equality grid
@pytest.mark.parametrize("kind,dim", KINDS)
def test_kinds_and_dimensions(kind, dim):
    sets = cycle_sets()
    counts = masks(sets).sum(1)
    assert counts[0] == 2140 + 65 and counts[2] == 129 and counts[6] == N - 100 and counts[8] == 0 and counts[12] == 0
    got = check(world_of(kind, dim), handle(kind, dim), sets, k=10)
    if kind not in ("i8q", "pq"):  # normalised rows: nothing is nearer to a row than its copies; ids decide among them
        for form in (0, 1):
            np.testing.assert_array_equal(got[form][0][0], DUPS[:10].astype(np.uint64))


@pytest.mark.parametrize("metric", [oracle.METRIC_L2, oracle.METRIC_ONE_MINUS_DOT])
def test_the_other_metrics(metric):
    check(world_of("f32", 24, metric), handle("f32", 24, metric), cycle_sets(), k=10)


# ---------------------------------------------------------------- 2: ties across lists
A, B, C3 = 21, 22, 23


@functools.lru_cache(maxsize=None)
def tie_handle():
    """the 40 copies of row 0 split between A and B, alternating by id; C3 on 70 other rows; nothing else is listed"""
    lab = np.full(N, NONE, dtype=np.int64)
    lab[DUPS[0::2]], lab[DUPS[1::2]] = A, B
    lab[np.setdiff1d(np.arange(N), DUPS)[100:170]] = C3
    return lab, ph.Labels(sworld("f32", 24)["hix"], lab)


@pytest.mark.parametrize("slices", [None, "3"])
def test_ties_across_lists_come_back_in_id_order(monkeypatch, slices):
    w = sworld("f32", 24)
    lab, lb = tie_handle()
    sets = [[A, B, C3]] + [[C3, B, A], [B], [A, C3]] * 5
    with env(monkeypatch, **({} if slices is None else {"PHNSW_LABEL_SLICES": slices})):
        for k in (10, 40, 64):
            got = check(w, lb, sets, k=k, labels=lab)
            for form in (0, 1):  # query 0 is the duplicated row, stored query 0 one of its copies
                ids, d, ln = got[form]
                m = min(k, 40)
                np.testing.assert_array_equal(ids[0, :m], DUPS[:m].astype(np.uint64))  # A, B, A, B, ...: interleaved
                assert len(set(bits(d[0, :m]).tolist())) == 1 and ln[0] == min(k, 110)
                assert set(lab[ids[0, :m].astype(np.int64)][0::2]) == {A} and set(lab[ids[0, :m].astype(np.int64)][1::2]) == {B}


# ---------------------------------------------------------------- 3: knobs change nothing
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("pq", 24)])
def test_rows_do_not_depend_on_tiles_and_slices(monkeypatch, kind, dim):
    w, lb, sets = world_of(kind, dim), handle(kind, dim), cycle_sets()
    wanted_by = {v: sum(v in s for s in sets) for v in ALL13}
    assert wanted_by[BIG] > 16 and wanted_by[L65] > 16  # more than 2 and more than 16: tiles of T = 2 and of T = 16 split a group
    base = check(w, lb, sets, k=10)
    for tile in ("1", "2", None):
        for slices in (None, "1", "3"):
            kw = {} if slices is None else dict(PHNSW_LABEL_SLICES=slices)
            if tile:
                kw["PHNSW_LABEL_TILE"] = tile
            with env(monkeypatch, **kw):
                now = check(w, lb, sets, k=10, scan=False)
            for form in (0, 1):
                same(now[form], base[form])


# ---------------------------------------------------------------- 4: k edges
@pytest.mark.parametrize("k", [1, 64, 65, 1024])
def test_k_edges(k):
    w, lb = sworld("f32", 24), handle("f32", 24)
    sets = cycle_sets(16)
    sets[1], sets[2] = list(ALL13), [L65]
    got = check(w, lb, sets, k=k)
    for form in (0, 1):
        assert got[form][2][1] == min(k, N - 100) and got[form][2][2] == min(k, 65)  # full rows; 65 entries and padding


# ---------------------------------------------------------------- 5: exclude
def test_exclude():
    w, lb, sets, lab = sworld("f32", 24), handle("f32", 24), cycle_sets(), column()
    first = check(w, lb, sets, k=64, device=False)
    counts = masks(sets).sum(1)
    for form in (0, 1):
        best = first[form][0][:, 0]  # each query's best hit, where it has one: inside one of its lists, and it matters
        inside = np.where(best == EMPTY, np.uint64(5), best)
        got = check(w, lb, sets, exclude=inside, k=64, forms=(form,))[form]
        has = best != EMPTY
        assert has.sum() > 40 and not (got[0][has] == best[has, None]).any()
        np.testing.assert_array_equal(got[2][has], np.minimum(64, counts[has] - 1))
    # outside every wanted list: a vector of a label the query does not want, an unlabelled one, an id past n, PHNSW_EMPTY
    outside = np.full(NQX, EMPTY, dtype=np.uint64)
    outside[0::4] = int(np.nonzero(lab == HALF)[0][0])
    outside[1::4] = int(np.nonzero(lab == NONE)[0][0])
    outside[2::4] = N + 7
    outside[[HALF in s for s in sets]] = EMPTY
    got = check(w, lb, sets, exclude=outside, k=64)
    for form in (0, 1):
        same(got[form], first[form])
    # a stored query that excludes itself while one of its wanted labels lists it
    qids = w["qids"][:NQX]
    own = [[int(lab[int(v)]), ONE] if lab[int(v)] != NONE else [ONE] for v in qids]
    got = check(w, lb, own, exclude=qids.copy(), k=10, forms=(1,))[1]
    listed = lab[qids.astype(np.int64)] != NONE
    assert listed.sum() > 50 and not (got[0] == qids[:, None]).any()
    plain = check(w, lb, own, k=10, forms=(1,), device=False)[1]
    alone = listed & ~np.isin(qids, DUPS.astype(np.uint64))  # a copy of row 0 ties with the other copies
    assert (plain[0][alone, 0] == qids[alone]).all()  # without the exclude it is its own best hit


# ---------------------------------------------------------------- 6: the order of labels and of queries
def test_rows_do_not_depend_on_the_order_of_labels_or_queries():
    w, lb, sets = sworld("f32", 256), handle("f32", 256), cycle_sets()
    base = check(w, lb, sets, k=10)
    rng = np.random.default_rng(3)
    shuffled = [list(rng.permutation(np.array(s, dtype=np.int64))) if s else [] for s in sets]
    assert any(a != b for a, b in zip(shuffled, sets))
    perm = rng.permutation(NQX)
    for form in (0, 1):
        kw = dict(queries=w["q"]) if form == 0 else dict(qids=w["qids"])
        same(w["hix"].search_exact_labelset(labels=lb, want=shuffled, k=10, **kw), base[form])
        same(device_labelset(w["hix"], lb, 10, shuffled, **kw), base[form])
        kwp = {name: v[perm] for name, v in kw.items()}
        moved = [sets[i] for i in perm]
        same(w["hix"].search_exact_labelset(labels=lb, want=moved, k=10, **kwp), tuple(x[perm] for x in base[form]))
        same(device_labelset(w["hix"], lb, 10, moved, **kwp), tuple(x[perm] for x in base[form]))


# ---------------------------------------------------------------- 7: one-label sets
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("i8q", 24)])
def test_one_label_sets_are_the_labeled_call(kind, dim):
    w, lb = world_of(kind, dim), handle(kind, dim)
    want = np.array([ALL13[i % 13] for i in range(NQX)], dtype=np.int64)
    sets = [[int(v)] for v in want]
    for form in (0, 1):
        kw = dict(queries=w["q"]) if form == 0 else dict(qids=w["qids"])
        ref = w["hix"].search_exact_labeled(labels=lb, want=want, k=10, **kw)
        same(w["hix"].search_exact_labelset(labels=lb, want=sets, k=10, **kw), ref)
        dv, dl = device_labelset(w["hix"], lb, 10, sets, **kw), device_labeled(w["hix"], lb, 10, want, **kw)
        same(dv, ref)
        same(dv, dl)
        np.testing.assert_array_equal(dv[3], dl[3])


# ---------------------------------------------------------------- 8: counts
def test_counts():
    w, lb = sworld("f32", 24), handle("f32", 24)
    sets = cycle_sets() + [[BIG, BIG, BIG], [NONE], [ABSENT, ABSENT], [], [TOP, HALF, TOP]]
    m = masks(sets)
    np.testing.assert_array_equal(lb.count_sets(sets), m.sum(1))
    np.testing.assert_array_equal(lb.count_sets(sets), w["hix"].filter_count(m))
    assert lb.count_sets(sets)[-5:].tolist() == [2140, 0, 0, 0, 300]
    assert lb.count_sets([[], []]).tolist() == [0, 0]  # nothing wanted at all: no values
    # the count does not trust the offsets either: a range past nwant and one that runs backwards count 0
    import torch
    first, values = ph.hnsw.pack_label_sets(sets, len(sets))
    bad = first.copy()
    bad[4] = len(values) + 7
    dev = torch.device("cuda", 0)
    fd, vd = torch.from_numpy(bad.view(np.int32)).to(dev), torch.from_numpy(values.view(np.int32)).to(dev)
    out = torch.full((len(sets),), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    lb.count_set_device(len(sets), len(values), fd.data_ptr(), vd.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    expect = m.sum(1)
    expect[[3, 4]] = 0
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), expect)


# ---------------------------------------------------------------- 9: the device form
def test_the_device_form_runs_on_the_caller_s_stream():
    import torch
    w, lb, sets = sworld("f32", 24), handle("f32", 24), cycle_sets()
    first, values = ph.hnsw.pack_label_sets(sets, NQX)
    ref = xr.exact_topk(w["Dq"], masks(sets), None, None, 10)
    launch, out = staged_labelset(w["hix"], lb, 10, first, values, queries=w["q"])
    torch.cuda.synchronize()
    assert (out[0] == 7).all() and (out[2] == -1).all() and (out[3] == -1).all()  # the sentinels are in place
    stream = torch.cuda.Stream()
    launch(stream)  # enqueues and returns
    stream.synchronize()  # this stream alone
    got = fetch(out)
    assert not got[3].any()
    same(got, ref)


def test_a_stored_query_id_past_n_is_reported_and_harms_nobody():
    w, lb, sets = sworld("f32", 24), handle("f32", 24), cycle_sets(40)
    qids = w["qids"][:40].copy()
    bad = [3, 17, 39]
    qids[bad] = [N, N + 12345, 0xFFFFFFFE]
    ref = xr.exact_topk(w["Ds"][:40], masks(sets), None, None, 10)
    good = np.setdiff1d(np.arange(40), bad)
    dv = device_labelset(w["hix"], lb, 10, sets, qids=qids)
    same(tuple(x[good] for x in dv[:3]), tuple(x[good] for x in ref))
    assert (dv[3][bad] == 4).all() and not dv[3][good].any()
    assert (dv[0][bad] == EMPTY).all() and (bits(dv[1][bad]) == bits(xr.FMAX)).all() and not dv[2][bad].any()
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses such an id and names the query
        w["hix"].search_exact_labelset(qids=qids, labels=lb, want=sets, k=10)
    assert e.value.code == -1 and "phnsw_search_exact_labelset: query 3:" in str(e.value) and "out of range" in str(e.value)


@pytest.mark.parametrize("knobs", [dict(), dict(PHNSW_LABEL_TILE="1", PHNSW_LABEL_SLICES="3")])
def test_offsets_that_are_not_sound_spoil_their_own_queries_only(monkeypatch, knobs):
    """one offset out of place: want_first[j] = nwant + 7 makes query j - 1 run past nwant and query j run backwards;
    every other query keeps the range it had"""
    import torch
    w, lb, sets = sworld("f32", 24), handle("f32", 24), cycle_sets()
    first, values = ph.hnsw.pack_label_sets(sets, NQX)
    j = 23  # queries 22 ([ALL13]) and 23 (the five REST labels): both want something
    assert first[j - 1] < first[j] < first[j + 1]
    broken = first.copy()
    broken[j] = len(values) + 7
    with env(monkeypatch, **knobs):
        for form in (0, 1):
            kw = dict(queries=w["q"]) if form == 0 else dict(qids=w["qids"])
            launch, out = staged_labelset(w["hix"], lb, 10, first, values, **kw)
            launch_b, out_b = staged_labelset(w["hix"], lb, 10, broken, values, **kw)
            torch.cuda.synchronize()
            launch()
            launch_b()
            honest, got = fetch(out), fetch(out_b)
            assert not honest[3].any()
            same(honest, xr.exact_topk((w["Dq"], w["Ds"])[form], masks(sets), None, None, 10))
            spoilt = [j - 1, j]
            others = np.setdiff1d(np.arange(NQX), spoilt)
            assert (got[3][spoilt] == ST_RANGE).all() and not got[3][others].any()
            assert (got[0][spoilt] == EMPTY).all() and (bits(got[1][spoilt]) == bits(xr.FMAX)).all() and not got[2][spoilt].any()
            same(tuple(x[others] for x in got[:3]), tuple(x[others] for x in honest[:3]))


def test_two_calls_on_two_streams():
    import torch
    w, lb = sworld("f32", 256), handle("f32", 256)
    a, b = cycle_sets(), [list(SHAPES[(i * 3 + 1) % len(SHAPES)]) for i in range(40)]
    fa, va = ph.hnsw.pack_label_sets(a, NQX)
    fb, vb = ph.hnsw.pack_label_sets(b, 40)
    la, oa = staged_labelset(w["hix"], lb, 10, fa, va, queries=w["q"])
    lb_, ob = staged_labelset(w["hix"], lb, 64, fb, vb, qids=w["qids"][:40])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    la(s1)
    lb_(s2)
    ga, gb = fetch(oa), fetch(ob)
    assert not ga[3].any() and not gb[3].any()
    same(ga, xr.exact_topk(w["Dq"], masks(a), None, None, 10))
    same(gb, xr.exact_topk(w["Ds"][:40], masks(b), None, None, 64))


# ---------------------------------------------------------------- 10: an index over part of its store
def test_vectors_outside_the_index_are_never_returned():
    w = sworld("f32", 24)
    even = np.arange(N) % 2 == 0
    hix = ph.Hnsw.from_layers(w["store"], ring(np.arange(0, N, 2)))  # every second vector: vec2node is not the identity
    lb = ph.Labels(hix, column())
    sets = cycle_sets()
    np.testing.assert_array_equal(lb.count_sets(sets), (masks(sets) & even).sum(1))
    np.testing.assert_array_equal(lb.count_sets(sets), hix.filter_count(masks(sets)))
    got = check(w, lb, sets, members=even, hix=hix, k=100)
    for form in (0, 1):
        assert not (got[form][0][got[form][0] != EMPTY] % 2).any()
    lb.close()


# ---------------------------------------------------------------- 11: checks
def test_checks_in_their_order():
    w, lb = sworld("f32", 24), handle("f32", 24)
    hix, q, sets = w["hix"], w["q"][:4], [[BIG], [], [ONE, ABSENT], [NONE]]
    for k in (0, 1025):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_labelset(queries=q, labels=lb, want=sets, k=k)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_labelset: k must be 1..1024 (got %d)" % k
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_labelset_device(lb, 4, 4, k, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_labelset_device: k must be 1..1024 (got %d)" % k
    # k before the handle, the handle before the other arguments
    other = ph.Hnsw.from_layers(w["store"], ring(np.arange(N)))
    with pytest.raises(ph.PhnswError) as e:
        other.search_exact_labelset_device(lb, 4, 4, 0, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)
    assert "k must be" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:
        other.search_exact_labelset_device(lb, 4, 4, 3, 8, 8, 8, 8)
    assert e.value.code == -1 and "the labels are stale" in str(e.value) and "phnsw_search_exact_labelset_device" in str(e.value)
    # both, neither, no offsets, no values although some are promised, too many pairs
    for bad in (dict(queries=16, ldq=24, qids=8, want_first=8, want_values=8), dict(want_first=8, want_values=8),
                dict(qids=8, want_values=8), dict(qids=8, want_first=8)):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_labelset_device(lb, 4, 4, 3, 8, 8, 8, 8, **bad)
        assert e.value.code == -1 and "phnsw_search_exact_labelset_device: invalid argument" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:
        hix.search_exact_labelset_device(lb, 4, 2 ** 31 - 1, 3, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)
    assert e.value.code == -1 and "below 2^31 - 1" in str(e.value)
    import ctypes as C
    buf = (C.c_uint64 * 64)()
    L = ph.lib()
    for args in ((buf, buf), (None, None)):  # both, then neither, in the host form
        assert L.phnsw_search_exact_labelset(hix._h, lb._h, args[0], args[1], 4, None, buf, buf, 3, buf, buf, buf) == -1
        assert L.phnsw_last_error().decode() == "phnsw_search_exact_labelset: pass queries or qids (exactly one)"
    # nq == 0: a no-op, whatever else is passed
    assert L.phnsw_search_exact_labelset(hix._h, lb._h, None, None, 0, None, None, None, 3, None, None, None) == 0
    assert L.phnsw_search_exact_labelset_device(hix._h, lb._h, None, 0, None, 0, None, None, None, 0, 3, None, None, None, None,
                                                None) == 0
    ids, d, ln = hix.search_exact_labelset(queries=np.zeros((0, 24), dtype=np.float32), labels=lb, want=[], k=3)
    assert ids.shape == (0, 3)
    # the host form refuses offsets that do not start at 0 or run backwards, and names the query
    qp = np.ascontiguousarray(q)
    vals = np.array([BIG, ONE, ABSENT, 5], dtype=np.uint32)
    out_i, out_d, out_l = np.zeros((4, 3), dtype=np.uint64), np.zeros((4, 3), dtype=np.float32), np.zeros(4, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for offsets, who in (([0, 1, 3, 2, 4], 2), ([1, 1, 2, 3, 4], 0)):
        f = np.array(offsets, dtype=np.uint32)
        assert L.phnsw_search_exact_labelset(hix._h, lb._h, p(qp), None, 4, None, p(f), p(vals), 3, p(out_i), p(out_d), p(out_l)) == -1
        msg = L.phnsw_last_error().decode()
        assert msg.startswith("phnsw_search_exact_labelset: query %d: want_first must start at 0 and never run backwards" % who)
    assert not out_i.any() and not out_l.any()  # nothing was written


def test_a_handle_is_stale_after_the_store_has_grown():
    rows = oracle.synth_rows(0, 300, 24)[:, :24].copy()
    store = ph.VectorStore(rows[:200], metric=COS)
    hix = ph.Hnsw.from_layers(store, ring(np.arange(200)))
    lab = np.arange(200) % 4
    lb = ph.Labels(hix, lab)
    sets = [[0, 1], [2], []]
    got = hix.search_exact_labelset(queries=rows[:3], labels=lb, want=sets, k=5)
    same(got, hix.search_exact_filtered(queries=rows[:3], allow=masks(sets, lab), k=5))
    store.append(rows[200:])
    with pytest.raises(ph.PhnswError) as e:
        hix.search_exact_labelset(queries=rows[:3], labels=lb, want=sets, k=5)
    assert e.value.code == -1 and "the labels are stale" in str(e.value) and "phnsw_search_exact_labelset:" in str(e.value)


# ---------------------------------------------------------------- 12: the grids stride past their cap
NS, NQS, PER, LONG = 16000, 600, 8, 9


@functools.lru_cache(maxsize=None)
def stride_world():
    """16 000 rows: one list of 14 100 rows that nobody wants (221 batches: the slice count is clamped to the batches of
    the LONGEST list) and 640 lists of 1 to 3 rows"""
    rows = oracle.synth_rows(5, NS, 24)[:, :24].copy()
    store = ph.VectorStore(rows, metric=COS)
    hix = ph.Hnsw.from_layers(store, ring(np.arange(NS)))
    lab = np.full(NS, NONE, dtype=np.int64)
    perm = np.random.default_rng(8).permutation(NS)
    lab[perm[:14100]] = LONG
    at = 14100
    for j in range(640):
        c = 1 + j % 3
        lab[perm[at:at + c]] = 1000 + j
        at += c
    q = oracle.synth_rows(2 ** 33, NQS, 24)[:, :24].copy()
    D = fr.distance_rows(oracle_over(store, COS), queries=q, mode=oracle.SUM_BLOCKED64)
    rng = np.random.default_rng(9)
    sets = [[int(1000 + v) for v in rng.permutation(640)[:PER]] for _ in range(NQS)]
    return dict(hix=hix, lab=lab, lb=ph.Labels(hix, lab), q=q, D=D, sets=sets)


@pytest.mark.parametrize("tile", [None, "1"])
def test_the_scan_and_the_merge_stride_past_the_grid_cap(monkeypatch, tile):
    w = stride_world()
    assert w["lb"].longest == 14100 and ls.batches(14100) == 221
    slices = ls.slice_count(221, w["lb"].longest)
    assert NQS * PER * slices > ls.GRID_MAX  # positions x slices: the scan's work items
    m = masks(w["sets"], w["lab"])
    assert m.sum(1).max() <= 3 * PER and m.sum(1).min() >= PER
    kw = dict(PHNSW_LABEL_SLICES="221")
    if tile:
        kw["PHNSW_LABEL_TILE"] = tile
    with env(monkeypatch, **kw):
        got = w["hix"].search_exact_labelset(queries=w["q"], labels=w["lb"], want=w["sets"], k=2)
    same(got, xr.exact_topk(w["D"], m, None, None, 2))
    same(got, w["hix"].search_exact_filtered(queries=w["q"], allow=m, k=2))
