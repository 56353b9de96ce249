"""The exact radius search (phnsw_search_exact_radius[_device], filter_radius.hip): every candidate with d < radius[q], as
CSR.  Every comparison is on offsets, ids and distance bits, no tolerance anywhere.

Two yardsticks: tests/radius_reference.py over the oracle's ORC_SUM_BLOCKED64 distances (which the code under test did
not make), and search_exact_shared(k = 1024), whose row cut at d < r the leading entries of a segment must equal.

The world is that of tests/test_gpu_exact_shared.py: N = 5000 rows, 40 copies of row 0 spread over the id range, 65 raw
and 65 stored queries (one block tile of the table plus one row), one-layer ring indexes; f32 rows of 24 floats (the
vector-unit tile pass) and of 256 (the matrix cores), f16 / i8 / i8q rows of 24, the other two metrics on f32."""
import ctypes as C

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import filter_reference as fr
import filter_value_worlds as fw
import radius_reference as rr
from test_gpu_exact_filter import DUPS, EMPTY, N, mask, ring
from test_gpu_exact_shared import NQX, exactly, sworld
from test_gpu_i8 import bits
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

KINDS = [("f32", 24), ("f32", 256), ("f16", 24), ("i8", 24), ("i8q", 24)]
MS = (0, 1, 63, 64, 65, 1000, N - 1)
UP = np.float32(np.inf)


def same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(bits(a[2]), bits(b[2]))


def raw_call(hix, radius, cap, queries=None, qids=None, allow=None, exclude=None, null_arrays=False):
    """phnsw_search_exact_radius as it stands: -> first, total, ids[cap], d[cap]; the arrays are prefilled, so what the
    call did not write shows"""
    nq = len(queries) if queries is not None else len(qids)
    q = None if queries is None else np.ascontiguousarray(queries, dtype=np.float32)
    qi = None if qids is None else np.ascontiguousarray(qids, dtype=np.uint64)
    ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
    words, stride = ph.hnsw.pack_allow(allow, hix.store.n, nq)
    assert stride == 0
    r = rr.radii(radius, nq)
    first = np.full(nq + 1, 77, dtype=np.uint64)
    ids = np.full(min(cap, 1 << 22), 7, dtype=np.uint64)
    d = np.full(min(cap, 1 << 22), -1.0, dtype=np.float32)
    total = C.c_uint64(99)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ph.hnsw.check(ph.lib().phnsw_search_exact_radius(hix._h, p(q), p(qi), nq, p(ex), p(words), p(r), cap, p(first),
                                                    None if null_arrays else p(ids), None if null_arrays else p(d),
                                                    C.byref(total)))
    return first, int(total.value), ids, d


def device_radius(hix, radius, cap, queries=None, qids=None, allow=None, exclude=None, null_arrays=False):
    """phnsw_search_exact_radius_device with torch buffers -> (first, ids u64, d) cut at the total, status, total, and
    the whole prefilled ids / d buffers"""
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
    words, stride = ph.hnsw.pack_allow(allow, hix.store.n, nq)
    assert stride == 0
    wd = 0 if words is None else up(words, np.int32).data_ptr()
    rd = up(rr.radii(radius, nq), None)
    first = torch.full((nq + 1,), 77, dtype=torch.int64, device=dev)
    ids = torch.full((max(cap, 1),), 7, dtype=torch.int32, device=dev)
    d = torch.full((max(cap, 1),), -1.0, dtype=torch.float32, device=dev)
    status = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    total = torch.full((1,), 99, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    hix.search_exact_radius_device(nq, rd.data_ptr(), cap, first.data_ptr(), 0 if null_arrays else ids.data_ptr(),
                                   0 if null_arrays else d.data_ptr(), status.data_ptr(), total.data_ptr(), queries=qd, ldq=ld,
                                   qids=qi, exclude=ex, allow=wd)
    torch.cuda.synchronize()
    t = int(total.cpu().numpy()[0])
    i_all, d_all = ids.cpu().numpy().view(np.uint32).astype(np.uint64), d.cpu().numpy()
    n = t if t <= cap else 0
    return (first.cpu().numpy().view(np.uint64), i_all[:n], d_all[:n]), status.cpu().numpy(), t, i_all, d_all


def forms(w, nq):
    return ((dict(queries=w["q"][:nq]), w["Dq"][:nq]), (dict(qids=w["qids"][:nq]), w["Ds"][:nq]))


def check(w, radius, nq=NQX, allow=None, exclude=None, members=None, hix=None, ref_allow=None, device=True, shared=True,
          which=(0, 1), cap=None):
    """raw (0) and stored (1) queries, host and device form, against both yardsticks.  radius(D) -> [nq] or a value.
    Returns the host results by form."""
    hix = hix or w["hix"]
    out = {}
    for form in which:
        kw, D = forms(w, nq)[form]
        e = None if exclude is None else exclude[:nq]
        ra = ref_allow if ref_allow is not None else allow
        r = radius(D) if callable(radius) else radius
        ref = rr.exact_radius(D, r, ra, e, members)
        got = hix.search_exact_radius(radius=r, allow=allow, exclude=e, cap=cap, **kw)
        same(got, ref)
        np.testing.assert_array_equal(hix.count_exact_radius(radius=r, allow=allow, exclude=e, **kw), ref[0])
        if shared:  # the second yardstick: the leading min(1024, count) entries of every segment
            ti, td, tl = hix.search_exact_shared(allow=allow, exclude=e, k=1024, **kw)
            rq = rr.radii(r, nq)
            for q in range(nq):
                si, sd = rr.segment(got, q)
                with np.errstate(invalid="ignore"):
                    cut = int(((td[q, :int(tl[q])] < rq[q]) & (rq[q] > 0)).sum())
                assert cut == min(1024, len(si))
                np.testing.assert_array_equal(si[:cut], ti[q, :cut])
                np.testing.assert_array_equal(bits(sd[:cut]), bits(td[q, :cut]))
        if device:
            dv, status, total, _, _ = device_radius(hix, r, max(len(ref[1]), 1), allow=allow, exclude=e, **kw)
            assert not status.any() and total == len(ref[1])
            same(dv, ref)
        out[form] = got
    return out


# ---------------------------------------------------------------- 1: radii taken from the oracle matrix
@pytest.mark.parametrize("kind,dim", KINDS)
def test_radii_at_the_mth_smallest_distance_and_the_next_float_up(kind, dim):
    w = sworld(kind, dim)
    for shift in (0, 3):  # the radii differ inside a batch: query q takes m = MS[(q + shift) % 7]
        m = np.array([MS[(q + shift) % len(MS)] for q in range(NQX)])
        assert len(set(m.tolist())) == len(MS)
        at = lambda D: rr.mth_smallest(D, m[:len(D)])
        above = lambda D: np.nextafter(at(D), UP)
        lo = check(w, at, device=shift == 0, shared=shift == 0)
        hi = check(w, above, device=shift == 3, shared=shift == 3)
        for form in (0, 1):
            D = forms(w, NQX)[form][1]
            n_lo, n_hi = np.diff(lo[form][0].astype(np.int64)), np.diff(hi[form][0].astype(np.int64))
            pos = at(D) > 0  # a radius at or below zero matches nothing (a cosine distance of a copy may round below 0)
            assert (n_lo[pos] <= m[pos]).all() and (n_hi[pos & (above(D) > 0)] > m[pos & (above(D) > 0)]).all()
            assert (n_lo[~pos] == 0).all()


@pytest.mark.parametrize("kind,dim,metric", [(k, d, None) for k, d in KINDS] +
                         [("f32", 24, oracle.METRIC_L2), ("f32", 24, oracle.METRIC_ONE_MINUS_DOT)])
def test_the_forty_copies_at_their_distance_and_at_the_next_float_up(kind, dim, metric):
    w = sworld(kind, dim) if metric is None else sworld(kind, dim, metric)
    dup = DUPS.astype(np.uint64)
    seen_all = 0
    for form in (0, 1):  # query 0 is the duplicated row, stored query 0 one of its copies
        kw, D = forms(w, NQX)[form]
        d0 = D[0, DUPS[0]]
        assert (bits(D[0, DUPS]) == bits(d0)).all()
        r = rr.mth_smallest(D, 70)  # the other queries: a radius of their own
        r[0] = d0
        got = check(w, r, which=(form,), device=False)[form]
        assert not np.isin(rr.segment(got, 0)[0], dup).any()  # strict: at their distance none of them
        r[0] = np.nextafter(d0, UP)
        got = check(w, r, which=(form,), device=form == 0)[form]
        si, sd = rr.segment(got, 0)
        at = np.nonzero(np.isin(si, dup))[0]
        if r[0] > 0:
            seen_all += 1
            assert len(at) == 40 and (np.diff(at) == 1).all()  # all forty, adjacent, in id order, one distance
            np.testing.assert_array_equal(si[at], dup)
            assert len(set(bits(sd[at]).tolist())) == 1
        else:
            assert len(si) == 0
    if metric == oracle.METRIC_L2:
        assert seen_all == 2  # equal rows are at exactly 0.0 under L2: the next float up is above zero


# ---------------------------------------------------------------- 2: radius value edges
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("f32", 256), ("i8q", 24)])
def test_zero_negative_nan_and_infinite_radii(kind, dim):
    w = sworld(kind, dim)
    allow = mask(0.3, N, 41)
    for value in (0.0, -1.0, np.nan, -np.inf, -0.0):
        got = check(w, np.float32(value), nq=40, allow=allow, device=value == 0.0)
        for form in (0, 1):
            assert not got[form][0].any() and len(got[form][1]) == 0
    got = check(w, np.float32(np.inf), nq=40, allow=allow)
    for form in (0, 1):
        assert (np.diff(got[form][0].astype(np.int64)) == allow.sum()).all()  # every candidate: all distances are finite
    mixed = np.tile(np.array([np.inf, 0.0, 0.3, np.nan, -1.0, 0.6], dtype=np.float32), 7)[:40]  # all of them in one batch
    got = check(w, mixed, nq=40, allow=allow)
    n = np.diff(got[0][0].astype(np.int64))
    assert (n[0::6] == allow.sum()).all() and not n[1::6].any() and not n[3::6].any() and not n[4::6].any()


@pytest.mark.parametrize("key", fw.INF_WORLDS, ids=fw.world_id)
def test_a_row_at_inf_is_never_inside_a_radius(key):
    from test_gpu_filter_value_edges import ring_index
    w, hix = fw.world(*key), ring_index(key)
    allow = fw.inf_bitmap(w)
    finite = np.isfinite(w["Dq"][:, allow])
    assert (~finite).any() and finite.any()
    for r in (np.float32(np.inf), fr.FMAX):
        ref = rr.exact_radius(w["Dq"], r, allow)
        got = hix.search_exact_radius(queries=w["q"], radius=r, allow=allow)
        same(got, ref)
        np.testing.assert_array_equal(np.diff(got[0].astype(np.int64)), finite.sum(axis=1))
        assert np.isfinite(got[2]).all()
        dv, status, total, _, _ = device_radius(hix, r, len(ref[1]), queries=w["q"], allow=allow)
        same(dv, ref)
    ref = rr.exact_radius(w["Dq"], np.float32(np.inf))  # no filter: 2100 candidates, the replaced rows among them
    same(hix.search_exact_radius(queries=w["q"], radius=np.inf), ref)
    assert (np.diff(ref[0].astype(np.int64)) < fw.N).all()


# ---------------------------------------------------------------- 3: chunking
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("f32", 24), ("i8q", 24)])
def test_the_result_does_not_depend_on_the_chunks(monkeypatch, capfd, kind, dim):
    w = sworld(kind, dim)
    allow = mask(0.06, N, 9)
    allow[DUPS] = True  # ties that cross chunk borders: the copies are spread over the id range
    c = int(allow.sum())
    r = lambda D: rr.mth_smallest(D, np.arange(len(D)) * 4 % c, allow)
    base = check(w, r, allow=allow)
    nodes, positions = 64, 22
    with env(monkeypatch, PHNSW_DENSE_NODES=str(nodes), PHNSW_DENSE_TABLE_BYTES=str(64 * 4 * positions), PHNSW_VERBOSE="1"):
        capfd.readouterr()
        now = check(w, r, allow=allow, device=False, shared=False, which=(0,), cap=1 << 20)
        lines = [x for x in capfd.readouterr().err.splitlines() if "exact radius table: node chunk" in x]
        rest = check(w, r, allow=allow, shared=False, which=(1,))
    # dense_plan.h's rules: node chunks of 64 ids, tables of 64 x 4 bytes a row, so 22 positions each
    node_chunks, pos_chunks = (c + nodes - 1) // nodes, (NQX + positions - 1) // positions
    assert node_chunks >= 3 and pos_chunks == 3
    assert len(lines) == 2 * node_chunks * pos_chunks  # the search (its room suffices: one call) and the count-only call
    assert sum("positions 44..+21" in x for x in lines) == 2 * node_chunks
    same(base[0], now[0])
    same(base[1], rest[1])
    with env(monkeypatch, PHNSW_DENSE_TABLE_BYTES="1", PHNSW_DENSE_NODES="192"):  # one position per table
        one = check(w, r, nq=16, allow=allow, device=False, shared=False)
    for form in (0, 1):
        end = int(base[form][0][16])  # the first sixteen queries have the radii they had among the 65
        same(one[form], (base[form][0][:17], base[form][1][:end], base[form][2][:end]))


# ---------------------------------------------------------------- 4: capacity
def test_size_negotiation():
    w = sworld("f32", 256)
    allow = mask(0.3, N, 5)
    for form in (0, 1):
        kw, D = forms(w, 40)[form]
        r = rr.mth_smallest(D, 30 + np.arange(40), allow)
        ref = rr.exact_radius(D, r, allow)
        total = len(ref[1])
        assert total > 40 * 29
        first, t, ids, d = raw_call(w["hix"], r, total, allow=allow, **kw)  # cap == total: filled
        assert t == total
        same((first, ids, d), ref)
        for cap in (total - 1, 1):  # too small: exact offsets and total, the arrays not touched
            first, t, ids, d = raw_call(w["hix"], r, cap, allow=allow, **kw)
            assert t == total and (ids == 7).all() and (d == -1.0).all()
            np.testing.assert_array_equal(first, ref[0])
            dv, status, t, i_all, d_all = device_radius(w["hix"], r, cap, allow=allow, **kw)
            assert t == total and (i_all == 7).all() and (d_all == -1.0).all() and not status.any()
            np.testing.assert_array_equal(dv[0], ref[0])
        first, t, ids, d = raw_call(w["hix"], r, total + 1000, allow=allow, **kw)  # room to spare: the tail untouched
        same((first, ids[:total], d[:total]), ref)
        assert (ids[total:] == 7).all() and (d[total:] == -1.0).all()
        first, t, _, _ = raw_call(w["hix"], r, 0, allow=allow, null_arrays=True, **kw)  # counts only
        assert t == total
        np.testing.assert_array_equal(first, ref[0])
        dv, status, t, _, _ = device_radius(w["hix"], r, 0, allow=allow, null_arrays=True, **kw)
        assert t == total and not status.any()
        np.testing.assert_array_equal(dv[0], ref[0])
        got = w["hix"].search_exact_radius(radius=r, allow=allow, cap=5, **kw)  # the method asks again, once
        same(got, ref)
    with pytest.raises(ph.PhnswError) as e:
        raw_call(w["hix"], 1.0, 1 << 31, queries=w["q"][:4])
    assert e.value.code == -1  # PHNSW_E_INVALID
    assert str(e.value) == "phnsw error -1: phnsw_search_exact_radius: cap must be at most 2^31 - 1 (got 2147483648)"
    with pytest.raises(ph.PhnswError) as e:
        w["hix"].search_exact_radius_device(4, 8, 1 << 31, 8, 8, 8, 8, 8, qids=8)
    assert str(e.value) == "phnsw error -1: phnsw_search_exact_radius_device: cap must be at most 2^31 - 1 (got 2147483648)"


# ---------------------------------------------------------------- 5: filter, exclude, members
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("f16", 24)])
def test_filter_exclude_and_an_index_over_part_of_its_store(kind, dim):
    import torch
    w = sworld(kind, dim)
    few = exactly(40, 3)  # a few dozen bits
    check(w, lambda D: rr.mth_smallest(D, 20, few), allow=few)
    got = check(w, lambda D: rr.mth_smallest(D, 0, few), allow=few)  # ... none of them inside the radius
    assert not got[0][0].any() and not got[1][0].any()
    check(w, 0.4, allow=np.zeros(N, dtype=bool))  # no candidate at all
    own = np.full(NQX, EMPTY, dtype=np.uint64)
    ex = {0: own, 1: w["qids"].copy()}  # a stored query excludes itself
    allow = mask(0.3, N, 78)
    allow[w["qids"].astype(np.int64)] = True
    for form in (0, 1):
        r = lambda D: rr.mth_smallest(D, 50, allow)  # the radius of the call without exclude: the query itself is inside
        got = check(w, r, allow=allow, exclude=ex[form], which=(form,))[form]
        if form == 1:
            for q in range(NQX):
                assert int(w["qids"][q]) not in rr.segment(got, q)[0]
            assert (np.diff(got[0].astype(np.int64)) <= 49).all()
    mixed = np.full(NQX, EMPTY, dtype=np.uint64)  # a candidate, a non-candidate, PHNSW_EMPTY, an id past n, in turn
    mixed[0::4], mixed[1::4], mixed[3::4] = np.nonzero(allow)[0][5], np.nonzero(~allow)[0][5], N + 7
    check(w, np.float32(np.inf), allow=allow, exclude=mixed)
    even = np.arange(N) % 2 == 0
    hix = ph.Hnsw.from_layers(w["store"], ring(np.arange(0, N, 2)))  # every second vector: vec2node is not the identity
    got = check(w, lambda D: rr.mth_smallest(D, 100, allow, None, even), allow=allow, members=even, hix=hix)
    assert not (got[0][1] % 2).any() and len(got[0][1])
    head = np.arange(N) < N - 100
    hix = ph.Hnsw.from_layers(w["store"], ring(np.arange(N - 100)))  # the first N - 100: identity, shorter than the store
    got = check(w, np.float32(np.inf), nq=16, allow=None, members=head, hix=hix, device=False)
    assert (np.diff(got[0][0].astype(np.int64)) == N - 100).all()
    words = torch.from_numpy(fr.pack(few).view(np.int32)).to(torch.device("cuda", 0))  # the default filter serves NULL
    torch.cuda.synchronize()
    w["hix"].set_filter(words.data_ptr())
    try:
        check(w, 0.45, nq=40, allow=None, ref_allow=few)
        check(w, 0.45, nq=40, allow=allow)  # an explicit filter wins
    finally:
        w["hix"].set_filter(0)
    check(w, 0.3, nq=40, allow=None)


# ---------------------------------------------------------------- 6: the device form, refusals
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("f32", 24)])
def test_a_stored_query_id_past_n_is_reported_and_harms_nobody(monkeypatch, kind, dim):
    w = sworld(kind, dim)
    allow = mask(0.3, N, 21)
    qids = w["qids"][:40].copy()
    bad = [3, 17, 39]
    qids[bad] = [N, N + 12345, 0xFFFFFFFE]
    r = rr.mth_smallest(w["Ds"][:40], 25, allow)
    for knobs in ({}, dict(PHNSW_DENSE_NODES="64")):  # ... and carried through many node chunks
        with env(monkeypatch, **knobs):
            dv, status, total, _, _ = device_radius(w["hix"], r, 40 * 25, qids=qids, allow=allow)
        rz = r.copy()
        rz[bad] = 0.0  # the reference: those three match nothing
        ref = rr.exact_radius(w["Ds"][:40], rz, allow)
        same(dv, ref)
        assert total == len(ref[1]) and 37 * 20 < total <= 37 * 25
        good = np.setdiff1d(np.arange(40), bad)
        assert (status[bad] == 4).all() and not status[good].any()
    none = device_radius(w["hix"], r, 10, qids=qids, allow=np.zeros(N, dtype=bool))  # no candidate at all: the same report
    assert (none[1][bad] == 4).all() and not none[1][good].any() and none[2] == 0 and not none[0][0].any()
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses it like its siblings
        w["hix"].search_exact_radius(qids=qids.astype(np.uint64), radius=r)
    with pytest.raises(ph.PhnswError) as e2:
        w["hix"].search_exact_shared(qids=qids.astype(np.uint64), k=3)
    assert e.value.code == e2.value.code == -1 and str(e.value) == str(e2.value)


def test_refusals():
    w = sworld("f32", 24)
    hix, q = w["hix"], w["q"][:4]
    with pytest.raises(ValueError):
        hix.search_exact_radius(queries=q, qids=w["qids"][:4], radius=1.0)
    with pytest.raises(ValueError):
        hix.search_exact_radius(radius=1.0)
    with pytest.raises(ValueError):
        hix.search_exact_radius(queries=q)
    with pytest.raises(ValueError):  # a 2-D mask: per-query bitmaps are out of scope
        hix.search_exact_radius(queries=q, radius=1.0, allow=np.ones((4, N), dtype=bool))
    with pytest.raises(ph.PhnswError) as e:  # queries and qids
        hix.search_exact_radius_device(4, 8, 3, 8, 8, 8, 8, 8, queries=16, ldq=24, qids=8)
    assert e.value.code == -1 and "phnsw_search_exact_radius_device" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # no radius
        hix.search_exact_radius_device(4, 0, 3, 8, 8, 8, 8, 8, qids=8)
    assert e.value.code == -1 and "phnsw_search_exact_radius_device" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:  # cap without arrays
        hix.search_exact_radius_device(4, 8, 3, 8, 0, 0, 8, 8, qids=8)
    assert e.value.code == -1
    first, ids, d = hix.search_exact_radius(queries=np.zeros((0, 24), dtype=np.float32), radius=1.0)  # nq == 0: the empty result
    assert first.tolist() == [0] and len(ids) == 0 and len(d) == 0
    # PQ stores of either form and rows longer than 1536 floats: unsupported, the message names the call
    rows = oracle.synth_rows(0, 400, 32)[:, :32].copy()
    f2 = ph.VectorStore(rows, metric=ph.METRIC_L2)
    shared = ph.SharedPqStore(f2, 16, 100, seed=3, centroid_bp=ph.BuildParameters(seed=2),
                              quantized_search=ph.SearchParameters(32, 32, 2))
    long_rows = ph.VectorStore(oracle.synth_rows(0, 64, 1540)[:, :1540].copy(), metric=ph.METRIC_L2)
    for store, n, dim in ((ph.PqStore(f2, 16), 400, 32), (shared, 400, 32), (long_rows, 64, 1540)):
        pix = ph.Hnsw.from_layers(store, ring(np.arange(n)))
        with pytest.raises(ph.PhnswError) as e:
            pix.search_exact_radius(queries=np.zeros((2, dim), dtype=np.float32), radius=1.0)
        assert e.value.code == -7 and "phnsw_search_exact_radius:" in str(e.value)  # PHNSW_E_UNSUPPORTED
        with pytest.raises(ph.PhnswError) as e:
            pix.search_exact_radius_device(2, 8, 3, 8, 8, 8, 8, 8, qids=8)
        assert e.value.code == -7 and "phnsw_search_exact_radius_device:" in str(e.value)
        with pytest.raises(ph.PhnswError) as e:  # the index, then cap, then the store
            pix.search_exact_radius_device(2, 8, 1 << 31, 8, 8, 8, 8, 8, qids=8)
        assert e.value.code == -1
