"""The radius search by graph walk (phnsw_search_batch_radius[_device], search_radius.hip) against its restatement
(tests/radius_reference.search_radius_one, pinned to the oracle by tests/test_radius_cpu.py) over the oracle's
ORC_SUM_BLOCKED64 distances: ids, distance bits, out_len, status and the {evaluations, hops} counters, no tolerance.

Worlds: the small multi-layer index of tests/test_gpu_filter.py (N = 2000, phnsw_build's graph), raw and stored queries,
with and without exclude; and a one-layer ring over 50 rows, fewer than number_of_candidates, where the queue never
fills.  The radii come from the oracle matrix, and which shape of the loop each query takes is asserted from the
restatement's own trace, so no case can quietly stop happening."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import radius_reference as rr
import value_families as vf
from test_gpu_exact_filter import ring
from test_gpu_filter import COS, EMPTY, N, dist, raw_queries, world
from test_gpu_i8 import bits
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

NQ = 18
INF = np.float32(np.inf)


def same(got, ref):
    """ids, distance bits, out_len, status, counters"""
    np.testing.assert_array_equal(got[2], ref[2])
    np.testing.assert_array_equal(got[3], ref[3])
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(bits(got[1]), bits(ref[1]))
    np.testing.assert_array_equal(got[4], ref[4])


def device_walk(hix, sp, radius, max_out, queries=None, qids=None, exclude=None):
    """phnsw_search_batch_radius_device with torch buffers -> ids u64, d, len u64, status, stats u64"""
    import torch
    dev = torch.device("cuda", 0)
    keep = []

    def up(a, dt):
        t = torch.from_numpy(np.array(a).view(dt) if dt is not None else np.array(a)).to(dev)
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
    rd = up(rr.radii(radius, nq), None)
    ids = torch.full((nq, max_out), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq, max_out), -1.0, dtype=torch.float32, device=dev)
    ln = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    st = torch.full((nq, 2), -1, dtype=torch.int32, device=dev)
    status = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    hix.search_radius_device(nq, sp, rd.data_ptr(), max_out, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(),
                             queries=qd, ldq=ld, qids=qi, exclude=ex, out_stats=st.data_ptr())
    torch.cuda.synchronize()
    i64 = ids.cpu().numpy().view(np.uint32).astype(np.uint64)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return (i64, d.cpu().numpy(), ln.cpu().numpy().view(np.uint32).astype(np.uint64), status.cpu().numpy().view(np.uint32),
            st.cpu().numpy().view(np.uint32).astype(np.uint64))


@functools.lru_cache(maxsize=None)
def walk_world(kind, dim):
    """the index, its layers for the restatement, NQ raw and NQ stored queries and the oracle's distance of each to
    every row; made once, changed by no test"""
    hix, oix, layers, _ = world(kind, dim)
    q = raw_queries(kind, dim, NQ)
    qids = np.linspace(3, N - 1, NQ).astype(np.uint64)
    return dict(hix=hix, layers=layers, q=q, qids=qids, Dq=dist(oix, queries=q), Ds=dist(oix, qids=qids))


def forms(w):
    return ((dict(queries=w["q"]), w["Dq"]), (dict(qids=w["qids"]), w["Ds"]))


def check(w, sp, radius, max_out=64, exclude=None, which=(0, 1), device=True, layers=None, hix=None):
    """host and device form of both query forms against the restatement -> the reference results (with traces) by form"""
    hix, layers = hix or w["hix"], layers or w["layers"]
    out = {}
    for form in which:
        kw, D = forms(w)[form]
        r = radius(D) if callable(radius) else radius
        ref = rr.search_radius(layers, D, sp, r, exclude, max_out)
        got = hix.search_radius(radius=r, sp=ph.SearchParameters(*sp), exclude=exclude, max_out=max_out, stats=True, **kw)
        same(got, ref)
        if device:
            same(device_walk(hix, ph.SearchParameters(*sp), r, max_out, exclude=exclude, **kw), ref)
        out[form] = ref
    return out


# upper_layer_candidate_count below number_of_candidates: the bottom-layer queue then starts with room to grow into (a
# queue that starts full ends the loop after one call, whatever the radius: len cannot pass last_size)
SP = (64, 8, 2)
# the m-th smallest distance of each query as its radius: from a handful of rows inside it to several hundred
MS = (2, 12, 40, 75, 110, 160, 220, 300, 450)


def by_m(D):
    return rr.mth_smallest(D, [MS[q % len(MS)] for q in range(len(D))])


# ---------------------------------------------------------------- 1: the shapes of the loop
@pytest.mark.parametrize("with_exclude", [False, True], ids=["all", "exclude"])
def test_the_loop_runs_once_doubles_once_and_doubles_twice(with_exclude):
    w = walk_world("f32", 100)
    ex = None
    if with_exclude:  # a stored query excludes itself, a raw one the nearest row the walk would return
        ex = w["qids"].copy()
    res = check(w, SP, by_m, exclude=ex, which=(1,) if with_exclude else (0, 1))
    for form, ref in res.items():
        traces = ref[5]
        assert not ref[3].any() and all(t["capacity"] <= 1024 and not t["over"] for t in traces)  # nothing hides behind status 6
        caps = [t["capacity"] for t in traces]
        assert any(t["calls"] == 1 for t in traces)            # the loop runs once
        assert 128 in caps and 256 in caps                     # the queue doubles once; twice: 64 -> 256
        assert any(t["calls"] >= 3 for t in traces)
        if with_exclude:
            assert not (ref[0] == ex[:, None]).any()
            assert (ref[2] > 0).any()
    if not with_exclude:  # raw queries excluding the best hit of the call without exclude
        best = res[0][0][:, 0].copy()
        got = check(w, SP, by_m, exclude=best, which=(0,))[0]
        assert not (got[0] == best[:, None]).any()


def test_radii_at_and_below_zero_make_no_bottom_layer_call():
    w = walk_world("f32", 100)
    r = np.tile(np.array([0.0, -1.0, np.nan, -0.0, 0.4, -np.inf], dtype=np.float32), 3)
    res = check(w, SP, r)
    for form, ref in res.items():
        none = np.arange(NQ) % 6 != 4
        assert not ref[2][none].any() and (ref[0][none] == EMPTY).all() and all(ref[5][q]["calls"] == 0 for q in np.nonzero(none)[0])
        assert ref[2][~none].any()
        # the counters of the upper layers only: less than the queries that walk the bottom layer
        assert (ref[4][none, 0] < ref[4][~none, 0].min()).all()


def test_a_queue_that_would_pass_1024_entries_is_status_6():
    w = walk_world("f32", 100)
    w = dict(w, q=w["q"][:5], qids=w["qids"][:5], Dq=w["Dq"][:5], Ds=w["Ds"][:5])  # five queries: the restatement walks 1024-entry queues
    res = check(w, (512, 512, 2), INF)
    for form, ref in res.items():
        assert (ref[3] == 6).all() and not ref[2].any() and (ref[0] == EMPTY).all()
        assert all(t["over"] and t["capacity"] == 1024 for t in ref[5])
    res = check(w, (512, 64, 2), lambda D: rr.mth_smallest(D, 200), device=False)  # the same queues, a radius they hold
    for form, ref in res.items():
        assert not ref[3].any() and (ref[2] > 0).all()


@functools.lru_cache(maxsize=None)
def ring_world():
    """50 rows, one layer, every node linked to its two neighbours: fewer nodes than number_of_candidates"""
    n, dim = 50, 100
    rows = oracle.synth_rows(77, n, dim)
    store = ph.VectorStore(rows[:, :dim].copy(), metric=COS)
    layer = ring(np.arange(n))
    hix = ph.Hnsw.from_layers(store, layer)
    q = np.ascontiguousarray(oracle.synth_rows(2 ** 33, NQ, dim)[:, :dim])
    qids = np.arange(NQ, dtype=np.uint64) * 2
    layers = [(layer[0][0], layer[0][1], {i: i for i in range(n)})]
    return dict(hix=hix, layers=layers, q=q, qids=qids, Dq=vf.oracle_matrix(rows, q, COS, oracle.SUM_BLOCKED64),
                Ds=vf.oracle_matrix(rows, np.ascontiguousarray(rows[qids.astype(np.int64), :dim]), COS, oracle.SUM_BLOCKED64))


def test_a_queue_that_never_fills_grows_over_two_calls():
    w = ring_world()
    res = check(w, SP, INF, max_out=64, exclude=None)
    for form, ref in res.items():
        assert all(t["calls"] >= 2 and t["capacity"] == 64 for t in ref[5]) and not ref[3].any()
        assert (ref[2] <= 50).all() and (ref[2] > 2).all()
    check(w, SP, lambda D: rr.mth_smallest(D, 20), exclude=w["qids"], which=(1,))
    check(w, (16, 16, 1), lambda D: rr.mth_smallest(D, 30))  # 16 -> 32 -> 64 on the ring


# ---------------------------------------------------------------- 2: truncation, the exact call, the fallback
def test_max_out_below_out_len_keeps_the_nearest():
    w = walk_world("f32", 100)
    wide = check(w, SP, by_m, max_out=1024, device=False)
    for max_out in (1, 8, 65):
        cut = check(w, SP, by_m, max_out=max_out)
        for form in (0, 1):
            np.testing.assert_array_equal(cut[form][2], wide[form][2])  # out_len is not truncated
            assert (cut[form][2] > max_out).any()
            np.testing.assert_array_equal(cut[form][0], wide[form][0][:, :max_out])
            np.testing.assert_array_equal(bits(cut[form][1]), bits(wide[form][1][:, :max_out]))


def test_every_returned_pair_is_in_the_exact_segment_and_the_fallback():
    w = walk_world("f32", 100)
    hix = w["hix"]
    for form in (0, 1):
        kw, D = forms(w)[form]
        r = by_m(D)
        ex = w["qids"] if form == 1 else None
        ids, d, ln, status = hix.search_radius(radius=r, sp=ph.SearchParameters(*SP), exclude=ex, max_out=1024, **kw)
        exact = hix.search_exact_radius(radius=r, exclude=ex, **kw)
        assert not status.any()
        for q in range(NQ):
            xi, xd = rr.segment(exact, q)
            pairs = set(zip(xi.tolist(), bits(xd).tolist()))
            assert all((int(i), int(b)) in pairs for i, b in zip(ids[q, :int(ln[q])], bits(d[q, :int(ln[q])])))
            assert int(ln[q]) <= len(xi)
        # the fallback: max_out 32 is too small for some queries, and at number_of_candidates 512 a wide radius is status 6
        for sp, rad, mo in ((SP, r, 32), ((512, 512, 2), np.where(np.arange(NQ) % 2 == 0, r, INF).astype(np.float32), 1024)):
            wi, wd, wl, ws = hix.search_radius(radius=rad, sp=ph.SearchParameters(*sp), exclude=ex, max_out=mo, **kw)
            back = (ws == 6) | (wl > mo)
            assert back.any() and not back.all()
            xf = hix.search_exact_radius(radius=rad, exclude=ex, **kw)
            first, fi, fd, fs = hix.search_radius(radius=rad, sp=ph.SearchParameters(*sp), exclude=ex, max_out=mo, exact_fallback=True, **kw)
            assert not fs.any() and first[0] == 0 and first[NQ] == len(fi) == len(fd)
            for q in range(NQ):
                gi, gd = rr.segment((first, fi, fd), q)
                wi_q, wd_q = (rr.segment(xf, q) if back[q] else (wi[q, :int(wl[q])], wd[q, :int(wl[q])]))
                np.testing.assert_array_equal(gi, wi_q)
                np.testing.assert_array_equal(bits(gd), bits(wd_q))


# ---------------------------------------------------------------- 3: the launch plan, the other row kinds, refusals
def test_the_result_does_not_depend_on_the_launch_plan(monkeypatch):
    w = walk_world("f32", 100)
    base = check(w, SP, by_m, device=False)
    with env(monkeypatch, PHNSW_TWO_LAUNCH_MIN="1", PHNSW_SPLIT_BYTES="1"):  # a plain search of this size would now split
        check(w, SP, by_m)
    with env(monkeypatch, PHNSW_NO_LOCALITY="1"):
        now = check(w, SP, by_m, device=False)
    full = check(w, (64, 64, 2), by_m, device=False)  # a queue that starts full: one call, however wide the radius
    for form in (0, 1):  # (where the layer above handed over a full set of candidates)
        assert all(t["calls"] == 1 and t["capacity"] <= 128 for t in full[form][5] if t["start"] == 64)
        assert any(t["start"] == 64 for t in full[form][5])
    for form in (0, 1):
        same(now[form], base[form])


@pytest.mark.parametrize("kind,dim", [("f32", 768), ("f16", 100), ("i8", 100), ("i8q", 128)])
def test_the_other_row_kinds_and_three_chunks_a_lane(kind, dim):
    w = walk_world(kind, dim)
    res = check(w, SP, by_m)
    for form, ref in res.items():
        assert not ref[3].any()
        if kind != "i8q":  # (on the lattice rows of the i8q world the restated walk never fills its 64 slots inside these radii)
            assert max(t["capacity"] for t in ref[5]) >= 128


def test_refusals():
    w = walk_world("f32", 100)
    hix, q = w["hix"], w["q"][:4]
    for max_out in (0, 1025):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_radius(queries=q, radius=0.3, max_out=max_out)
        assert e.value.code == -1 and str(e.value) == "phnsw error -1: phnsw_search_batch_radius: max_out must be 1..1024 (got %d)" % max_out
        with pytest.raises(ph.PhnswError) as e:
            hix.search_radius_device(4, ph.SearchParameters(*SP), 8, max_out, 8, 8, 8, 8, qids=8)
        assert e.value.code == -1 and "phnsw_search_batch_radius_device: max_out" in str(e.value)
    with pytest.raises(ValueError):
        hix.search_radius(queries=q, qids=w["qids"][:4], radius=0.3)
    with pytest.raises(ValueError):
        hix.search_radius(queries=q)
    with pytest.raises(ph.PhnswError) as e:  # number_of_candidates past the queues, as everywhere
        hix.search_radius(queries=q, radius=0.3, sp=ph.SearchParameters(2048, 64, 2))
    assert e.value.code in (-1, -7)
    with pytest.raises(ph.PhnswError) as e:  # a stored query id at or past n: the host form refuses it
        hix.search_radius(qids=np.array([1, N], dtype=np.uint64), radius=0.3)
    assert e.value.code == -1
    with pytest.raises(ph.PhnswError) as e:  # no radius
        hix.search_radius_device(4, ph.SearchParameters(*SP), 0, 8, 8, 8, 8, 8, qids=8)
    assert e.value.code == -1 and "phnsw_search_batch_radius_device" in str(e.value)
    ids, d, ln, status = hix.search_radius(queries=np.zeros((0, 100), dtype=np.float32), radius=0.3)  # nq == 0: a no-op
    assert ids.shape == (0, 64) and len(status) == 0
    pix = world("pq", 128)[0]
    with pytest.raises(ph.PhnswError) as e:
        pix.search_radius(queries=np.zeros((2, 128), dtype=np.float32), radius=0.3)
    assert e.value.code == -7 and "phnsw_search_batch_radius:" in str(e.value)  # PHNSW_E_UNSUPPORTED
