"""Run time on an MI355X: 58 s (371 cases, the slowest 0.74 s); run it under `timeout -k 10 174`, three times that.

The filtered and exact top-k calls on value edges, all three metrics: the exact scan (search_exact_filtered,
filter_exact.hip), the shared-bitmap distance table with its select (search_exact_shared, filter_dense.hip), the
allow-list walk (search_batch_filtered, search_filtered.hip) and the routed call (search_filtered, filter_auto.hip) over
f32, f16 and i8 stores of the families of tests/value_families.py -- negative and huge distances, exact ties over the
whole id range, cancelling sums, subnormal products and L2 sums that overflow to +inf -- at N = 2100 rows
(tests/filter_value_worlds.py: two scan passes, the second ragged; one 2 048-id border in the candidate list).

Two yardsticks, neither made by the code under test, both for every case:
  1. the restatements (exact_filter_reference, filter_reference, filter_auto_reference) over the oracle's
     ORC_SUM_BLOCKED64 distances of the rows each store holds: ids, distance bits, lengths, routes, counters and status,
     bit for bit;
  2. float64 (filter_value_worlds.second_opinion): ref32 / topk64 on the lattice, ref64 within value_families.bound()
     elsewhere, for the returned entries and for the candidates left out.
tests/test_filter_value_edges_cpu.py proves on the references alone that what is asserted to occur here does occur.

+inf (l2_overflow): the exact calls return a candidate at +inf behind every finite one, in id order, in front of the
f32::MAX padding; the walk never returns one; so the routed call scans a query whose finite candidates are fewer than
min(k, candidates)."""
import functools

import numpy as np
import pytest

import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import filter_auto_reference as ar
import filter_reference as fr
import filter_value_worlds as fw
from filter_value_worlds import N, NQ, world_id
from test_gpu_exact_filter import device_exact, ring, same
from test_gpu_exact_shared import device_shared
from test_gpu_filter import device_search
from test_gpu_filter import same as same_walk
from test_gpu_filter_auto import device_auto
from test_gpu_i8q import env
from value_families import bits

pytestmark = pytest.mark.gpu

EMPTY = xr.EMPTY


# ---------------------------------------------------------------- the GPU side of a world
@functools.lru_cache(maxsize=None)
def stores(family, metric, dim, kind):
    """(f32 store, store of `kind`) over the family's rows; the rows it holds are the ones yardstick 1 was made from"""
    full = ph.VectorStore(fw.family_rows(family, dim)[0][:, :dim], metric=metric)
    store = {"f32": lambda f: f, "f16": ph.F16Store.from_full, "i8": ph.I8Store.from_full}[kind](full)
    np.testing.assert_array_equal(bits(store.read()), bits(fw.held_rows(family, dim, kind)[:, :dim]))
    return full, store


@functools.lru_cache(maxsize=None)
def ring_index(key):
    """the scan and the table never walk: a one-layer ring over every vector"""
    return ph.Hnsw.from_layers(stores(*key)[1], ring(np.arange(N)))


@functools.lru_cache(maxsize=None)
def graph_index(key):
    """the oracle's graph over the family's f32 rows, adopted over the store"""
    return ph.Hnsw.from_layers(stores(*key)[1], fw.graph(*key[:3]))


def queries_of(w, form, rows=None):
    x = w["q"] if form == 0 else w["qids"]
    x = x if rows is None else x[rows]
    return dict(queries=np.ascontiguousarray(x)) if form == 0 else dict(qids=x)


def cut(a, n):
    return None if a is None else a[:n]


def padded(got, k):
    past = np.arange(k)[None, :] >= got[2][:, None]
    assert (got[0][past] == EMPTY).all() and (bits(got[1])[past] == bits(xr.FMAX)).all()


def occurs(w, name, form, got, allow, exclude, k, seen):
    """what the CPU file proves the references to hold, asserted on the GPU's rows"""
    if name == "no filter k 64":
        seen["negative"] = seen.get("negative", 0) + fw.has_negative(got)
    if w["family"] == "tiny" and w["metric"] != 2:
        fw.assert_whole_tie(w, got, allow, exclude, k)
        if name == "no filter k 1024" and form == 0:
            np.testing.assert_array_equal(got[0], np.tile(np.arange(1024, dtype=np.uint64), (len(got[0]), 1)))
            seen["tie"] = True
    if w["family"] == "lattice" and k == 1024:
        assert (got[2] == allow.sum()).all()  # every candidate is returned
        seen["copies"] = seen.get("copies", 0) + fw.assert_copies_adjacent(got)


def occurred(w, seen, forms=2):
    if fw.expects_negative(w):
        assert seen["negative"] == forms
    if w["family"] == "tiny" and w["metric"] != 2:
        assert seen["tie"]
    if w["family"] == "lattice":
        assert seen["copies"] > 0 and seen["copies"] % len(fw.COPIES) == 0


# ---------------------------------------------------------------- A: the scan
@pytest.mark.parametrize("key", fw.WORLDS, ids=world_id)
def test_scan(monkeypatch, key):
    w, hix = fw.world(*key), ring_index(key)
    refs, seen = {}, {}
    for slices in ("1", "2"):
        with env(monkeypatch, PHNSW_EXACT_SLICES=slices):
            for name, allow, exclude, k in fw.scan_cases(w):
                for form in (0, 1):
                    D, a = fw.of_form(w, form, allow)
                    e, kw = exclude[form], queries_of(w, form)
                    if (name, form) not in refs:
                        refs[name, form] = xr.exact_topk(D, a, e, None, k)
                    ref = refs[name, form]
                    got = hix.search_exact_filtered(allow=a, exclude=e, k=k, **kw)
                    same(got, ref)
                    padded(got, k)
                    dv = device_exact(hix, k, allow=a, exclude=e, **kw)
                    assert not dv[3].any()
                    same(dv, ref)
                    if slices == "1":
                        fw.second_opinion(w, form, got, a, e, k)
                        occurs(w, name, form, got, a, e, k, seen)
    occurred(w, seen)


# ---------------------------------------------------------------- B: the shared table
def shared_case(w, hix, form, nq, allow, exclude, k, device=True):
    """one shared call, host and device form, against yardstick 1 and against the scan with stride 0 -> the host rows"""
    D, a = fw.of_form(w, form, allow, nq)
    e, kw = cut(exclude[form], len(D)), queries_of(w, form, slice(0, len(D)))
    ref = xr.exact_topk(D, a, e, None, k)
    got = hix.search_exact_shared(allow=a, exclude=e, k=k, **kw)
    same(got, ref)
    same(got, hix.search_exact_filtered(allow=a, exclude=e, k=k, **kw))
    padded(got, k)
    if device:
        dv = device_shared(hix, k, allow=a, exclude=e, **kw)
        assert not dv[3].any()
        same(dv, ref)
    return got, a, e


@pytest.mark.parametrize("key", fw.WORLDS, ids=world_id)
def test_shared_table(monkeypatch, key):
    w, hix = fw.world(*key), ring_index(key)
    cases = fw.scan_cases(w, per_query=False)
    seen = {}
    for knobs in ({}, dict(PHNSW_TINY_VALU="1")):
        with env(monkeypatch, **knobs):
            for name, allow, exclude, k in cases:
                # 40 raw queries: the matrix-core table where the store has one; 16: the vector-unit pass; 8 stored
                for form, nq in ((0, NQ), (0, 16), (1, fw.NS)):
                    got, a, e = shared_case(w, hix, form, nq, allow, exclude, k)
                    if not knobs:
                        fw.second_opinion(w, form, got, a, e, k)
                        if nq != 16:
                            occurs(w, name, form, got, a, e, k, seen)
    occurred(w, seen)
    if key[0] in ("tiny", "lattice"):
        # 64 candidates per table: the ties cross node-chunk borders between running top-k merges
        again = {}
        with env(monkeypatch, PHNSW_DENSE_NODES="64"):
            for name, allow, exclude, k in cases:
                if k == 1024 or name == "shared 0.3 k 64":
                    for form in (0, 1):
                        got, a, e = shared_case(w, hix, form, NQ, allow, exclude, k, device=False)
                        occurs(w, name, form, got, a, e, k, again)
        occurred(w, again)


@pytest.mark.parametrize("dim", [256, 768, 1536])
def test_the_one_minus_dot_table_on_the_matrix_cores(monkeypatch, capfd, dim):
    """metric 1 on `scaled`: 40 queries take the matrix-core table (the call says so under PHNSW_VERBOSE), 16 queries
    and PHNSW_TINY_VALU=1 the vector units; the rows are the yardstick's on all three"""
    key = ("scaled", 1, dim, "f32")
    w, hix = fw.world(*key), ring_index(key)
    allow, none = fw.shared_bitmap(), (None, None)
    for knobs, nq, cores in ((dict(), NQ, True), (dict(), 16, False), (dict(PHNSW_TINY_VALU="1"), NQ, False)):
        capfd.readouterr()
        with env(monkeypatch, PHNSW_VERBOSE="1", **knobs):
            got, a, e = shared_case(w, hix, 0, nq, allow, none, 10, device=False)
        err = capfd.readouterr().err
        assert "exact shared table" in err and ("matrix cores" in err) == cores, err
        fw.second_opinion(w, 0, got, a, e, 10)
        assert fw.has_negative(got)


# ---------------------------------------------------------------- C: the walk
@pytest.mark.parametrize("key", fw.WALK_WORLDS, ids=world_id)
def test_walk(key):
    w, gix = fw.world(*key), graph_index(key)
    evaluated_inf = False
    for sp in (fw.SP_WIDE, fw.SP_NARROW):
        spp = ph.SearchParameters(*sp)
        for density, seed in ((0.5, 306), (0.1, 307)):
            allow = fw.mask(density, N, seed)
            for form in (0, 1):
                ok = np.nonzero(fw.walkable(w, form))[0]
                e = None if form == 0 else fw.own_ids(form)[ok]
                kw = queries_of(w, form, ok)
                ref = fw.restated_walk(w, form, sp, allow, fw.own_ids(form), rows=ok)
                got = gix.search_batch_filtered(sp=spp, allow=allow, exclude=e, stats=True, **kw)
                same_walk(got, ref)  # ids, distance bits, lengths and the counters
                dv = device_search(gix, spp, allow=allow, exclude=e, **kw)
                assert not dv[4].any()
                same_walk(dv, ref)
                want = fr.strict(ref, allow)
                strict = gix.search_batch_filtered(sp=spp, allow=allow, exclude=e, strict=True, stats=True, **kw)
                same_walk(strict, want)
                dv = device_search(gix, spp, allow=allow, exclude=e, strict=True, **kw)
                assert not dv[4].any()
                same_walk(dv, want)
                valid = np.arange(sp[0])[None, :] < got[2][:, None]
                assert np.isfinite(got[1][valid]).all() and (bits(got[1][~valid]) == bits(xr.FMAX)).all()
                fw.second_opinion_distances(w, form, *got[:3], rows=ok)
                evaluated_inf |= bool(np.isinf((w["Dq"], w["Ds"])[form][ok]).any())
    assert evaluated_inf == (key[0] == "l2_overflow")


# ---------------------------------------------------------------- D: the routed call
@pytest.mark.parametrize("key", fw.ROUTED_WORLDS, ids=world_id)
def test_routed(key):
    w, gix = fw.world(*key), graph_index(key)
    ef, k = fw.ROUTED_EF, fw.ROUTED_K
    spp = ph.SearchParameters(ef, ef, 2)
    allow = fw.routed_bitmaps()
    for form in (0, 1):
        D, a = fw.of_form(w, form, allow)
        e, kw = fw.own_ids(form), queries_of(w, form)
        want = fw.restated_routed(w, form, a, ef, k, exclude=e)
        got = gix.search_filtered(sp=spp, allow=a, exclude=e, k=k, scan_below=1, route=True, **kw)
        print("routes", np.bincount(got[3], minlength=3).tolist(), "expected", np.bincount(want[3], minlength=3).tolist())
        np.testing.assert_array_equal(got[3], want[3])
        same(got, want)
        counts = gix.filter_count(a)
        for i in range(len(D)):  # c * 64 >= 10 * 2100 sends c >= 329 to the graph
            r = ar.rule(counts[i], 1, ef, k, N)
            assert got[3][i] == r or (got[3][i] == ar.GRAPH_THEN_SCAN and r == ar.GRAPH)
            assert r == (ar.SCAN if i % 2 else ar.GRAPH)
        assert (got[3] == ar.GRAPH).any() and (got[3][1::2] == ar.SCAN).all()
        ar.assert_complete(got, N, k, a, e)
        dv = device_auto(gix, spp, k, allow=a, exclude=e, scan_below=1, **kw)
        assert not dv[4].any()
        same(dv, want)
        np.testing.assert_array_equal(dv[3], want[3])
        fw.second_opinion_distances(w, form, *got[:3])
        if key[0] == "scaled":
            assert fw.has_negative(got)


# ---------------------------------------------------------------- E: +inf
@pytest.mark.parametrize("key", fw.INF_WORLDS, ids=world_id)
def test_candidates_at_inf(key):
    w, hix, gix = fw.world(*key), ring_index(key), graph_index(key)
    k, ef = fw.INF_K, fw.INF_EF
    allow = fw.inf_bitmap(w)
    replaced = set(w["big_q"].tolist())
    ref = xr.exact_topk(w["Dq"], allow, None, None, k)
    for got in (hix.search_exact_filtered(queries=w["q"], allow=allow, k=k), device_exact(hix, k, queries=w["q"], allow=allow),
                hix.search_exact_shared(queries=w["q"], allow=allow, k=k), device_shared(hix, k, queries=w["q"], allow=allow)):
        same(got, ref)
        assert (got[2] == k).all()
        assert fw.assert_inf_tail(w, got, allow, k, replaced) == NQ  # five finite candidates: every row has a +inf tail
        fw.second_opinion(w, 0, got, allow, None, k)
        assert len(got) == 3 or not got[3].any()
    # the routed call: the walk keeps the finite candidates only, fewer than k, so every query is scanned after it
    ok = np.nonzero(fw.walkable(w, 0))[0]
    assert len(ok) == NQ - len(replaced)
    spp = ph.SearchParameters(ef, ef, 2)
    kw = queries_of(w, 0, ok)
    want = fw.restated_routed(w, 0, allow, ef, k, rows=ok)
    got = gix.search_filtered(sp=spp, allow=allow, k=k, scan_below=1, route=True, **kw)
    assert (got[3] == ar.GRAPH_THEN_SCAN).all() and (want[3] == ar.GRAPH_THEN_SCAN).all()
    same(got, want)
    same(got, [x[ok] for x in ref])
    ar.assert_complete(got, N, k, allow)
    dv = device_auto(gix, spp, k, allow=allow, scan_below=1, **kw)
    assert not dv[4].any() and (dv[3] == ar.GRAPH_THEN_SCAN).all()
    same(dv, want)
    # the walk itself on this bitmap: finite entries only, as restated
    walk = fw.restated_walk(w, 0, (ef, ef, 2), allow, rows=ok)
    for strict, wanted in ((False, walk), (True, fr.strict(walk, allow))):
        got = gix.search_batch_filtered(sp=spp, allow=allow, strict=strict, stats=True, **kw)
        same_walk(got, wanted)
        valid = np.arange(ef)[None, :] < got[2][:, None]
        assert np.isfinite(got[1][valid]).all() and (not strict or (got[2] < k).all())
