"""The premises of tests/test_gpu_filter_value_edges.py, proved on the references alone (no GPU, no library): the
oracle's distance matrix lies within the a-priori bound of float64 for every world, the restated exact top-k agrees with
the float64 second opinion, and what the GPU file asserts to occur -- negative distances, the whole-range tie, equal
lattice rows next to each other, +inf tails, both routes, walks without +inf -- occurs in the restatements."""
import numpy as np
import pytest

import exact_filter_reference as xr
import filter_auto_reference as ar
import filter_reference as fr
import filter_value_worlds as fw
import value_families as vf
from filter_value_worlds import N, NQ, NS, WORLDS, world_id


def test_the_shape_of_the_worlds():
    assert len(WORLDS) == len(set(WORLDS)) == 156
    assert fw.ROUTED_WORLDS[0] in WORLDS and all(w in WORLDS for w in fw.WALK_WORLDS + fw.INF_WORLDS)
    assert len(fw.QIDS) == NS and len(set(fw.QIDS.tolist())) == NS and 5 in fw.QIDS and 2 in fw.QIDS
    rows = fw.family_rows("lattice", 100)[0]
    assert not rows[2].any() and rows[5].any()
    for a, b in fw.COPIES:
        assert (rows[a] == rows[b]).all() and rows[a].any() and b == a + 3
    # the per-query bitmaps and the small one cross the 2 048-id border and reach the ragged last word
    for m in (fw.shared_bitmap(), fw.small_bitmap()) + tuple(fw.per_query_bitmaps()[:4]):
        assert m[:2048].any() and m[2048:].any() and m[(fw.NW - 1) * 32:].any()
    counts = fw.routed_bitmaps().sum(axis=1)
    first = ar.first_graph_count(fw.ROUTED_EF, fw.ROUTED_K, N)
    assert first == 329 and (counts[0::2] >= first).all() and (counts[1::2] < first).all() and (counts > 1).all()


@pytest.mark.parametrize("key", WORLDS, ids=world_id)
def test_the_oracle_lies_within_the_bound_and_exact_rows_agree_with_float64(key):
    w = fw.world(*key)
    assert w["Dq"].shape == (NQ, N) and w["Ds"].shape == (NS, N)
    for form, D in ((0, w["Dq"]), (1, w["Ds"])):
        R64, B, R32 = fw.opinion(*key)[form]
        fin = np.isfinite(R32)
        np.testing.assert_array_equal(np.isinf(D) & (D > 0), ~fin)  # +inf exactly where the f32 sum overflows, never NaN
        assert (np.abs(D[fin].astype(np.float64) - R64[fin]) <= B[fin]).all()
        if key[0] == "lattice":
            np.testing.assert_array_equal(vf.bits(D + np.float32(0.0)), vf.bits(R32 + np.float32(0.0)))
        if key[0] != "l2_overflow":
            assert fin.all()
    if key[0] == "tiny" and key[1] != 2:
        want = np.float32(0.5 if key[1] == 0 else 1.0)
        assert (vf.bits(w["Dq"]) == vf.bits(want)).all() and (vf.bits(w["Ds"]) == vf.bits(want)).all()
    negative = {0: False, 1: False}
    copies = 0
    for name, allow, exclude, k in fw.scan_cases(w):
        for form in (0, 1):
            D, a = fw.of_form(w, form, allow)
            ref = xr.exact_topk(D, a, exclude[form], None, k)
            fw.second_opinion(w, form, ref, a, exclude[form], k)
            if name == "no filter k 64":
                negative[form] = fw.has_negative(ref)
            if key[0] == "tiny" and key[1] != 2:
                fw.assert_whole_tie(w, ref, a, exclude[form], k)
                if name == "no filter k 1024" and form == 0:
                    np.testing.assert_array_equal(ref[0], np.tile(np.arange(1024, dtype=np.uint64), (NQ, 1)))
            if key[0] == "lattice" and k == 1024:
                assert (ref[2] == a.sum()).all()
                copies += fw.assert_copies_adjacent(ref)
    if fw.expects_negative(w):
        assert negative[0] and negative[1]
    if key[0] == "lattice":
        assert copies == (NQ + NS) * len(fw.COPIES)


@pytest.mark.parametrize("key", fw.INF_WORLDS, ids=world_id)
def test_inf_tails_and_routes_on_l2_overflow(key):
    w = fw.world(*key)
    allow = fw.inf_bitmap(w)
    assert len(w["big_rows"]) > fw.INF_K and allow.sum() == len(w["big_rows"]) + 5
    assert ((np.isinf(w["Dq"])).mean() > 0.01) and fw.entry_vector(w) not in w["big_rows"]
    ref = xr.exact_topk(w["Dq"], allow, None, None, fw.INF_K)
    assert fw.assert_inf_tail(w, ref, allow, fw.INF_K, set(w["big_q"].tolist())) == NQ  # five finite candidates, k = 10
    fw.second_opinion(w, 0, ref, allow, None, fw.INF_K)
    ok = np.nonzero(fw.walkable(w, 0))[0]
    assert len(ok) == NQ - len(w["big_q"]) and not np.isin(w["big_q"], ok).any()
    assert ar.first_graph_count(fw.INF_EF, fw.INF_K, N) == 21 <= allow.sum()
    routed = fw.restated_routed(w, 0, allow, fw.INF_EF, fw.INF_K, rows=ok)
    assert (routed[3] == ar.GRAPH_THEN_SCAN).all()
    ar.assert_complete(routed, N, fw.INF_K, allow)
    for x, y in zip(routed[:3], ref[:3]):
        np.testing.assert_array_equal(vf.bits(x) if x.dtype == np.float32 else x, (vf.bits(y) if y.dtype == np.float32 else y)[ok])
    walk = fr.strict(fw.restated_walk(w, 0, (fw.INF_EF, fw.INF_EF, 2), allow, rows=ok), allow)
    print("strict restated walk, entries per query:", walk[2].tolist())
    assert (walk[2] < fw.INF_K).all()


@pytest.mark.parametrize("key", fw.ROUTED_WORLDS, ids=world_id)
def test_both_routes_occur_in_the_restated_routed_call(key):
    w = fw.world(*key)
    allow = fw.routed_bitmaps()
    for form in (0, 1):
        D, a = fw.of_form(w, form, allow)
        routed = fw.restated_routed(w, form, a, fw.ROUTED_EF, fw.ROUTED_K)
        assert (routed[3][1::2] == ar.SCAN).all() and (routed[3][0::2] != ar.SCAN).all()
        assert (routed[3] == ar.GRAPH).any()
        ar.assert_complete(routed, N, fw.ROUTED_K, a)


@pytest.mark.parametrize("key", [w for w in fw.WALK_WORLDS if w[2] == 100 and w[3] == "f32"], ids=world_id)
def test_the_restated_walk_never_returns_inf(key):
    """on every family (l2_overflow is where +inf is evaluated at all), strict or not, both queue widths"""
    w = fw.world(*key)
    allow = fw.mask(0.5, N, 306)
    evaluated_inf = False
    for sp in (fw.SP_WIDE, fw.SP_NARROW):
        for form in (0, 1):
            ok = np.nonzero(fw.walkable(w, form))[0]
            res = fw.restated_walk(w, form, sp, allow, fw.own_ids(form), rows=ok)
            valid = np.arange(sp[0])[None, :] < res[2][:, None]
            assert np.isfinite(res[1][valid]).all() and (res[2] >= 1).all()
            fw.second_opinion_distances(w, form, *res[:3], rows=ok)
            evaluated_inf |= bool(np.isinf((w["Dq"], w["Ds"])[form][ok]).any())
    assert evaluated_inf == (key[0] == "l2_overflow")
