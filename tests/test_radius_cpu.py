"""The radius search without a GPU: the integer rules of parallel_hnsw_amd/csrc/radius_plan.h in a stand-alone host program
under AddressSanitizer and UBSan (tests/cpp/test_radius_plan.cpp, compiled with g++ and run as a process of its own;
nothing loaded into Python), and the numpy restatement the GPU tests compare against (tests/radius_reference.py) pinned
to the restatement of the exact top-k it extends (tests/exact_filter_reference.py)."""
import functools
import os
import subprocess

import numpy as np

import oracle

import exact_filter_reference as xr
import filter_reference as fr
import radius_reference as rr
import value_families as vf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_radius_plan_rules_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_radius_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_radius_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout


def matrix(nq=9, n=300, seed=5):
    """distances with ties (a grid of 40 values), a +inf, a NaN and a -0.0 in every row"""
    rng = np.random.default_rng(seed)
    D = (rng.integers(1, 41, (nq, n)) / np.float32(8)).astype(np.float32)
    D[:, 7], D[:, 11], D[:, 13] = np.inf, np.nan, -0.0
    return D


def test_the_restatement_is_the_exact_top_k_cut_at_the_radius():
    D = matrix()
    nq, n = D.shape
    allow = np.random.default_rng(1).random(n) < 0.6
    allow[[7, 11, 13]] = True
    members = np.arange(n) % 5 != 0
    exclude = np.arange(nq, dtype=np.uint64) * 3
    radius = np.array([0.5, 1.0, 2.5, 5.0, 5.125, np.inf, 0.0, -1.0, np.nan], dtype=np.float32)
    for a, e, m in ((None, None, None), (allow, None, None), (allow, exclude, members)):
        first, ids, d = rr.exact_radius(D, radius, a, e, m)
        ti, td, tl = xr.exact_topk(D, a, e, m, n)
        assert first[0] == 0 and first[nq] == len(ids) == len(d) and (np.diff(first.astype(np.int64)) >= 0).all()
        for q in range(nq):
            si, sd = rr.segment((first, ids, d), q)
            row_d = td[q, :int(tl[q])]
            with np.errstate(invalid="ignore"):
                keep = (row_d < radius[q]) if radius[q] > 0 else np.zeros(len(row_d), dtype=bool)
            # the top-k row is ascending, NaN last: what is inside the radius is a prefix of it
            assert not keep.any() or keep[:keep.sum()].all()
            np.testing.assert_array_equal(si, ti[q, :keep.sum()])
            np.testing.assert_array_equal((sd + np.float32(0)).view(np.uint32), (row_d[:keep.sum()] + np.float32(0)).view(np.uint32))
            assert not np.isin(si, [7, 11]).any()  # +inf and NaN: never inside a radius, not even +inf
            assert not (sd.view(np.uint32) == 0x80000000).any()  # -0.0 is reported as +0.0
    first, ids, d = rr.exact_radius(D, radius)
    assert first[6] == first[7] == first[8] == first[9]  # 0, -1 and NaN match nothing
    assert first[6] - first[5] == n - 2  # +inf: everything but the +inf and the NaN column
    assert 13 in rr.segment((first, ids, d), 0)[0]  # -0.0 < 0.5


def test_strictness_and_the_next_float_up():
    D = matrix(nq=4, n=200, seed=9)
    for m in (0, 1, 63, 64, 65, 150):
        r = rr.mth_smallest(D, m)
        lo = rr.exact_radius(D, r)
        hi = rr.exact_radius(D, np.nextafter(r, np.float32(np.inf)))
        for q in range(4):
            row = np.sort(D[q][np.isfinite(D[q])])
            assert len(rr.segment(lo, q)[0]) == (row < r[q]).sum() <= m
            assert len(rr.segment(hi, q)[0]) == (row <= r[q]).sum() > m
    np.testing.assert_array_equal(rr.exact_radius(D, 2.0)[1], rr.exact_radius(D, np.full(4, 2.0))[1])  # a scalar broadcasts


# ---------------------------------------------------------------- the walk's restatement against the unchanged oracle
@functools.lru_cache(maxsize=None)
def small_world(n=600, dim=16, metric=oracle.METRIC_COSINE_HALF):
    rows = oracle.synth_rows(0, n, dim)
    oix = vf.graph_over(rows, dim, metric)
    assert oix.layer_count >= 2
    q = np.ascontiguousarray(oracle.synth_rows(2 ** 32, 24, dim)[:, :dim])
    Dq = vf.oracle_matrix(rows, q, metric, oracle.SUM_BLOCKED64)
    Dself = vf.oracle_matrix(rows, np.ascontiguousarray(rows[:, :dim]), metric, oracle.SUM_BLOCKED64)
    return oix, fr.layers_of(oix), q, Dq, Dself


def test_the_growth_loop_is_threshold_nn():
    """seeded with (self, 0.0) at capacity initial_search_depth on the bottom layer, the loop must give what
    oracle.Index.threshold_nn gives: ids, distances, lengths -- in a world where queues double twice"""
    oix, layers, _, _, Dself = small_world()
    bottom = layers[-1]
    nodes = bottom[0]
    n = len(nodes)
    isd, pd = 4, 2
    threshold = np.float32(np.median(np.sort(Dself, axis=1)[:, 14]))  # about 14 rows inside: 4 -> 8 -> 16 for many
    ids, d, ln = oix.threshold_nn(float(threshold), pd, isd, max_out=n)
    most = 0
    for i in range(n):
        queue = oracle.PriorityQueue.new(isd)
        queue.merge_pairs([(i, 0.0)])
        queue, trace = rr.growth_loop(bottom, queue, Dself[int(nodes[i])], threshold, pd, [0, 0])
        res = rr.queue_result(bottom, queue, threshold, skip_node=i)
        most = max(most, trace["capacity"])
        assert len(res) == int(ln[i]), i
        np.testing.assert_array_equal(np.array([v for v, _ in res], dtype=np.uint64), ids[i, :len(res)])
        np.testing.assert_array_equal(np.array([x for _, x in res], dtype=np.float32).view(np.uint32), d[i, :len(res)].view(np.uint32))
    assert most >= 4 * isd  # at least one queue doubled twice


def test_the_full_walk_is_the_search_row_cut_at_the_radius():
    """with a radius at or below the last distance of oracle.search's row the loop runs once, and the walk's result is
    that row cut at d < r (exclude = None)"""
    oix, layers, q, Dq, _ = small_world()
    for sp in ((16, 16, 2), (64, 8, 3)):
        ids, d, ln = oix.search(queries=q, sp=sp)
        for i in range(len(q)):
            row_i, row_d = ids[i, :int(ln[i])], d[i, :int(ln[i])]
            for r in (row_d[-1], row_d[len(row_d) // 2], np.nextafter(row_d[0], np.float32(np.inf))):
                gi, gd, glen, status, _, trace = rr.search_radius_one(layers, Dq[i], sp, r, max_out=sp[0])
                keep = int((row_d < r).sum())
                assert status == 0 and glen == keep and trace["calls"] == 1 and trace["capacity"] == sp[0]
                np.testing.assert_array_equal(gi[:keep], row_i[:keep])
                np.testing.assert_array_equal(gd[:keep].view(np.uint32), row_d[:keep].view(np.uint32))
                assert (gi[keep:] == rr.EMPTY).all()
    # a zero, negative or NaN radius: no bottom-layer call, the counters of the upper layers only
    for r in (0.0, -1.0, np.nan):
        gi, gd, glen, status, stats, trace = rr.search_radius_one(layers, Dq[0], (16, 16, 2), r)
        assert glen == 0 and status == 0 and trace["calls"] == 0 and (gi == rr.EMPTY).all()
        upper = [1, 0]
        cand = oracle.PriorityQueue.new(16)
        cand.insert(int(layers[0][0][0]), Dq[0][int(layers[0][0][0])])
        for layer in layers[:-1]:
            cand.merge_pairs(fr.closest_vectors(layer, cand, 16, 2, lambda v: True, Dq[0], upper))
        assert stats == upper
