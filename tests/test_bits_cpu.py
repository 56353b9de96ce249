"""The premise the GPU tests of the bits row store stand on, proved on the CPU: a distance of the bits store is defined
from a popcount (tests/bits_reference.py), and the UNCHANGED oracle over the +1 / -1 rows with the +1 / -1 query gives
the same float, bit for bit, in every summation mode -- every partial sum is an integer of magnitude at most 4 * 1536
< 2^24, which f32 holds exactly in any order.  So the oracle the repository already owns pins the new store.

These tests need no GPU and no new library code: they pass before the bits store exists, by design (the GPU tests in
tests/test_gpu_bits*.py are the ones that fail without it)."""
import numpy as np
import pytest

import oracle

import bits_reference as br
from bits_reference import bit_edge_rows

METRICS = [oracle.METRIC_COSINE_HALF, oracle.METRIC_ONE_MINUS_DOT, oracle.METRIC_L2]
SUM_MODES = [oracle.SUM_SEQ, oracle.SUM_BLOCKED64, oracle.SUM_SEQFMA]
DIMS = [6, 100, 256, 768, 1536]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def world(dim, n=64):
    rng = np.random.default_rng(1000 + dim)
    rows = np.concatenate([bit_edge_rows(dim), rng.standard_normal((n, dim)).astype(np.float32)])
    q = np.concatenate([rng.standard_normal((5, dim)).astype(np.float32), bit_edge_rows(dim)[:6]])
    return rows, q


def test_the_rule_and_the_packing_on_the_edge_rows():
    for dim in (1, 6, 31, 32, 33, 100, 257):                      # dims that are no multiple of 4 / 32 among them
        rows = bit_edge_rows(dim)
        w = br.pack(rows)
        assert w.shape == (len(rows), (dim + 31) // 32)
        assert not w[0].any() and not w[1].any() and not w[2].any()
        full = np.zeros_like(w[3])
        for j in range(dim):
            full[j >> 5] |= np.uint32(1) << np.uint32(j & 31)
        np.testing.assert_array_equal(w[3], full)                 # every component, and no padding bit
        np.testing.assert_array_equal(w[4], full)
        held = br.unpack(w, dim)
        np.testing.assert_array_equal(held, np.where(rows < 0, -1.0, 1.0).astype(np.float32))
        np.testing.assert_array_equal(br.pack(held), w)           # the +-1 view packs to the same words
        for i in range(5, len(rows)):
            j = int(np.flatnonzero(rows[i] < 0)[0])
            want = np.zeros_like(w[i])
            want[j >> 5] = np.uint32(1) << np.uint32(j & 31)
            np.testing.assert_array_equal(w[i], want)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
def test_oracle_distances_equal_the_restatement_in_every_sum_mode(dim, metric):
    rows, q = world(dim)
    w = br.pack(rows)
    held = br.unpack(w, dim)
    ix = oracle.Index(held, metric=metric)
    for qv in q:
        want = br.distances(w, br.pack(qv)[0], dim, metric)
        sq = br.signed_query(qv)
        for mode in SUM_MODES:
            got = np.array([ix.distance(sq, held[i], mode) for i in range(len(held))], dtype=np.float32)
            np.testing.assert_array_equal(bits(got), bits(want))
    # a stored query is its row
    want = br.distances(w, w[7], dim, metric)
    for mode in SUM_MODES:
        got = np.array([ix.distance(held[7], held[i], mode) for i in range(len(held))], dtype=np.float32)
        np.testing.assert_array_equal(bits(got), bits(want))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
def test_oracle_searches_agree_between_blocked_and_sequential_order(dim, metric):
    n = 600
    norm = metric != oracle.METRIC_L2
    rows = oracle.synth_rows(0, n, dim, normalize=norm)[:, :dim]
    held = br.unpack(br.pack(rows), dim)
    bp = oracle.default_build_params(seed=1)
    g = oracle.Index.generate(np.ascontiguousarray(rows), np.arange(n), bp, metric=metric, sum_mode=oracle.SUM_BLOCKED64)
    q = br.signed_query(oracle.synth_rows(2 ** 32, 20, dim, normalize=norm)[:, :dim])
    qids = np.arange(0, n, 37, dtype=np.uint64)
    results = []
    for mode in (oracle.SUM_BLOCKED64, oracle.SUM_SEQ):
        ix = oracle.Index(held, metric=metric, sum_mode=mode)
        for l in range(g.layer_count):
            nodes, nb = g.layer(l)
            ix.push_layer(nodes, nb, nb.shape[1] if nb.ndim == 2 else len(nb) // len(nodes))
        results.append((ix.search(queries=q, sp=(48, 48, 2), stats=True), ix.search(qids=qids, sp=(48, 48, 2), stats=True)))
    for a, b in zip(results[0], results[1]):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(bits(a[1]), bits(b[1]))
        np.testing.assert_array_equal(a[2], b[2])
        np.testing.assert_array_equal(a[3], b[3])
    # and the distances the searches returned are the restatement's
    ids, d, ln, _ = results[0][0]
    w = br.pack(rows)
    for i in range(len(q)):
        m = int(ln[i])
        np.testing.assert_array_equal(bits(d[i, :m]), bits(br.distances(w[ids[i, :m].astype(np.int64)], br.pack(q[i])[0], dim, metric)))


def test_rerank_restatement_orders_by_distance_then_id():
    ids = np.array([[9, 3, 7, 1, 5]], dtype=np.uint64)
    d = np.array([[0.5, 0.25, 0.25, -0.0, 0.0]], dtype=np.float32)
    out_ids, out_d, out_len = br.rerank(ids, np.array([5]), d, 4)
    np.testing.assert_array_equal(out_ids[0], [1, 5, 3, 7])
    np.testing.assert_array_equal(out_len, [4])
    out_ids, out_d, out_len = br.rerank(ids, np.array([2]), d, 4)
    np.testing.assert_array_equal(out_ids[0, :2], [3, 9])
    assert out_len[0] == 2 and out_ids[0, 2] == 0xFFFFFFFFFFFFFFFF
