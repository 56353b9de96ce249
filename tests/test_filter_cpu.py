"""CPU checks of the filtered search's test reference and of the Python-side packing.

tests/filter_reference.py restates search_layers / closest_vectors / closest_nodes with an arbitrary `include`.  Here the
unchanged oracle pins it on built multi-layer indexes, in both summation modes, for raw and stored queries: with every id
allowed it must equal oracle.search, and with exactly one id disallowed per query it must equal
oracle.search(exclude=that id) -- ids, distance bits, lengths and both counters."""
import numpy as np
import pytest

import oracle
from parallel_hnsw_amd.hnsw import pack_allow

import filter_reference as fr
from value_families import bits, graph_over

N, NQ = 1500, 24


def same(a, b):
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(bits(a[1]), bits(b[1]))
    np.testing.assert_array_equal(a[3], b[3])


_made = {}


def built(dim):
    if dim not in _made:
        rows = oracle.synth_rows(0, N, dim)
        ix = graph_over(rows, dim, oracle.METRIC_COSINE_HALF)
        assert ix.layer_count >= 3
        _made[dim] = (ix, fr.layers_of(ix), oracle.synth_rows(2 ** 32, NQ, dim)[:, :dim].copy())
    return _made[dim]


@pytest.mark.parametrize("mode", [oracle.SUM_SEQ, oracle.SUM_BLOCKED64])
@pytest.mark.parametrize("dim,sp", [(6, (64, 16, 2)), (100, (96, 96, 3))])
def test_restatement_is_the_oracle(dim, sp, mode):
    ix, layers, q = built(dim)
    ix.set_sum_mode(mode)
    try:
        qids = np.arange(3, N, N // NQ, dtype=np.uint64)[:NQ]
        for kw, D in ((dict(queries=q), fr.distance_rows(ix, queries=q, mode=mode)),
                      (dict(qids=qids), fr.distance_rows(ix, qids=qids, mode=mode))):
            plain = ix.search(sp=sp, stats=True, **kw)
            # every id allowed: the unfiltered search
            same(fr.search(ix, D, sp, allow=np.ones(N, dtype=bool), layers=layers), plain)
            same(fr.search(ix, D, sp, layers=layers), plain)
            # one bit cleared per query (a result of the unfiltered search, so that it matters) = exclude
            ex = plain[0][np.arange(NQ), np.arange(NQ) % 5 + 1].copy()
            allow = np.ones((NQ, N), dtype=bool)
            allow[np.arange(NQ), ex.astype(np.int64)] = False
            excl = ix.search(sp=sp, exclude=ex, stats=True, **kw)
            assert (excl[0] != plain[0]).any()
            same(fr.search(ix, D, sp, allow=allow, layers=layers), excl)
            same(fr.search(ix, D, sp, exclude=ex, layers=layers), excl)
    finally:
        ix.set_sum_mode(oracle.SUM_SEQ)


def test_packing_of_bool_masks():
    rng = np.random.default_rng(5)
    for n in (1, 31, 32, 33, 1000):
        nw = (n + 31) // 32
        a = rng.random(n) < 0.4
        words, stride = pack_allow(a, n, 7)
        assert stride == 0 and words.dtype == np.uint32 and words.shape == (nw,)
        for v in range(n):
            assert bool((int(words[v >> 5]) >> (v & 31)) & 1) == bool(a[v])
        assert n % 32 == 0 or int(words[-1]) >> (n % 32) == 0  # bits at or past n are clear
        np.testing.assert_array_equal(words, fr.pack(a))
        b = rng.random((7, n)) < 0.5
        words, stride = pack_allow(b, n, 7)
        assert stride == nw and words.shape == (7, nw) and words.flags.c_contiguous
        np.testing.assert_array_equal(words, fr.pack(b))
        for q in (0, 6):
            for v in range(n):
                assert bool((int(words[q, v >> 5]) >> (v & 31)) & 1) == bool(b[q, v])


def test_packing_accepts_words_and_rejects_other_shapes():
    n, nq = 70, 3
    w = np.array([1, 2, 3], dtype=np.uint32)
    words, stride = pack_allow(w, n, nq)
    assert stride == 0 and words is not None and (words == w).all()
    w2 = np.arange(12, dtype=np.uint32).reshape(3, 4)  # per-query bitmaps wider than ceil(n/32): the stride says so
    words, stride = pack_allow(w2, n, nq)
    assert stride == 4 and (words == w2).all()
    assert pack_allow(None, n, nq) == (None, 0)
    for bad in (np.ones(n + 1, dtype=bool), np.ones((nq + 1, n), dtype=bool), np.zeros(2, dtype=np.uint32),
                np.zeros((nq, 2), dtype=np.uint32)):
        with pytest.raises(ValueError):
            pack_allow(bad, n, nq)
    with pytest.raises(TypeError):
        pack_allow(np.ones(n, dtype=np.int64), n, nq)
