"""CPU pins of tests/filter_scale_reference.py, the pure-Python pieces of tests/test_gpu_filter_scale.py, on hand-made
cases: the restated integer rules against figures worked out by hand from exact_slices.h, dense_plan.h and
hostpath.hip's plan_chunks, the popcount against bitmaps written bit by bit, the makers against their promises."""
import numpy as np

import filter_reference as fr
import filter_scale_reference as sr


def test_shapes_of_the_two_worlds():
    assert sr.words_of(70001) == 2188 == 2 * 1024 + 140 and sr.passes_of(70001) == 35 and 2188 - 34 * 64 == 12
    assert sr.trips(2188, sr.COUNT_THREADS) == 9 and sr.trips(2188, sr.PREFIX_WORDS) == 3
    assert sr.words_of(32768) == 1024 and sr.passes_of(32768) == 16 and sr.trips(1024, sr.PREFIX_WORDS) == 1
    assert sr.words_of(32769) == 1025 and sr.passes_of(32769) == 17 and sr.trips(1025, sr.PREFIX_WORDS) == 2
    assert sr.trips(600, sr.ROUTE_QUERIES) == 3 and sr.trips(256, sr.ROUTE_QUERIES) == 1 and sr.trips(0, 7) == 0


def test_slice_ranges():
    def sizes(slices):
        return [b - a for a, b in sr.slice_ranges(35, slices)]

    assert sr.slice_ranges(35, 1) == [(0, 35)]
    assert sr.slice_ranges(35, 2) == [(0, 17), (17, 35)]
    assert sizes(3) == [11, 12, 12] and sizes(4) == [8, 9, 9, 9] and sizes(6) == [5, 6, 6, 6, 6, 6]
    assert sorted(sizes(34)) == [1] * 33 + [2]
    assert sizes(35) == [1] * 35 and sizes(1000) == [1] * 35 and sizes(0) == [35]
    for s in (1, 2, 3, 4, 6, 34, 35, 1000):  # the ranges tile [0, 35)
        r = sr.slice_ranges(35, s)
        assert r[0][0] == 0 and r[-1][1] == 35 and all(a[1] == b[0] for a, b in zip(r, r[1:]))
    assert sr.slice_ranges(3, 1000) == [(0, 1), (1, 2), (2, 3)]


def test_node_chunks():
    assert sr.node_chunks(8191) == [8191] and sr.node_chunks(8192) == [8192] and sr.node_chunks(8193) == [8192, 1]
    assert sr.node_chunks(20000) == [8192, 8192, 3616]
    assert sr.node_chunks(70001) == [8192] * 8 + [4465]
    assert sr.node_chunks(35001) == [8192] * 4 + [2233]
    assert sr.node_chunks(0) == []
    assert sr.node_chunks(300, 100) == [128, 128, 44]  # rounded up to a multiple of 64
    for knob in (65536, 100000):  # the clamp
        assert sr.node_chunks(65536, knob) == [65536] and sr.node_chunks(65537, knob) == [65536, 1]
        assert sr.node_chunks(70001, knob) == [65536, 4465]


def test_host_chunk_bounds():
    assert sr.host_chunk_bounds(65, 0, 5, 7) == [0, 5, 11, 18, 25, 31, 38, 45, 51, 58, 65]
    assert max(np.diff(sr.host_chunk_bounds(65, 0, 5, 7))) <= 7
    assert sr.host_chunk_bounds(65, 4000000000, 1024, 4096) == [0, 65]
    assert sr.host_chunk_bounds(3, 0, 5, 7) == [0, 3, 3]
    assert sr.host_chunk_bounds(10000, 6144, 1024, 4096) == [0, 1024, 4016, 7008, 10000]


def test_popcount_candidates():
    n = 70  # three words, six bits of the last one
    words = np.array([0x80000001, 0, 0xFFFFFFFF], dtype=np.uint32)
    assert sr.popcount_candidates(words, n).tolist() == [2 + 6]  # ids 0, 31, 64..69; 70..95 are past n
    assert sr.popcount_candidates(words, n, members=np.arange(n) % 2 == 0).tolist() == [1 + 3]  # 0; 64, 66, 68
    wide = np.array([[1, 2, 4, 0xFFFFFFFF, 0xFFFFFFFF], [0, 0, 0x3F, 7, 7], [0xFFFFFFFF] * 5], dtype=np.uint32)
    assert sr.popcount_candidates(wide, n).tolist() == [3, 6, 70]  # the words between the bitmaps are no one's
    assert sr.popcount_candidates(np.zeros(3, dtype=np.uint32), n).tolist() == [0]
    rng = np.random.default_rng(1)
    allow = rng.random((5, 1000)) < 0.3
    np.testing.assert_array_equal(sr.popcount_candidates(fr.pack(allow), 1000), allow.sum(axis=1))
    even = np.arange(1000) % 2 == 0
    np.testing.assert_array_equal(sr.popcount_candidates(fr.pack(allow), 1000, even), (allow & even).sum(axis=1))


def test_words_mask():
    m = sr.words_mask(70, [0, 2])
    assert m.shape == (70,) and np.nonzero(m)[0].tolist() == list(range(32)) + list(range(64, 70))
    assert not sr.words_mask(70, []).any()
    np.testing.assert_array_equal(fr.pack(sr.words_mask(100, [1, 3])), np.array([0, 0xFFFFFFFF, 0, 0xF], dtype=np.uint32))


def test_exactly_of():
    for count in (0, 1, 3, 50, 100):
        m = sr.exactly_of(100, count, seed=count, first=(99, 0, 50, 7))
        assert m.shape == (100,) and m.sum() == count
        assert m[[99, 0, 50, 7][:count]].all()
    assert (sr.exactly_of(100, 40, 1) != sr.exactly_of(100, 40, 2)).any()
    np.testing.assert_array_equal(sr.exactly_of(100, 40, 1), sr.exactly_of(100, 40, 1))


def test_the_batch_arrangers():
    assert sr.cycle_counts(7, [5, 0, 9]) == [5, 0, 9, 5, 0, 9, 5]
    assert sr.arranged_counts(7, 3, [1, 2], [8]) == [1, 2, 1, 8, 8, 8, 8]
    assert sr.arranged_counts(4, 0, [1], [8, 9]) == [8, 9, 8, 9]
    counts = [0, 1, 10, 49, 50, 3]
    allow = sr.bitmaps_of(50, counts, seed=4)
    assert allow.shape == (6, 50) and allow.sum(axis=1).tolist() == counts
    assert (sr.bitmaps_of(50, [10, 10], 4)[0] != sr.bitmaps_of(50, [10, 10], 4)[1]).any()  # drawn per query
    pool = np.arange(0, 50, 2)
    part = sr.bitmaps_of(50, [0, 7, 25], seed=5, pool=pool)
    assert part.sum(axis=1).tolist() == [0, 7, 25] and not part[:, 1::2].any()
