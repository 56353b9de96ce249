"""Run time on an MI355X: 4.5 s together with tests/test_gpu_grouped_shim.py (3 cases, first clean run); run it under
`timeout -k 10 30`.

phnsw_search_exact_grouped[_device] (filter_grouped.hip) at the smallest shapes where its loops over the bitmap turn
more than once, on the worlds of tests/test_gpu_filter_scale.py: World A (N = 70 001 rows, 2188 bitmap words: three
trips of the per-group prefix kernel, nine of the count loop, more candidates than one node chunk holds, so the running
top-k is carried between node chunks) and World B at n = 32 769 (word 1024 holds one valid bit, and the bitmaps set
it).  Both yardsticks of tests/test_gpu_exact_grouped.py; ids, distance bits, lengths and status, no tolerance."""
import numpy as np
import pytest

import filter_scale_reference as sr
from test_gpu_exact_grouped import ALL, check
from test_gpu_filter_scale import DUPS, N, NB, NQX, NW, mask, world, world_b

pytestmark = pytest.mark.gpu


def test_four_densities_over_three_prefix_trips():
    w = world("f32", 24)
    masks = np.stack([mask(d, N, 60 + i) for i, d in enumerate((0.001, 0.02, 0.5))] + [np.ones(N, dtype=bool)])
    masks[:, DUPS] = True  # ties in every trip of the prefix kernel and across node chunks: the ids decide
    masks[:, N - 1] = True
    counts = masks.sum(axis=1)
    assert sr.trips(NW, sr.PREFIX_WORDS) == 3 and counts[0] < 200 and counts[2] > 4 * 8192 and counts[3] == N
    of = np.arange(NQX) % 4  # interleaved groups of 16 or 17 queries
    got = check(w, masks, of, k=64)
    for form in (0, 1):
        np.testing.assert_array_equal(got[form][0][0, :40], DUPS.astype(np.uint64))  # query 0 is the duplicated row


def test_one_valid_bit_in_the_last_word():
    n = NB[1]
    w = world_b(n)
    assert n % 32 == 1 and sr.words_of(n) == 1025
    few = np.zeros(n, dtype=bool)
    few[[0, 31, 32, n - 2, n - 1]] = True
    half = mask(0.5, n, 71)
    half[n - 1] = True
    last = np.zeros(n, dtype=bool)
    last[n - 1] = True
    masks = np.stack([few, half, last])
    of = np.arange(16) % 4
    of[of == 3] = ALL
    got = check(w, masks, of, k=10)
    for form in (0, 1):
        np.testing.assert_array_equal(got[form][2], np.array([5, 10, 1, 10] * 4))
        assert (got[form][0][of == 2, 0] == n - 1).all()
