"""CPU pins of tests/labeled_scale_reference.py, the pure-Python pieces of tests/test_gpu_labeled_scale.py, on hand-made
cases: the restated integer rules against figures worked out by hand from label_plan.h, exact_slices.h and the launcher
of filter_labeled.hip, the column makers against their promises."""
import numpy as np

import labeled_reference as lr
import labeled_scale_reference as ls


def test_batches_of_the_long_lists():
    assert [ls.batches(x) for x in (0, 1, 63, 64, 65, 128, 129)] == [0, 1, 1, 1, 2, 2, 3]
    assert ls.batches(70001) == 1094 and ls.last_batch_ids(70001) == 49 == 70001 - 1093 * 64
    assert ls.batches(69901) == 1093 and ls.last_batch_ids(69901) == 13
    assert ls.batches(25040) == 392 and ls.last_batch_ids(25040) == 16
    assert ls.batches(65536) == 1024 and ls.last_batch_ids(65536) == 64 and ls.last_batch_ids(0) == 0


def test_slice_count_and_ranges():
    assert ls.slice_count(5000, 69901) == 1093 and ls.slice_count(1093, 69901) == 1093 and ls.slice_count(7, 69901) == 7
    assert ls.slice_count(1094, 70001) == 1094 and ls.slice_count(392, 25040) == 392 and ls.slice_count(3, 0) == 1
    assert ls.slice_ranges(25040, 1) == [(0, 392)] and ls.slice_ranges(25040, 2) == [(0, 196), (196, 392)]
    assert [b - a for a, b in ls.slice_ranges(25040, 3)] == [130, 131, 131]
    assert [b - a for a, b in ls.slice_ranges(25040, 7)] == [56] * 7
    assert sorted(b - a for a, b in ls.slice_ranges(25040, 391)) == [1] * 390 + [2]
    assert ls.slice_ranges(70001, 1094) == [(s, s + 1) for s in range(1094)]
    # the clamp looks at the longest list: a list of 65 rows under 7 slices has two batches and five empty ranges
    assert ls.slice_ranges(65, 7) == [(0, 0), (0, 0), (0, 0), (0, 1), (1, 1), (1, 1), (1, 2)]
    for length in (1, 64, 65, 25040, 69901):  # the ranges tile the batches
        for s in (1, 2, 3, 7, 391, 392, 1093):
            r = ls.slice_ranges(length, s)
            assert r[0][0] == 0 and r[-1][1] == ls.batches(length) and all(a[1] == b[0] for a, b in zip(r, r[1:]))


def test_tile_of():
    assert ls.tile_query_lds(10, 24) == 96 + 160 + 512 + 256 + 16 == 1040
    assert ls.tile_of(10, 24) == 16 and ls.tile_of(10, 24, 3) == 3 and ls.tile_of(10, 24, 1) == 1  # 40 960 / 1040 = 39: the cap
    assert ls.tile_of(10, 768) == 10       # 40 960 / (3072 + 672 + 256 + 16), as tests/cpp/test_label_plan.cpp
    assert ls.tile_of(1024, 24) == 2       # 40 960 / (96 + 16 896 + 256 + 16) = 2
    assert ls.tile_of(64, 256) == 14       # 40 960 / (1024 + 1536 + 256 + 16)
    assert ls.tile_of(1024, 1536) == 1 and ls.tile_of(10, 24, 1000) == 39


def test_slots_and_the_sort():
    values = [3, 4, 900, 0x80000001, 0xFFFFFFFE]
    want = [4, 3, 5, 0, 0xFFFFFFFE, 0xFFFFFFFF, -1, 0x80000001, 0x80000002, 899, 900]
    none = ls.SLOT_NONE
    assert ls.slots_of(values, want).tolist() == [1, 0, none, none, 4, none, none, 3, none, none, 2]
    assert ls.slots_of([], [1, 2]).tolist() == [none, none]
    sslot, order = ls.sorted_slots([2, none, 0, 2, 0, none, 2])
    assert sslot.tolist() == [0, 0, 2, 2, 2, none, none] and order.tolist() == [2, 4, 0, 3, 6, 1, 5]


def test_tiles():
    sslot = [0] * 5 + [1] + [4] * 6 + [ls.SLOT_NONE] * 4
    assert ls.tiles(sslot, 3) == [(0, 3), (3, 2), (5, 1), (6, 3), (9, 3), (12, 3), (15, 1)]
    assert ls.tiles(sslot, 16) == [(0, 5), (5, 1), (6, 6), (12, 4)]
    assert ls.tiles(sslot, 1) == [(p, 1) for p in range(16)] and ls.tiles([], 4) == []
    assert [c for _, c in ls.tiles([7] * 33, 16)] == [16, 16, 1]


def test_the_items_past_the_grid_clamp():
    assert ls.GRID_MAX == 2 ** 20 and 959 * 1094 > 2 ** 20 >= 958 * 1094
    assert ls.items(1000, 1094) == 1094000 > 2 ** 20 and ls.items(958, 1094) == 1048052 <= 2 ** 20
    assert ls.item_of(576, 1048, 1000) == 2 ** 20 and ls.item_of(575, 1048, 1000) == 2 ** 20 - 1
    past = ls.past_clamp(1000, 1094)
    assert past.shape == (1094, 1000) and past.sum() == 1094000 - 2 ** 20
    assert past[1049:].all() and not past[:1048].any()                     # slices >= 1049: every position
    assert not past[1048, :576].any() and past[1048, 576:].all()           # slice 1048: positions >= 576 alone
    assert not ls.past_clamp(958, 1094).any()
    # a list that holds every row: slice s is batch s, so the second turn reads list positions from 1048 * 64 on, and
    # from 1049 * 64 = 67 136 on for every position
    assert ls.second_turn_first_row(1000, 1094, 70001) == (67072, 67136)
    assert ls.second_turn_first_row(958, 1094, 70001) == (None, None)


def test_blocks_that_carry_lds_into_a_second_turn():
    # the scan kernel: every item is live, so each of the 45 424 blocks with a second item has two live ones
    assert len(ls.both_turns(1000, 1094, 1000)) == 1094000 - 2 ** 20 == 45424
    # the tile kernel at T = 16 over 1000 queries of one label has 63 tiles: block b meets tile b % 1000 and then tile
    # (b + 576) % 1000, and both are below 63 for no b -- no block of that call has two live items
    assert len(ls.tiles([0] * 1000, 16)) == 63 and len(ls.both_turns(1000, 1094, 63)) == 0
    # at T = 2 there are 500 tiles: blocks with b % 1000 in 424 .. 499 meet tile b % 1000 - 424 in their second turn
    b = ls.both_turns(1000, 1094, 500)
    assert len(ls.tiles([0] * 1000, 2)) == 500 and len(b) == 76 * 45 and set((b % 1000).tolist()) == set(range(424, 500))
    assert len(ls.both_turns(958, 1094, 958)) == 0 and len(ls.both_turns(10, 3, 10)) == 0


def test_the_column_makers():
    n = 5000
    dups = np.linspace(0, n - 1, 40).astype(np.int64)
    none = ls.none_rows(n, 100, dups, 4000, 1)
    assert len(none) == 100 == len(set(none.tolist())) and none.max() < 4000 and not np.isin(none, dups).any()
    one = ls.column_one(n, 0x80000001, none)
    assert ls.info_of(one, n) == (n, 1, n - 100, n - 100) and ls.info_of(ls.column_one(n, 5), n) == (n, 1, n, n)
    own = ls.column_own(n, none)
    assert ls.info_of(own, n) == (n, n - 100, n - 100, 1) and own[1] == 2654435761 and own[2] == (2 * 2654435761) % 2 ** 32
    listed = own[own != ls.LABEL_NONE]
    assert all(len(np.unique((listed >> s) & 0xFF)) == 256 for s in (0, 8, 16, 24))  # every byte takes every value
    mix, info = ls.column_mix(n, dups, 1000, none, 3, rounds=2)
    sizes = info["sizes"]
    assert sizes[info["big"]] == 1040 and (mix[dups] == info["big"]).all() and (mix == ls.LABEL_NONE).sum() == 100
    assert sizes[info["top"]] == 1 and info["adjacent"][1] == info["adjacent"][0] + 1 and all(a in sizes for a in info["adjacent"])
    assert sorted(sizes.values())[:2] == [1, 1] and sorted(set(ls.SMALL_SIZES)) == sorted(set(sizes.values()) & set(ls.SMALL_SIZES))
    values = np.array(sorted(sizes))
    assert info["between"] not in sizes and values[0] < info["between"] < values[-1] and info["below"] < values[0]
    assert info["below"] not in sizes and values[-1] == 0xFFFFFFFE
    tail = [c for v, c in sizes.items() if c not in ls.SMALL_SIZES and v != info["big"]]
    assert all(20 <= c <= 40 for c in sorted(tail)[1:]) and len(tail) > 20
    for v, c in sizes.items():
        assert (mix == v).sum() == c
    want = list(sizes)[:50] + [info["between"], info["below"], ls.LABEL_NONE, -1]
    np.testing.assert_array_equal(ls.counts_of(mix, want), lr.masks_of(mix, want).sum(axis=1))
    even = np.arange(n) % 2 == 0
    np.testing.assert_array_equal(ls.counts_of(mix, want, even), (lr.masks_of(mix, want) & even).sum(axis=1))
    assert ls.info_of(mix, n) == (n, len(sizes), n - 100, 1040)
    col = ls.sized_column(n, [1, 9, 10, 2000], 4, first=5)
    assert [(col == v).sum() for v in (5, 6, 7, 8)] == [1, 9, 10, 2000] and (col == ls.LABEL_NONE).sum() == n - 2020


def test_spread_groups():
    want = ls.spread_groups(100, [(7, 1), (8, 15), (9, 16), (10, 17)], 3, seed=2)
    assert [(want == g).sum() for g in (7, 8, 9, 10, 3)] == [1, 15, 16, 17, 51]
    at = np.nonzero(want == 10)[0]
    assert (np.diff(at) > 1).any()  # spread over the batch, not one run
