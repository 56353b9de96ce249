"""CPU pins of tests/ranged_scale_reference.py, the pure-Python pieces of the three range scale modules, on hand-made
cases: the restated span rules against figures worked out by hand from range_plan.h, label_range_plan.h and
labelset_range_plan.h, the column makers against their promises and against the yardsticks' masks."""
import numpy as np

import label_ranged_reference as lrr
import labeled_scale_reference as ls
import labelset_ranged_reference as srr
import ranged_reference as rr
import ranged_scale_reference as rs

NONE = rs.NONE


def test_the_rules_of_batches_and_items_are_the_label_modules():
    assert rs.batches is ls.batches and rs.slice_count is ls.slice_count and rs.slice_ranges is ls.slice_ranges
    assert rs.items is ls.items and rs.past_clamp is ls.past_clamp and rs.both_turns is ls.both_turns
    assert rs.GRID_MAX == 2 ** 20 and rs.BATCH == 64


def test_the_span_order_of_a_column():
    #        id:  0   1     2   3   4  5     6
    keys = [30, 10, NONE, 30, 20, 0, 0xFFFFFFFE]
    ids, skeys = rs.span_order(keys)
    assert ids.tolist() == [5, 1, 4, 0, 3, 6] and skeys.tolist() == [0, 10, 20, 30, 30, 0xFFFFFFFE]  # ids ascend within key 30
    even = np.arange(7) % 2 == 0
    ids, skeys = rs.span_order(keys, even)
    assert ids.tolist() == [4, 0, 6] and skeys.tolist() == [20, 30, 0xFFFFFFFE]


def test_spans_of_ranges():
    skeys = np.array([0, 10, 20, 30, 30, 0xFFFFFFFE])
    #           all      no end     lo>hi     gap       plateau   above     one     top        bounds in gaps
    lo = [0,          0,         25,       11,       30,       NONE,     10,     0xFFFFFFFE, 5]
    hi = [0xFFFFFFFE, NONE,      15,       19,       30,       NONE,     10,     NONE,       25]
    at, ln = rs.spans_of(skeys, lo, hi)
    assert at.tolist() == [0, 0, 0, 0, 3, 0, 1, 5, 1] and ln.tolist() == [6, 6, 0, 0, 2, 0, 1, 1, 2]
    # (lo > hi with keys between: lower_bound(25) = 3 > upper_bound(15) = 2 -- the rule returns (0, 0), not a negative length)
    np.testing.assert_array_equal(ln, rr.masks_of([30, 10, NONE, 30, 20, 0, 0xFFFFFFFE], lo, hi).sum(1))


def test_spans_of_pairs():
    #          id:   0  1     2  3  4           5           6     7
    labels = [7, 7,    8, 8, 0xFFFFFFFE, 7,          NONE, 8]
    keys = [5, NONE, 0, 9, 0xFFFFFFFE, 0xFFFFFFFE, 1,    9]
    ids, spairs = rs.pair_order(labels, keys)
    assert ids.tolist() == [0, 5, 2, 3, 7, 4]  # rows 1 (no key) and 6 (no label) are not listed; 3 before 7 on equal pairs
    assert [int(x) for x in spairs] == [(7 << 32) | 5, (7 << 32) | 0xFFFFFFFE, 8 << 32, (8 << 32) | 9, (8 << 32) | 9,
                                        (0xFFFFFFFE << 32) | 0xFFFFFFFE]
    assert int(spairs[-1]) == 0xFFFFFFFEFFFFFFFE < rs.PAIR_NONE  # the largest composite there is
    #       7 open end       8 all   absent 6 (below)  absent between  NONE   -1   lo>hi  top         9 (above all but top)
    want = [7,               8,      6,                 9,              NONE,  -1,  8,     0xFFFFFFFE, 0xFFFFFFFD]
    lo = [0,                 0,      0,                 0,              0,     0,   9,     0,          0]
    hi = [NONE,              9,      NONE,              NONE,           NONE,  9,   0,     NONE,       NONE]
    at, ln = rs.pair_spans_of(spairs, want, lo, hi)
    # label 7 with no upper end runs directly against the first row of label 8 (position 2) and holds none of it
    assert at.tolist() == [0, 2, 0, 0, 0, 0, 0, 5, 0] and ln.tolist() == [2, 3, 0, 0, 0, 0, 0, 1, 0]
    np.testing.assert_array_equal(ln, lrr.masks_of(rs.u32(labels), keys, rs.u32(want), lo, hi).sum(1))
    even = np.arange(8) % 2 == 0
    ids, spairs = rs.pair_order(labels, keys, even)
    assert ids.tolist() == [0, 2, 4]


def test_the_batch_order_by_span_start():
    at = [40, 0, 7, 0, 40, 0]
    ln = [5, 0, 1, 9, 2, 0]
    # starts 0 (p 3), 7 (p 2), 40 (p 0, then p 4: stable), the empty spans (p 1, p 5) last although their `at` is 0
    assert rs.batch_order(at, ln).tolist() == [3, 2, 0, 4, 1, 5]
    assert rs.batch_order([0, 0, 0], [1, 1, 1]).tolist() == [0, 1, 2]


def test_the_rows_of_a_second_turn():
    # 1000 positions x 1094 slices over spans that hold every row: slice s is batch s; items at or past 2^20 are slices
    # >= 1049 for every position and slice 1048 from position 576 on (tests/test_labeled_scale_cpu.py)
    n, nq = 70001, 1000
    at, ln = np.zeros(nq, dtype=np.int64), np.full(nq, n, dtype=np.int64)
    at[1::2], ln[1::2] = 3200, n - 3200  # every second query: everything from rank 3200 on
    order = rs.batch_order(at, ln)
    assert order[:500].tolist() == list(range(0, nq, 2)) and order[500:].tolist() == list(range(1, nq, 2))
    rows = rs.second_turn_rows(order, at, ln, 1094)
    # position 0 .. 499 are the whole-column spans, p = 2 * pos: batches 1049 .. 1093 -> ranks from 67 136
    assert rows[0].tolist() == [67136, n] and rows[998].tolist() == [67136, n]
    # positions 500 .. 999 hold the spans of 66 801 rows = 1044 batches under 1094 slices: slice s reads the batches
    # [s * 1044 // 1094, (s + 1) * 1044 // 1094); position 500 + j is p = 2 * j + 1; positions >= 576 take slice 1048 in
    # a second turn (1048 * 1044 // 1094 = 1000), the others slice 1049 (1049 * 1044 // 1094 = 1001)
    assert 66801 == n - 3200 and ls.batches(66801) == 1044
    assert rows[1].tolist() == [1001 * 64, 66801] and rows[2 * 75 + 1].tolist() == [1001 * 64, 66801]
    assert rows[2 * 76 + 1].tolist() == [1000 * 64, 66801] and rows[999].tolist() == [1000 * 64, 66801]
    # 958 positions: nothing is past the clamp
    assert not rs.second_turn_rows(np.arange(958), np.zeros(958, dtype=np.int64), np.full(958, n), 1094).any()
    # a short span has no batch in a late slice
    at2, ln2 = np.zeros(nq, dtype=np.int64), np.full(nq, n, dtype=np.int64)
    ln2[7] = 65  # two batches: slice_ranges(65, 1094) puts them in slices 546 and 1093 -> the second is a second-turn row
    assert ls.slice_ranges(65, 1094)[1093] == (1, 2) and ls.slice_ranges(65, 1094)[546] == (0, 1)
    assert rs.second_turn_rows(rs.batch_order(at2, ln2), at2, ln2, 1094)[7].tolist() == [64, 65]


def test_the_blocks_that_carry_lds():
    every = np.ones(1000, dtype=bool)
    np.testing.assert_array_equal(rs.carrying_blocks(every, 1094), ls.both_turns(1000, 1094, 1000))
    assert len(rs.carrying_blocks(every, 1094)) == 45424 and len(rs.carrying_blocks(np.ones(958, dtype=bool), 1094)) == 0
    head = np.arange(1000) < 500
    np.testing.assert_array_equal(rs.carrying_blocks(head, 1094), ls.both_turns(1000, 1094, 500))
    # 1200 positions x 1094 slices = 1 312 800 items: 264 224 blocks take a second item, 2^20 % 1200 = 976 positions on; with
    # the first 400 positions live, b % 1200 < 400 and (b + 976) % 1200 < 400 hold together for b % 1200 in 224 .. 399
    live = np.arange(1200) < 400
    b = rs.carrying_blocks(live, 1094)
    assert 2 ** 20 % 1200 == 976 and rs.items(1200, 1094) - 2 ** 20 == 264224
    assert set((b % 1200).tolist()) == set(range(224, 400)) and len(b) == 176 * 220 + sum(1 for x in range(224, 400) if x < 264224 % 1200)


def test_the_kept_pairs_of_a_set_range_batch():
    # spans by label: 5 -> (10, 4), 6 -> (14, 2), 9 -> empty
    span = {5: (10, 4), 6: (14, 2), 9: (0, 0), NONE: (0, 0)}
    sets = [[5, 9, 5], [6, 5], [], [9, 9], [5, 5, 5, 6, 6], [NONE, 6]]
    first, values = rs.csr(sets)
    assert first.tolist() == [0, 3, 5, 5, 7, 12, 14] and rs.pairs_of(first).tolist() == [0, 0, 0, 1, 1, 3, 3, 4, 4, 4, 4, 4, 5, 5]
    at = np.array([span[int(v)][0] for v in values])
    ln = np.array([span[int(v)][1] for v in values])
    kept, order = rs.kept_pairs(first, values, at, ln)
    # the run of start 10 holds pairs 0, 2 (query 0), 4 (query 1), 7, 8, 9 (query 4) in pair order; that of start 14 pairs 3,
    # 10, 11, 13; the empty ones last
    assert order.tolist() == [0, 2, 4, 7, 8, 9, 3, 10, 11, 13, 1, 5, 6, 12]
    assert np.nonzero(kept)[0].tolist() == [0, 3, 4, 7, 10, 13]
    np.testing.assert_array_equal(kept, rs.distinct_pairs(first, values, ln))
    # the union the kept pairs stand for is the yardstick's
    labels = np.array([5] * 4 + [6] * 2 + [7] * 3)
    keys = np.arange(9) * 10
    ids, spairs = rs.pair_order(labels, keys)
    lo, hi = np.zeros(6, dtype=np.int64), np.full(6, 25)
    o = rs.pairs_of(first)
    at, ln = rs.pair_spans_of(spairs, values, lo[o], hi[o])
    kept, _ = rs.kept_pairs(first, values, at, ln)
    counts = np.bincount(o[kept], weights=ln[kept], minlength=6).astype(np.int64)
    assert counts.tolist() == [3, 3, 0, 0, 3, 0]
    np.testing.assert_array_equal(counts, srr.masks_of(labels, keys, sets, lo, hi).sum(1))


def test_the_ranked_column():
    n = 5000
    dups = np.linspace(0, n - 1, 40).astype(np.int64)
    missing = ls.none_rows(n, 100, dups, 4000, 1)
    fixed = dict(zip(dups.tolist(), np.linspace(3, n - 120, 40).astype(np.int64).tolist()))
    keys, rank_of = rs.ranked_column(n, 5, fixed, missing)
    listed = n - 100
    assert (keys == NONE).sum() == 100 and (keys[missing] == NONE).all() and (rank_of[missing] == -1).all()
    assert [int(rank_of[v]) for v in dups] == list(fixed.values())
    ids, skeys = rs.span_order(keys)
    assert len(ids) == listed and (np.diff(skeys) > 0).all() and skeys[0] == 0 and skeys[-1] == 0xFFFFFFFE
    np.testing.assert_array_equal(rank_of[ids], np.arange(listed))
    assert (np.diff(ids) < 0).sum() > 1000  # span order is not id order
    assert rs.key_of_rank([0, 1, 2, listed - 1], listed).tolist() == [0, 61363, 122719, 0xFFFFFFFE]
    assert 70000 * rs.STEP + 7 < 0xFFFFFFFE  # and the keys are spread over all four bytes (STEP = 4 * 15 339: 64 low bytes)
    spread = [len(np.unique((rs.key_of_rank(np.arange(70001), 70001) >> s) & 0xFF)) for s in (0, 8, 16, 24)]
    assert spread == [66, 256, 256, 256]
    for r, c in ((0, 1), (0, listed), (17, 0), (17, 1), (17, 64), (17, 65), (listed - 5, 5), (listed - 1, 1)):
        lo, hi = rs.span(r, c, listed)
        at, ln = rs.spans_of(skeys, [lo], [hi])
        assert (at[0], ln[0]) == ((r, c) if c else (0, 0)), (r, c)
        assert rr.masks_of(keys, [lo], [hi]).sum() == c


def test_the_plateau_column():
    n = 5000
    dups = np.linspace(0, n - 1, 40).astype(np.int64)
    missing = ls.none_rows(n, 100, dups, 4000, 1)
    keys, flat = rs.plateau_column(n, 6, dups, 1000, 1300, missing)
    assert (keys == flat).sum() == 1300 and (keys[dups] == flat).all() and (keys == NONE).sum() == 100
    ids, skeys = rs.span_order(keys)
    at, ln = rs.spans_of(skeys, [flat, flat + 1, 0], [flat, NONE, flat - 1])
    assert at.tolist() == [1000, 2300, 0] and ln.tolist() == [1300, n - 100 - 2300, 1000]
    assert (np.diff(ids[1000:2300]) > 0).all()  # ids ascend within the one key


def test_keys_within_labels():
    labels = ls.sized_column(2000, [300, 26, 1, 700], 9, first=40)
    keys = rs.within_label_keys(labels, 3)
    for v, c in ((40, 300), (41, 26), (42, 1), (43, 700), (NONE, 2000 - 1027)):
        assert sorted(keys[labels == v].tolist()) == [1000 + 10 * i for i in range(c)]
    lo, hi = rs.ranks(25, 275)
    sets = [[40], [40, 43], [40, 43, 41], [41], [42], [40, 41, 40]]
    m = srr.masks_of(labels, keys, sets, np.full(6, lo), np.full(6, hi))
    assert m.sum(1).tolist() == [250, 500, 501, 1, 0, 251]
    lo, hi = rs.ranks(5, 5)
    assert lo <= hi and not srr.masks_of(labels, keys, [[40, 43]], [lo], [hi]).any()
    ids, spairs = rs.pair_order(labels, keys)
    at, ln = rs.pair_spans_of(spairs, [40, 43, 41, 42, 44], *[np.full(5, x) for x in rs.ranks(25, 275)])
    assert ln.tolist() == [250, 250, 1, 0, 0] and at.tolist() == [25, 300 + 26 + 1 + 25, 300 + 25, 0, 0]
