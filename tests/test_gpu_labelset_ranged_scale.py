"""Run time on an MI355X: 15 s (22 cases, first clean run, the slowest 1.9 s); run it under `timeout -k 10 45`, three times that.

The set-range stack (phnsw_label_attr_count_set_device, the PAIRS form of ph_label_ranged_scan_kernel with
ph_labelset_ranged_lookup / _dup / _merge_kernel in filter_label_ranged.hip, labelset_range_plan.h, the search kernels'
set-range mode, phnsw_search_labelset_ranged_auto) at the smallest shapes where its loops turn more than once, on the
worlds of tests/test_gpu_filter_scale.py: World A, N = 70 001 rows with 40 copies of row 0 at DUPS, its built graph and
its every-second-vector index, imported and never rebuilt.  tests/test_gpu_exact_labelset_ranged.py,
test_gpu_labelset_ranged_walk.py and test_gpu_labelset_ranged_auto.py cover kinds, dimensions, metrics and refusals on
2000 and 5000 rows.  Every comparison here is on ids, distance bits, lengths, status, routes and stats, no tolerance
anywhere.  The columns and handles are tests/test_gpu_label_ranged_scale.py's (ONE, PLAT, OWN, MIX, PART, ROUTE, FAR: the
set calls take the same phnsw_label_attr), the calls by name, the device forms and the bodies of the tests
tests/test_gpu_ranged_scale.py's.

The seven gaps, each with the test that closes it and the shape it asserts:
  1. the item loop of ph_label_ranged_scan_kernel<Dist, PAIRS> past the 2^20-block clamp --
     test_the_second_turn_of_the_item_loop: 400 queries, each with the set [V, absent, V], are 1200 pairs; x 1094 slices
     (PHNSW_LABELSET_RANGE_SLICES=5000 clamped by longest = 70 001) = 1 312 800 items > 1 048 576.  In span-start order
     the positions 0 .. 799 alternate a live pair and its duplicate (two span starts, 400 positions each), 800 .. 1199
     are the empty spans of the absent label: block b meets position b % 1200 and then (b + 976) % 1200, and both are live
     for 63 360 of the 264 224 blocks that take a second item; the others meet duplicates and empty pairs between live
     ones.  k = 10 (the scratch is nwant x slices x k x 8 bytes: 105 MB); query 0 is the duplicated row and six of the ten
     copies in its row sit at span ranks only second-turn items read.
  2. construction: the handles are the label-range module's; here test_count_sets_describe_the_columns counts about 1000
     sets against the kept pairs of the restated rule, numpy and filter_count, and once over every second vector.
  3. the per-call sort past one tile and the duplicate rule that leans on its stability -- the 1200 pairs of test 1 (runs
     of one span start that hold 400 pairs of 200 queries), test_every_row_its_own_label (600 queries, 1500 pairs) and the
     1000 sets of test 2; the kept pairs of every batch are asserted equal to the distinct labels with non-empty spans.
  4. a slice that overflows k = 1024 -- test_long_spans_whatever_the_slices, one label, a label twice, a union of three.
  5. the shipped threshold -- test_the_routed_call_*: unions of 5000 rows scan and unions of 5001 walk at (ef, k) =
     (256, 10), where the second rule does not hide that edge as it does at (64, 10); the unions are made of two and three
     labels, some sets name a label twice and a duplicate is not counted twice; 600 queries, both routes in every wave.
  6. the walk's set-range mode at N > 65 536 -- test_the_walk_by_set_and_range_at_scale.
  7. a wide query matrix -- test_wide_queries.

Yardsticks, named where they are applied: (1) tests/exact_filter_reference.exact_topk over World A's oracle distances
with the masks tests/labelset_ranged_reference.masks_of makes of the columns, which the code under test never sees; (2)
the established bitmap calls on the same masks (search_exact_filtered, search_batch_filtered,
filter_auto_reference.compose / rule / assert_complete, filter_count), pinned against the oracle on this very world by
tests/test_gpu_filter_scale.py; it carries the 400- and 600-query cases and the f16 / i8 stores.

Not exercised: the scan by a set of labels without a range (phnsw_search_exact_labelset, the set walk,
phnsw_search_labelset_auto), the 65 536-block clamp of grid1, the 2^20 clamp of ph_labelset_ranged_merge_kernel (more than
1 048 576 queries), nq or nwant near PH_LABEL_NQ_MAX, a third turn of the item loop,
and the threshold itself: these tests pin what scan_below = 0 does today."""
import numpy as np
import pytest

import exact_filter_reference as xr
import filter_auto_reference as ar
import ranged_scale_reference as rs
from test_gpu_exact_filter import same
from test_gpu_filter_scale import DUPS, EVEN, K, N, NQR, NQX, SP, both_routes_in_every_wave, first_graph, gworld, half_index, world
from test_gpu_label_ranged_scale import ABSENT, RA, RB, RC, RE, lcol, lhandle, own_batch
from test_gpu_labeled_scale import ABSENT_ROUTE, FULL, TURN_ROW, V_ONE, far_batch, forms, mix
from test_gpu_ranged_scale import (BELOW, BIG, KINDS, LATE, NONE, TOP, counts_of, device_call, far_body, host, join, kcol,
                                   long_spans_body, make_handle, masks_of, routed_check, scans_next_to_walks_body, second_turn_body,
                                   spec_of, take, three_blocks_body, walk_body, wide_body)

pytestmark = pytest.mark.gpu

EMPTY = xr.EMPTY
STACK = "set"
V_ABSENT = 0x80000000      # directly below the one label of ONE and PLAT
NQS = 400                  # queries of the second-turn case: 1200 pairs
SPR, KR = (256, 256, 2), 10  # the routed cases: 5001 * 256 >= 10 * N, so the first rule alone parts 5000 from 5001


def sone(labels, lo, hi):
    """the one-query batch (label IN labels, lo <= key <= hi)"""
    return spec_of([lo], [hi], [list(labels)])


def union(labels, c):
    """c rows of EVERY label of the set that has more than 25 + c rows (ROUTE: the ranks [25, 25 + c) inside each label)"""
    return sone(labels, *rs.ranks(25, 25 + c))


def pairs_of_batch(c, spec, members=None):
    """the batch as labelset_range_plan.h cuts it -> (first, values, owner, at, len, kept, order)"""
    first, values = rs.csr(spec["want"])
    owner = rs.pairs_of(first)
    ids, spairs = rs.pair_order(c["labels"], c["keys"], members)
    at, ln = rs.pair_spans_of(spairs, values, spec["lo"][owner], spec["hi"][owner])
    kept, order = rs.kept_pairs(first, values, at, ln)
    np.testing.assert_array_equal(kept, rs.distinct_pairs(first, values, ln))  # the duplicate rule finds the distinct labels
    return first, values, owner, at, ln, kept, order


def numpy_counts(c, spec, members=None):
    first, values, owner, at, ln, kept, order = pairs_of_batch(c, spec, members)
    return np.bincount(owner[kept], weights=ln[kept], minlength=len(spec["lo"])).astype(np.int64)


def sample_sets(c, count, seed):
    """`count` sets with one range each: one to four labels of listed rows drawn at random, in turn as they are, with the
    first label again at the end, with an absent label and NONE between them, and now and then the empty set; the range
    in turn unbounded, from a key drawn at random on, between two such keys, lo > hi"""
    rng = np.random.default_rng(seed)
    listed = np.nonzero((c["labels"] != NONE) & (c["keys"] != NONE))[0]
    values = np.unique(c["labels"][listed])
    absent = int(values[0]) - 1 if values[0] > 0 else int(values[-1]) + 1
    assert absent not in values and 0 <= absent < NONE
    sets, lo, hi = [], [], []
    for i in range(count):
        s = c["labels"][listed[rng.integers(0, len(listed), 1 + i % 4)]].tolist()
        s = (s, s + s[:1], s[:1] + [absent, NONE] + s[1:], s + [-1] + s)[i % 3 if i % 11 else 3]
        sets.append([] if i % 50 == 49 else s)
        a, b = np.sort(c["keys"][listed[rng.integers(0, len(listed), 2)]])
        r = ((0, NONE), (int(a), NONE), (int(a), int(b)), (0, TOP), (int(b) + 1, int(a)))[i % 5]
        lo.append(r[0]), hi.append(r[1])
    return spec_of(lo, hi, sets)


# ---------------------------------------------------------------- 1: the counts of sets
@pytest.mark.parametrize("name", ["own", "mix", "part", "route"])
def test_count_sets_describe_the_columns(name):
    w, c, h = world("f32", 24), lcol(name), lhandle("ring", "f32", name)
    hix = w["hix"]
    spec = sample_sets(c, 1000, 541)
    first, values, owner, at, ln, kept, order = pairs_of_batch(c, spec)
    assert len(values) > 2500 and (~kept & (ln > 0)).sum() > 100 and (ln == 0).sum() > 300   # duplicates and empty pairs
    counts = counts_of(STACK, h, spec)
    masks = masks_of(STACK, c, spec)
    np.testing.assert_array_equal(counts, numpy_counts(c, spec))                     # numpy: the kept pairs
    np.testing.assert_array_equal(counts, masks.sum(axis=1))                         # the yardstick's masks
    np.testing.assert_array_equal(counts, hix.filter_count(masks))                   # yardstick 2
    assert (counts == 0).sum() >= 20 and (counts > 0).sum() >= 400
    sq = take(spec, slice(0, NQX))
    for form, kw, D in forms(w):
        got = host(STACK, "exact", hix, h, sq, k=K, **kw)
        same(got, xr.exact_topk(D, masks[:NQX], None, None, K))                      # yardstick 1
        dv = device_call(STACK, "exact", hix, h, sq, k=K, **kw)
        assert not dv[3].any()
        same(dv, got)


def test_count_sets_over_every_second_vector():
    """vec2node is not the identity: odd ids carry labels and values and are listed nowhere"""
    w, c, half = world("f32", 24), lcol("mix"), half_index("f32", 24)
    h = make_handle(STACK, half, c)
    spec = sample_sets(c, NQR, 542)
    masks = masks_of(STACK, c, spec)
    counts = counts_of(STACK, h, spec)
    np.testing.assert_array_equal(counts, numpy_counts(c, spec, EVEN))               # numpy
    np.testing.assert_array_equal(counts, half.filter_count(masks))                  # yardstick 2
    np.testing.assert_array_equal(counts, (masks & EVEN).sum(axis=1))
    sq = take(spec, slice(0, NQX))
    sq["want"][0], sq["lo"][0], sq["hi"][0] = [int(c["labels"][0])] * 2, 0, NONE     # query 0 is the duplicated row
    masks = masks_of(STACK, c, sq)
    for form, kw, D in forms(w):
        got = host(STACK, "exact", half, h, sq, k=64, **kw)
        same(got, xr.exact_topk(D, masks, None, EVEN, 64))                           # yardstick 1
        same(got, half.search_exact_filtered(allow=masks, k=64, **kw))               # yardstick 2
        dv = device_call(STACK, "exact", half, h, sq, k=64, **kw)
        assert not dv[3].any()
        same(dv, got)
        assert not (got[0][got[0] != EMPTY] % 2).any() and got[2][0] == 64
    h.close()


def test_every_row_its_own_label():
    """OWN: 69 901 labels of one row, 600 queries, in turn by the label module's own_batch: [its label] with its key alone
    -- one row; [its label, an absent one, its label] with the gap above its key -- none; [the next label, its label]
    without bounds -- two rows; [its label + 1, NONE] -- none; and every 25th query the empty set"""
    w, c, h = gworld("f32"), lcol("own"), lhandle("graph", "f32", "own")
    hix, qids = w["hix"], w["qids"]
    lspec, _, turn = own_batch()
    mine = c["labels"][qids.astype(np.int64)]
    sets = [([int(m)], [int(m), V_ABSENT, int(m)], [int(x), int(m)], [int(x), NONE])[t] for m, x, t in zip(mine, lspec["want"], turn)]
    rows = np.array([1, 0, 2, 0])[turn]
    lo, hi = lspec["lo"].copy(), lspec["hi"].copy()
    for i in range(24, NQR, 25):
        sets[i], rows[i] = [], 0
    spec = spec_of(lo, hi, sets)
    first, values, owner, at, ln, kept, order = pairs_of_batch(c, spec)
    assert len(values) > 1000 and (np.bincount(owner[kept], minlength=NQR) == rows).all()
    assert len(set(at[kept].tolist())) == kept.sum() > 400                           # as many span starts as live pairs
    masks = masks_of(STACK, c, spec)
    assert (masks.sum(axis=1) == rows).all()
    for kw in (dict(queries=w["q"]), dict(qids=qids)):
        dv = device_call(STACK, "exact", hix, h, spec, k=10, **kw)
        assert not dv[3].any() and (dv[2] == rows.astype(np.uint64)).all()
        same(dv, hix.search_exact_filtered(allow=masks, k=10, **kw))                 # yardstick 2
        same(host(STACK, "exact", hix, h, spec, k=10, **kw), dv)
    own_row = (turn == 0) & (rows == 1)
    np.testing.assert_array_equal(dv[0][own_row, 0], qids[own_row])                  # a stored query finds its own row
    dv = device_call(STACK, "exact", hix, h, spec, k=10, qids=qids, exclude=qids)    # ... and not with it taken out
    assert not dv[3].any() and (dv[2] == (rows - (rows > 0)).astype(np.uint64)).all()
    same(dv, hix.search_exact_filtered(qids=qids, allow=masks, exclude=qids, k=10))


# ---------------------------------------------------------------- 2: long spans, whatever the slices
@pytest.mark.parametrize("kind", KINDS)
def test_long_spans_whatever_the_slices(monkeypatch, kind):
    """the plateau under a set that names its label twice around an absent one; BIG's 25 040 rows by distinct keys under
    [BIG]; the union of BIG and the adjacent labels x, x + 1; all 69 901 rows of PLAT"""
    flat = int(kcol("flat")[DUPS[0]])
    info = mix()[1]
    x, x1 = info["adjacent"]
    both = BIG + info["sizes"][x] + info["sizes"][x1]
    cases = [(lcol("plat"), lhandle("ring", kind, "plat"), sone([V_ONE, V_ABSENT, V_ONE], flat, flat), BIG, N - 100),
             (lcol("mix"), lhandle("ring", kind, "mix"), sone([info["big"]], 0, NONE), BIG, BIG),
             (lcol("mix"), lhandle("ring", kind, "mix"), sone([x1, info["big"], x, NONE, x1], 0, TOP), both, BIG),
             (lcol("plat"), lhandle("ring", kind, "plat"), sone([V_ONE], 0, NONE), N - 100, N - 100)]
    assert [c[1].info()[3] for c in cases] == [N - 100, BIG, BIG, N - 100]           # longest clamps the slices
    long_spans_body(STACK, monkeypatch, kind, cases)


# ---------------------------------------------------------------- 3: the second turn of the item loop
# blocks whose first and second item are both live pairs: the live positions are the even ones below 800; the second item of
# block b is 976 positions on, so b % 1200 must be even and in 224 .. 799: 288 residues, 220 whole rounds of 1200 in 264 224
CARRYING = 288 * 220


def turn_spec():
    """400 sets [V, absent, V]; every second query asks for every row, the others for everything from rank 3200 on"""
    even = np.arange(NQS) % 2 == 0
    return spec_of(np.where(even, 0, int(rs.key_of_rank(3200, N))), np.where(even, TOP, NONE), [[V_ONE, V_ABSENT, V_ONE]] * NQS)


def test_the_second_turn_of_the_item_loop(monkeypatch):
    """see the module docstring, gap 1"""
    c, h = lcol("one"), lhandle("ring", "f32", "one")
    spec = turn_spec()
    first, values, owner, at, ln, kept, order = pairs_of_batch(c, spec)
    nwant = len(values)
    assert h.info()[3] == N and rs.slice_count(5000, N) == FULL and nwant == 1200 and rs.items(nwant, FULL) == 1312800 > rs.GRID_MAX
    assert kept.sum() == NQS and (~kept & (ln > 0)).sum() == NQS and (ln == 0).sum() == NQS   # live, duplicate, empty
    assert set(zip(at[kept].tolist(), ln[kept].tolist())) == {(0, N), (3200, N - 3200)}
    # positions 0 .. 399: the pairs of the even queries that want V, a live pair and its duplicate in turn (the sort is
    # stable); 400 .. 799: those of the odd queries; 800 .. 1199 the empty spans
    live = kept[order]
    assert (live[:800] == (np.arange(800) % 2 == 0)).all() and not live[800:].any() and (ln[order[800:]] == 0).all()
    assert (owner[order[:400]] % 2 == 0).all() and (owner[order[400:800]] % 2 == 1).all() and (order != np.arange(nwant)).sum() > 1000
    blocks = rs.carrying_blocks(live, FULL)
    meets = rs.carrying_blocks(np.ones(nwant, dtype=bool), FULL)
    assert len(meets) == 1312800 - 2 ** 20 == 264224 and len(blocks) == CARRYING and 0 < len(blocks) < len(meets)
    # pair 0 is (query 0, V) with every row, at position 0: 2^20 = 873 * 1200 + 976, so its slices from 874 on are second-turn
    # items and read the span ranks from 874 * 64 = 55 936 on
    rows = rs.second_turn_rows(order, at, ln, FULL)
    assert rows[0].tolist() == [874 * 64, N] and 874 * 64 < TURN_ROW
    rank_of_dups = np.searchsorted(rs.pair_order(c["labels"], c["keys"])[1], rs.composites(c["labels"], c["keys"])[DUPS])
    assert (rank_of_dups[:LATE] >= rows[0, 0]).all()                                 # six of the ten copies of its row
    second_turn_body(STACK, monkeypatch, c, h, spec, rank_of_dups, k=10, nq=NQS)


# ---------------------------------------------------------------- 4: the routed call past 256 queries
def test_the_rule_at_the_edge_of_the_threshold():
    assert BELOW[STACK] == 5000
    assert ar.rule(5001, 5000, SPR[0], KR, N) == ar.GRAPH and ar.rule(5000, 5000, SPR[0], KR, N) == ar.SCAN
    assert ar.rule(5001, 5000, SP[0], K, N) == ar.SCAN and first_graph() == 10938    # (64, 10) hides that edge


def test_the_routed_call_over_three_blocks_of_queries():
    """scan_below = 0 at (ef, k) = (256, 10): unions of 5000 rows scan and unions of 5001 walk; RE has 26 rows, so the ranks
    [25, 2525) hold 2500 rows of RA, 2500 of RB and one of RE"""
    c, h = lcol("route"), lhandle("graph", "f32", "route")
    one = [sone([], 0, NONE), union([RE], 1), union([RA, RA], K - 1), union([RB], K), union([RA, RB], 2500), union([RA, RB, RA], 2500),
           union([RA, ABSENT, RB], 2499), sone([NONE, ABSENT], 0, NONE), union([RA, RE, RE], 4999)]
    assert counts_of(STACK, h, join(one)).tolist() == [0, 1, K - 1, K, 5000, 5000, 4998, 0, 5000]
    scans = join([one[i % 9] for i in range(NQR)])
    turn = [union([RA, RB, RE], 2500), union([RA, RB], 2500), union([RA, RB, RA], 2500), sone([ABSENT], 0, NONE),
            union([RB, RA, RE, RB], 2500), union([RC, RA], 2500), union([RE], 1)]
    assert counts_of(STACK, h, join(turn)).tolist() == [5001, 5000, 5000, 0, 5001, 5000, 1]  # a duplicate is not counted twice
    mixed = join([turn[i % 7] for i in range(NQR)])
    three_blocks_body(STACK, c, h, scans, mixed, np.isin(np.arange(NQR) % 7, (0, 4)), sp=SPR, k=KR)


@pytest.mark.parametrize("scan_first", [True, False])
def test_a_block_of_scans_next_to_blocks_of_walks(scan_first):
    scans = [union([RA, RB], 2500), union([RA, RB, RA], 2500), sone([ABSENT], 0, NONE), union([RC], 4999), sone([], 0, TOP), union([RE], 1)]
    scans_next_to_walks_body(STACK, lcol("route"), lhandle("graph", "f32", "route"), scans, union([RB, RE, RA], 2500), scan_first,
                             sp=SPR, k=KR)


def far_spec(want):
    """far_batch's wanted labels as sets: in turn [w], [w, absent, w] and [absent, w]; NONE stays alone"""
    sets = [[int(x)] if int(x) == NONE else ([int(x)], [int(x), ABSENT_ROUTE, int(x)], [ABSENT_ROUTE, int(x)])[i % 3]
            for i, x in enumerate(want)]
    return spec_of(np.zeros(len(want), dtype=np.int64), np.where(np.arange(len(want)) % 2 == 0, NONE, TOP), sets)


@pytest.mark.parametrize("stored", [False, True])
def test_an_explicit_threshold_and_the_rescan_past_256_queries(stored):
    far_body(STACK, lcol("far"), lhandle("graph", "f32", "far"), far_spec(far_batch("f32", stored)[1]), stored)


@pytest.mark.parametrize("kind", ["i8q", "pq"])
def test_the_routed_call_on_the_other_kinds(kind):
    turn = [union([RA, RB, RE], 2500), union([RA, RB], 2500), union([RA, RB, RA], 2500), sone([ABSENT], 0, NONE), union([RB, RA, RE, RB], 2500)]
    got = routed_check(STACK, gworld(kind), lcol("route"), lhandle("graph", kind, "route"), join([turn[i % 5] for i in range(NQR)]),
                       device=True, sp=SPR, k=KR)
    both_routes_in_every_wave(got[3])
    np.testing.assert_array_equal(got[3] == ar.SCAN, ~np.isin(np.arange(NQR) % 5, (0, 4)))


# ---------------------------------------------------------------- 5: the walk by set and range at N > 65 536
def walk_spec():
    """20 001 rows of one label named twice, a wanted NONE, a union of three labels, two whole labels without bounds, an
    absent label, lo > hi with keys between, the empty set, a union of 5001 rows"""
    turn = [union([RA, RA], 20001), sone([NONE], 0, NONE), union([RA, RC, RB], 5000), sone([RB, RE], 0, NONE), sone([ABSENT], 0, NONE),
            sone([RA, RB], 9000, 2000), sone([], 0, NONE), union([RA, RB, RE], 2500)]
    return join([turn[i % 8] for i in range(NQR)]), np.isin(np.arange(NQR) % 8, (1, 4, 5, 6))


def test_the_walk_by_set_and_range_at_scale():
    spec, empty_at = walk_spec()
    walk_body(STACK, lcol("route"), lhandle("graph", "f32", "route"), spec, empty_at)


# ---------------------------------------------------------------- 6: wide queries
def test_wide_queries():
    wide_body(STACK, lcol("route"), lhandle("graph", "f32", "route"), walk_spec()[0])
