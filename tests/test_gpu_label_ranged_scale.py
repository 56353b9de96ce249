"""Run time on an MI355X: 11 s (25 cases, first clean run, the slowest 1.5 s); run it under `timeout -k 10 33`, three times that.

The label-range stack (phnsw_label_attr_*, filter_label_ranged.hip, label_range_plan.h, the search kernels' label-range
mode, phnsw_search_label_ranged_auto) at the smallest shapes where its loops turn more than once, on the worlds of
tests/test_gpu_filter_scale.py: World A, N = 70 001 rows with 40 copies of row 0 at DUPS, its built graph and its
every-second-vector index, imported and never rebuilt.  tests/test_gpu_exact_label_ranged.py,
test_gpu_label_ranged_walk.py and test_gpu_label_ranged_auto.py cover kinds, dimensions, metrics and refusals on 2000 and
5000 rows.  Every comparison here is on ids, distance bits, lengths, status, routes and stats, no tolerance anywhere.
The calls by name, the device forms and the bodies of the tests are tests/test_gpu_ranged_scale.py's; the key columns
are its ALL, FLAT and MIX (the ranked column of tests/ranged_scale_reference.py).

The label columns are those of tests/test_gpu_labeled_scale.py, each paired with a key column:
  ONE    one label, 0x80000001, on every row, keys ALL: listed == longest == N, the head written at p == n;
  PLAT   that label on every row, keys FLAT: 69 901 listed, a plateau of 25 040 rows with one composite;
  OWN    ls.column_own, keys ALL: 69 901 labels over all four bytes, longest == 1, 100 unlabelled rows;
  MIX    ls.column_mix, keys MIX: about 1400 labels, BIG = 25 040 rows on the copies, the adjacent labels x and x + 1 (an
         open-ended range on x runs directly against the first row of x + 1), the label 0xFFFFFFFE with key 0xFFFFFFFE;
  PART   MIX with 300 rows that carry a label and no value beside the 100 that carry a value and no label: neither listed;
  ROUTE  ls.sized_column: labels of 20 101, 20 101, 11 000, 26 and 500 rows, inside every label the keys 1000 + 10 * rank,
         so (label, ranks [a, b)) holds exactly the rows the rule's edges need, with rows of the label on either side;
  FAR    the far-rows labels of tests/test_gpu_labeled_scale.far_column, keys ALL.

The seven gaps, each with the test that closes it and the shape it asserts:
  1. the item loop of ph_label_ranged_scan_kernel past the 2^20-block clamp -- test_the_second_turn_of_the_item_loop:
     1000 queries x 1094 slices (PHNSW_LABEL_RANGE_SLICES=5000 clamped by longest = 70 001) = 1 094 000 items, 45 424 blocks
     carry LDS from a live item into a live item, two span starts interleaved in query order, query 0 the duplicated
     row at k = 40 with six copies only second-turn items read.
  2. construction past one sort tile and 2^16 rows, the 64-bit sort, head[1] over 69 901 labels, head[2] from a binary
     search over the whole column -- test_the_handles_describe_the_columns (info of every column against numpy,
     from_device, about 1000 counted pairs: a lookup among 69 901 composites) and
     test_a_handle_over_every_second_vector.
  3. the per-call sort past one tile -- the 1000 queries of test 1 and test_every_row_its_own_label: 600 queries, 300
     different span starts of one row and 300 empty spans between them.
  4. a slice that overflows k = 1024 -- test_long_spans_whatever_the_slices.
  5. the shipped threshold -- test_the_routed_call_*: 600 queries, scan_below = 0 parts 20 000 from 20 001 rows of a
     (label, range) pair; the scanned queries of a mixed batch are a scattered list of more than 400.
  6. the walk's label-range mode at N > 65 536 -- test_the_walk_by_label_and_range_at_scale (pair_of[v] for v > 65 536).
  7. a wide query matrix -- test_wide_queries.

Yardsticks, named where they are applied: (1) tests/exact_filter_reference.exact_topk over World A's oracle distances
with the masks tests/label_ranged_reference.masks_of makes of the columns, which the code under test never sees; (2)
the established bitmap calls on the same masks (search_exact_filtered, search_batch_filtered,
filter_auto_reference.compose / rule / assert_complete, filter_count), pinned against the oracle on this very world by
tests/test_gpu_filter_scale.py; it carries the 600- and 1000-query cases and the f16 / i8 stores.

Not exercised: the 65 536-block clamp of grid1 (n or nq past 16.7 M), the 2^20 clamp of ph_list_merge_kernel (more than
1 048 576 queries), nq near PH_LABEL_NQ_MAX, a third turn of the item loop, and the
UNMEASURED threshold itself: these tests pin what scan_below = 0 does today."""
import functools

import numpy as np
import pytest

import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import filter_auto_reference as ar
import labeled_scale_reference as ls
import ranged_scale_reference as rs
from test_gpu_exact_filter import same
from test_gpu_filter_scale import DUPS, EVEN, K, N, NQR, NQX, SP, both_routes_in_every_wave, first_graph, gworld, half_index, world
from test_gpu_labeled_scale import FULL, NONE_ROWS, NQT, TURN_ROW, V_ONE, far_batch, forms, mix
from test_gpu_labeled_scale import col as label_col
from test_gpu_ranged_scale import (BELOW, BIG, KINDS, LATE, NONE, ROUTE_SCANS, ROUTE_WALK, TOP, counts_of, device_call, far_body, host,
                                   index_of, join, kcol, long_spans_body, make_handle, masks_of, routed_check,
                                   scans_next_to_walks_body, second_turn_body, spec_of, take, three_blocks_body, walk_body,
                                   wide_body)

pytestmark = pytest.mark.gpu

EMPTY = xr.EMPTY
STACK = "label"
ROUTE_SIZES = (20101, 20101, 11000, 26, 500)
RA, RB, RC, RE, RF = (0x7FFFFFF0 + j for j in range(5))  # the labels of ROUTE
ABSENT = 0x7FFFFFEF                                        # directly below them


# ---------------------------------------------------------------- columns and handles
@functools.lru_cache(maxsize=None)
def lcol(name):
    """(labels, keys) of every row, i64 [N] each; each column asserts its own counts"""
    if name == "one":
        c = dict(labels=ls.column_one(N, V_ONE), keys=kcol("all"))
        assert info_of(c) == (N, N, 1, N)
    elif name == "plat":
        c = dict(labels=ls.column_one(N, V_ONE), keys=kcol("flat"))
        assert info_of(c) == (N, N - 100, 1, N - 100)
    elif name == "own":
        c = dict(labels=label_col("own"), keys=kcol("all"))
        assert info_of(c) == (N, 69901, 69901, 1)
    elif name == "mix":
        c = dict(labels=mix()[0], keys=kcol("mix"))
        assert info_of(c)[1:] == (N - 100, len(mix()[1]["sizes"]), BIG) and (c["keys"][c["labels"] == TOP] == TOP).all()
    elif name == "part":
        c = dict(labels=mix()[0], keys=kcol("part"))
        no_key, no_label = c["keys"] == NONE, c["labels"] == NONE
        assert no_key.sum() == 300 and no_label.sum() == 100 and not (no_key & no_label).any() and info_of(c)[1] == N - 400
    elif name == "route":
        labels = ls.sized_column(N, ROUTE_SIZES, 521, first=RA)
        c = dict(labels=labels, keys=rs.within_label_keys(labels, 522))
        assert info_of(c) == (N, sum(ROUTE_SIZES), 5, 20101) and not (labels == ABSENT).any()
    elif name == "far":
        c = dict(labels=far_batch("f32", False)[0], keys=kcol("all"))
    for a in c.values():
        a.setflags(write=False)
    return c


def info_of(c, members=None):
    """(n, listed, nlabels, longest) as phnsw_label_attr_info reports them, by numpy"""
    listed = (c["labels"] != NONE) & (c["keys"] != NONE)
    if members is not None:
        listed &= members
    values, counts = np.unique(c["labels"][listed], return_counts=True)
    return N, int(listed.sum()), len(values), int(counts.max())


@functools.lru_cache(maxsize=None)
def lhandle(where, kind, name):
    return make_handle(STACK, index_of(where, kind), lcol(name))


def lone(label, lo, hi):
    """the one-query batch (label, lo <= key <= hi)"""
    return spec_of([lo], [hi], np.array([label], dtype=np.int64))


def route_one(c, label=RA):
    """exactly c rows of a label of ROUTE: its ranks [25, 25 + c); c == 0: an empty range between two of its keys"""
    return lone(label, *rs.ranks(25, 25 + c))


def sample_pairs(c, count, seed):
    """`count` (label, range) pairs over a column.  Around a listed row drawn at random, in turn: its own key alone, its
    whole label, the rows of its label above it (an open end: the upper bound lands on the next label's first row), a
    range between two keys drawn at random.  Then what a lookup must miss or get right: absent labels below, between
    and above the present ones, NONE and -1, lo > hi, bounds in gaps, hi = NONE"""
    rng = np.random.default_rng(seed)
    listed = np.nonzero((c["labels"] != NONE) & (c["keys"] != NONE))[0]
    values = np.unique(c["labels"][listed])
    gaps = np.nonzero(np.diff(values) > 1)[0]
    miss = ([int(values[0]) - 1] if values[0] > 0 else []) + ([int(values[-1]) + 1] if values[-1] + 1 < NONE else [])
    miss += [int(values[g]) + 1 for g in gaps[:: max(1, len(gaps) // 6)][:6]] + [NONE, -1]
    v = listed[rng.integers(0, len(listed), count - len(miss) - 4)]
    turn = np.arange(len(v)) % 4
    key = c["keys"][v]
    r = np.sort(c["keys"][listed[rng.integers(0, len(listed), (2, len(v)))]], axis=0)
    lo = np.select([turn == 0, turn == 1, turn == 2], [key, 0, key + 1], r[0])
    hi = np.select([turn == 0, turn == 1, turn == 2], [key, TOP, NONE], r[1])
    want = c["labels"][v]
    big = int(values[np.argmax(np.unique(c["labels"][listed], return_counts=True)[1])])
    edge = [(big, 900000, 100000), (big, 0, 0), (big, NONE, NONE), (big, 1, 6)]
    want = np.concatenate([want, miss, [e[0] for e in edge]]).astype(np.int64)
    lo = np.concatenate([lo, np.zeros(len(miss), dtype=np.int64), [e[1] for e in edge]]).astype(np.int64)
    hi = np.concatenate([hi, np.full(len(miss), NONE), [e[2] for e in edge]]).astype(np.int64)
    p = rng.permutation(count)
    return spec_of(lo[p], hi[p], want[p])


def numpy_counts(c, spec, members=None):
    ids, spairs = rs.pair_order(c["labels"], c["keys"], members)
    return rs.pair_spans_of(spairs, spec["want"], spec["lo"], spec["hi"])[1]


# ---------------------------------------------------------------- 1: the handle
@pytest.mark.parametrize("name", ["one", "plat", "own", "mix", "part", "route", "far"])
def test_the_handles_describe_the_columns(name):
    w, c, h = world("f32", 24), lcol(name), lhandle("ring", "f32", name)
    hix = w["hix"]
    assert h.info() == info_of(c)                                                    # numpy
    spec = sample_pairs(c, 1000, 531)
    if name == "mix":  # an open-ended range on x runs directly against the first row of x + 1; the largest composite
        x, x1 = mix()[1]["adjacent"]
        spec["want"][:4], spec["lo"][:4], spec["hi"][:4] = [x, x, x1, TOP], [0, 1, 0, TOP], [NONE, NONE, NONE, NONE]
    counts = counts_of(STACK, h, spec)
    masks = masks_of(STACK, c, spec)
    np.testing.assert_array_equal(counts, numpy_counts(c, spec))                     # numpy: two binary searches
    np.testing.assert_array_equal(counts, masks.sum(axis=1))                         # the yardstick's masks
    np.testing.assert_array_equal(counts, hix.filter_count(masks))                   # yardstick 2
    assert (counts == 0).sum() >= 5 and (counts > 0).sum() >= 400
    if name == "mix":
        sizes = mix()[1]["sizes"]
        assert counts[:4].tolist() == [sizes[x], ((c["labels"] == x) & (c["keys"] >= 1)).sum(), sizes[x1], 1]
    if name in ("mix", "own", "one"):  # the handle made from device columns: the same figures and the same rows
        import torch
        dev = torch.device("cuda", 0)
        tl = torch.from_numpy(c["labels"].astype(np.uint32).view(np.int32)).to(dev)
        tk = torch.from_numpy(c["keys"].astype(np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize()
        dv = ph.LabeledAttribute.from_device(hix, tl.data_ptr(), tk.data_ptr(), dtype=np.int32)
        assert dv.info() == h.info()
        np.testing.assert_array_equal(counts_of(STACK, dv, spec), counts)
        sq = take(spec, slice(0, NQX))
        for form, kw, D in forms(w):
            a = host(STACK, "exact", hix, h, sq, k=K, **kw)
            same(host(STACK, "exact", hix, dv, sq, k=K, **kw), a)
            same(a, xr.exact_topk(D, masks[:NQX], None, None, K))                    # yardstick 1
        dv.close()


@pytest.mark.parametrize("name", ["mix", "one"])
def test_a_handle_over_every_second_vector(name):
    """vec2node is not the identity: odd ids carry labels and values and are listed nowhere"""
    w, c, half = world("f32", 24), lcol(name), half_index("f32", 24)
    h = make_handle(STACK, half, c)
    assert h.info() == info_of(c, EVEN) and 32768 < h.listed <= (N + 1) // 2
    spec = sample_pairs(c, NQR, 532)
    masks = masks_of(STACK, c, spec)
    counts = counts_of(STACK, h, spec)
    np.testing.assert_array_equal(counts, numpy_counts(c, spec, EVEN))               # numpy
    np.testing.assert_array_equal(counts, half.filter_count(masks))                  # yardstick 2
    np.testing.assert_array_equal(counts, (masks & EVEN).sum(axis=1))
    sq = take(spec, slice(0, NQX))
    sq["want"][0], sq["lo"][0], sq["hi"][0] = c["labels"][0], 0, NONE  # query 0 is the duplicated row: the even copies tie
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


def own_batch():
    """600 stored queries over OWN, in turn: (its label, its key alone) -- one row; (its label, the gap above its key) --
    none; (the next label in label order, no bounds) -- another row; (its label + 1, which nobody carries) -- none"""
    c, qids = lcol("own"), gworld("f32")["qids"]
    v = qids.astype(np.int64)
    assert not np.isin(v, NONE_ROWS).any()
    values = np.unique(c["labels"][c["labels"] != NONE])
    mine, key = c["labels"][v], c["keys"][v]
    nxt = values[np.minimum(np.searchsorted(values, mine) + 1, len(values) - 1)]
    turn = np.arange(NQR) % 4
    assert not np.isin(mine + 1, values).any() and (nxt != mine).all()
    want = np.select([turn < 2, turn == 2], [mine, nxt], mine + 1)
    lo = np.select([turn == 0, turn == 1], [key, key + 1], 0)
    hi = np.select([turn == 0, turn == 1], [key, key + 5], NONE)
    return spec_of(lo, hi, want), np.array([1, 0, 1, 0])[turn], turn


def test_every_row_its_own_label():
    """OWN: 69 901 labels of one row.  The spans hold 1 and 0 rows; the exact call against search_exact_filtered"""
    w, c, h = gworld("f32"), lcol("own"), lhandle("graph", "f32", "own")
    hix, qids = w["hix"], w["qids"]
    spec, rows, turn = own_batch()
    ids, spairs = rs.pair_order(c["labels"], c["keys"])
    at, ln = rs.pair_spans_of(spairs, spec["want"], spec["lo"], spec["hi"])
    assert (ln == rows).all() and len(set(at[ln > 0].tolist())) == 300               # 300 span starts, 300 empty spans
    order = rs.batch_order(at, ln)
    assert (ln[order[:300]] > 0).all() and not ln[order[300:]].any() and (np.diff(order[:300]) < 0).any()
    masks = masks_of(STACK, c, spec)
    for kw in (dict(queries=w["q"]), dict(qids=qids)):
        dv = device_call(STACK, "exact", hix, h, spec, k=10, **kw)
        assert not dv[3].any() and (dv[2] == rows.astype(np.uint64)).all()
        same(dv, hix.search_exact_filtered(allow=masks, k=10, **kw))                 # yardstick 2
        same(host(STACK, "exact", hix, h, spec, k=10, **kw), dv)
    np.testing.assert_array_equal(dv[0][turn == 0, 0], qids[turn == 0])              # a stored query finds its own row
    dv = device_call(STACK, "exact", hix, h, spec, k=10, qids=qids, exclude=qids)    # ... and nothing without it
    assert not dv[3].any() and not dv[2][turn != 2].any() and (dv[2][turn == 2] == 1).all()
    same(dv, hix.search_exact_filtered(qids=qids, allow=masks, exclude=qids, k=10))


# ---------------------------------------------------------------- 2: long spans, whatever the slices
def long_cases(kind):
    """the plateau (lo == hi: 25 040 rows with one composite, the ids ascending), BIG's 25 040 rows by distinct keys, all
    69 901 rows of PLAT"""
    flat = int(kcol("flat")[DUPS[0]])
    big = mix()[1]["big"]
    return [(lcol("plat"), lhandle("ring", kind, "plat"), lone(V_ONE, flat, flat), BIG, N - 100),
            (lcol("mix"), lhandle("ring", kind, "mix"), lone(big, 0, NONE), BIG, BIG),
            (lcol("plat"), lhandle("ring", kind, "plat"), lone(V_ONE, 0, NONE), N - 100, N - 100)]


@pytest.mark.parametrize("kind", KINDS)
def test_long_spans_whatever_the_slices(monkeypatch, kind):
    cases = long_cases(kind)
    assert [c[1].info()[3] for c in cases] == [N - 100, BIG, N - 100]                # longest clamps the slices
    long_spans_body(STACK, monkeypatch, kind, cases)


# ---------------------------------------------------------------- 3: the second turn of the item loop
def turn_spec(nq=NQT):
    """every second query asks for every row of the label, the others for everything from rank 3200 on"""
    lo = np.where(np.arange(nq) % 2 == 0, 0, int(rs.key_of_rank(3200, N)))
    return spec_of(lo, np.where(np.arange(nq) % 2 == 0, TOP, NONE), np.full(nq, V_ONE, dtype=np.int64))


def test_the_second_turn_of_the_item_loop(monkeypatch):
    """see the module docstring, gap 1"""
    c, h = lcol("one"), lhandle("ring", "f32", "one")
    spec = turn_spec()
    ids, spairs = rs.pair_order(c["labels"], c["keys"])
    at, ln = rs.pair_spans_of(spairs, spec["want"], spec["lo"], spec["hi"])
    assert h.info()[3] == N and rs.slice_count(5000, N) == FULL and rs.items(NQT, FULL) > rs.GRID_MAX
    assert set(zip(at.tolist(), ln.tolist())) == {(0, N), (3200, N - 3200)}
    order = rs.batch_order(at, ln)
    assert (order != np.arange(NQT)).sum() > 900 and order[:500].tolist() == list(range(0, NQT, 2))   # sorted[] is no identity
    assert len(rs.carrying_blocks(ln[order] > 0, FULL)) == 45424                     # every item is live
    rows = rs.second_turn_rows(order, at, ln, FULL)
    assert rows[0].tolist() == [TURN_ROW, N] and (rows[:, 1] > rows[:, 0]).all()
    rank_of_dups = np.searchsorted(spairs, rs.composites(c["labels"], c["keys"])[DUPS])
    assert ((rank_of_dups >= rows[0, 0]) & (rank_of_dups < rows[0, 1])).sum() == LATE
    second_turn_body(STACK, monkeypatch, c, h, spec, rank_of_dups)


# ---------------------------------------------------------------- 4: the routed call past 256 queries
def test_the_routed_call_over_three_blocks_of_queries():
    """scan_below = 0: pairs of 20 000 rows scan and pairs of 20 001 walk; 10 938 = e rows scan by the first rule although
    the second would let them go"""
    e = first_graph()
    assert e == ROUTE_SCANS[-1] <= BELOW[STACK] and ar.rule(e, 100, SP[0], K, N) == ar.GRAPH
    assert [ar.rule(x, BELOW[STACK], SP[0], K, N) for x in ROUTE_SCANS + (ROUTE_WALK,)] == [ar.SCAN] * 8 + [ar.GRAPH]
    c, h = lcol("route"), lhandle("graph", "f32", "route")
    scans = join([route_one(ROUTE_SCANS[i % 8], (RA, RB)[i % 2]) for i in range(NQR)])
    turn = [route_one(ROUTE_WALK), route_one(e, RC), route_one(20000, RB), lone(ABSENT, 0, NONE), route_one(ROUTE_WALK, RB),
            route_one(19999), route_one(1, RE), lone(NONE, 0, NONE), lone(RE, 0, NONE)]
    mixed = join([turn[i % 9] for i in range(NQR)])
    walks_at = np.isin(np.arange(NQR) % 9, (0, 4))
    assert sorted(set(counts_of(STACK, h, scans).tolist())) == sorted(ROUTE_SCANS)
    assert counts_of(STACK, h, join(turn)).tolist() == [ROUTE_WALK, e, 20000, 0, ROUTE_WALK, 19999, 1, 0, 26]
    three_blocks_body(STACK, c, h, scans, mixed, walks_at)


@pytest.mark.parametrize("scan_first", [True, False])
def test_a_block_of_scans_next_to_blocks_of_walks(scan_first):
    scans = [route_one(20000), route_one(10938, RC), lone(ABSENT, 0, NONE), route_one(19999, RB), lone(NONE, 0, TOP), route_one(1, RE)]
    scans_next_to_walks_body(STACK, lcol("route"), lhandle("graph", "f32", "route"), scans, route_one(ROUTE_WALK, RB), scan_first)


def far_spec(want):
    """far_batch's wanted labels with, in turn, no bounds and the bounds of the whole column"""
    nq = len(want)
    return spec_of(np.zeros(nq, dtype=np.int64), np.where(np.arange(nq) % 2 == 0, NONE, TOP), np.asarray(want, dtype=np.int64))


@pytest.mark.parametrize("stored", [False, True])
def test_an_explicit_threshold_and_the_rescan_past_256_queries(stored):
    far_body(STACK, lcol("far"), lhandle("graph", "f32", "far"), far_spec(far_batch("f32", stored)[1]), stored)


@pytest.mark.parametrize("kind", ["i8q", "pq"])
def test_the_routed_call_on_the_other_kinds(kind):
    turn = [route_one(ROUTE_WALK), route_one(10938, RC), route_one(20000, RB), lone(ABSENT, 0, NONE), route_one(ROUTE_WALK, RB)]
    got = routed_check(STACK, gworld(kind), lcol("route"), lhandle("graph", kind, "route"), join([turn[i % 5] for i in range(NQR)]),
                       device=True)
    both_routes_in_every_wave(got[3])
    np.testing.assert_array_equal(got[3] == ar.SCAN, ~np.isin(np.arange(NQR) % 5, (0, 4)))


# ---------------------------------------------------------------- 5: the walk by label and range at N > 65 536
def walk_spec():
    """20 001 rows of a label, a wanted NONE, 10 938 rows, a whole label without bounds, an absent label, lo > hi with
    keys between, 5001 rows"""
    turn = [route_one(ROUTE_WALK), lone(NONE, 0, NONE), route_one(10938, RC), lone(RB, 0, NONE), lone(ABSENT, 0, NONE),
            lone(RA, 9000, 2000), route_one(5001, RB)]
    return join([turn[i % 7] for i in range(NQR)]), np.isin(np.arange(NQR) % 7, (1, 4, 5))


def test_the_walk_by_label_and_range_at_scale():
    spec, empty_at = walk_spec()
    walk_body(STACK, lcol("route"), lhandle("graph", "f32", "route"), spec, empty_at)


# ---------------------------------------------------------------- 6: wide queries
def test_wide_queries():
    wide_body(STACK, lcol("route"), lhandle("graph", "f32", "route"), walk_spec()[0])
