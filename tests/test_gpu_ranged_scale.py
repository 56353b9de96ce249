"""Run time on an MI355X: 11 s (22 cases, first clean run, the slowest 1.6 s); run it under `timeout -k 10 33`, three times that.

The range stack (phnsw_attr_*, filter_ranged.hip, range_plan.h, the search kernels' range mode, phnsw_search_ranged_auto)
at the smallest shapes where its loops turn more than once, on the worlds of tests/test_gpu_filter_scale.py: World A,
N = 70 001 rows with 40 copies of row 0 at DUPS, its built graph and its every-second-vector index, imported and never
rebuilt.  tests/test_gpu_exact_ranged.py, test_gpu_ranged_walk.py and test_gpu_ranged_auto.py cover kinds, dimensions,
metrics and refusals on 2000 and 5000 rows with at most 132 queries.  Every comparison here is on ids, distance bits,
lengths, status, routes and stats, no tolerance anywhere.  This module also holds what the three range scale modules
share (tests/test_gpu_label_ranged_scale.py and tests/test_gpu_labelset_ranged_scale.py import it): the calls of a stack
by name, the device forms with guard words, and the bodies of the tests that differ by stack in their inputs alone.

The key columns are constructed, not drawn (tests/ranged_scale_reference.py, pinned by tests/test_ranged_scale_cpu.py):
the row of rank r carries key r * 61 356 + 7 (rank 0: key 0, the top rank: 0xFFFFFFFE), the rows take their ranks in a
random order, so a span of exactly c rows from rank r is (key(r), key(r + c - 1)).  ALL lists every row (listed == N: the
head is written at p == n), SOME leaves 100 rows without a value (69 901 listed, 1093 batches), FLAT has a plateau of
25 040 rows with ONE key, the 40 copies among them (392 batches).  In ALL and SOME the copies take ranks spread over the
whole order, the six smallest ids among them at ranks from 67 136 on.

The seven gaps, each with the test that closes it and the shape it asserts:
  1. the item loop of ph_ranged_scan_kernel past the 2^20-block clamp -- test_the_second_turn_of_the_item_loop: 1000
     queries x 1094 slices (PHNSW_RANGE_SLICES=5000 clamped by listed = 70 001) = 1 094 000 items > 1 048 576, so 45 424
     blocks carry their LDS from a live item into a live item; every second query asks for everything and the others
     for everything from rank 3200 on, so sorted[] is no identity; query 0 is the duplicated row at k = 40 and six of
     the copies in its row sit at span ranks >= 67 136, which only second-turn items read.  All asserted from the
     restated rules before the call.
  2. construction past one sort tile and 2^16 rows -- test_the_handles_describe_the_columns (info of ALL, SOME, FLAT and
     FAR against numpy; from_device; about 1000 counted ranges against numpy and filter_count) and
     test_a_handle_over_every_second_vector (vec2node no identity).
  3. the per-call sort past one tile -- the 1000 queries of test 1 and test_spans_of_one_row_and_of_none: 600 queries,
     300 different span starts and 300 empty spans between them.
  4. a slice that overflows k = 1024 -- test_long_spans_whatever_the_slices: k = 1024 under 1 and 3 slices of 392 and
     1093 batches: every slice sees more than 8000 candidates and evicts.
  5. the shipped threshold -- test_the_routed_call_*: 600 queries = 3 trips of ph_auto_route_kernel, scan_below = 0
     parts 20 000 from 20 001 rows, 10 938 rows scan by the first rule; both routes in every wave of 64, so the scan's
     subset form (PhRangedCall::list) gets a scattered list of more than 400 queries; a block of 256 scans next to
     blocks of walks; an explicit threshold of 100 and the rescan past the first 256 queries.
  6. the walk's range mode at N > 65 536 -- test_the_walk_by_range_at_scale.
  7. a wide query matrix -- test_wide_queries: ldq = ld + 8 with NaN behind every row, the three device calls.

Yardsticks, named where they are applied: (1) tests/exact_filter_reference.exact_topk over World A's oracle distances
with the masks tests/ranged_reference.masks_of makes of the column, which the code under test never sees (the 65 queries
of world() on f32, i8q and pq); (2) the established bitmap calls on the same masks -- search_exact_filtered,
search_batch_filtered, filter_auto_reference.compose / rule / assert_complete over both, filter_count -- which
tests/test_gpu_filter_scale.py pins against the oracle on this very world; it carries the 600- and 1000-query cases and
the f16 / i8 stores.

Not exercised: the 65 536-block clamp of grid1 (n or nq past 16.7 M), the 2^20 clamp of ph_list_merge_kernel (more than
1 048 576 queries), nq near PH_LABEL_NQ_MAX, a third turn of the item loop (items past 2^21), and the UNMEASURED
thresholds themselves: these tests pin what scan_below = 0 does today, through ar.rule with the constants of
filter_route.h.  No test was run against a deliberately broken kernel; what each would show is reasoned from its inputs:
were second-turn items dropped, or given the position of the block's first item, the row of query 0 would lack the six
copies with the smallest ids, which sit at span ranks only second-turn items read."""
import functools

import numpy as np
import pytest

import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import filter_auto_reference as ar
import filter_scale_reference as sr
import label_ranged_reference as lrr
import labeled_scale_reference as ls
import labelset_ranged_reference as srr
import ranged_reference as rr
import ranged_scale_reference as rs
from test_gpu_exact_filter import same
from test_gpu_filter_scale import (DUPS, EVEN, K, N, NQR, NQX, SP, both_routes_in_every_wave, first_graph, gworld, half_index,
                                   rows_a, world)
from test_gpu_i8 import bits
from test_gpu_i8q import env
from test_gpu_labeled_scale import (ABSENT_ROUTE, FULL, NONE_ROWS, NQT, TURN_ROW, cut, far_batch, forms, lworld, padded, turn_queries,
                                    without)

pytestmark = pytest.mark.gpu

EMPTY, NONE, TOP = xr.EMPTY, rs.NONE, rs.TOP
SLICES = (None, "1", "2", "3", "7", "391", "392", "1093", "5000")
KINDS = ["f32", "i8q", "pq", "f16", "i8"]
SUFFIX = {"range": "ranged", "label": "label_ranged", "set": "labelset_ranged"}
KNOB = {"range": "PHNSW_RANGE_SLICES", "label": "PHNSW_LABEL_RANGE_SLICES", "set": "PHNSW_LABELSET_RANGE_SLICES"}
BELOW = {"range": 20000, "label": 20000, "set": 5000}  # filter_route.h: PH_AUTO_SCAN_BELOW_RANGED, _LABEL_RANGED, _LABELSET_RANGED
KT = 40        # k of the second-turn case: all 40 copies
BIG = 25040    # rows of the plateau and of the long span: 392 batches
LATE = 6       # copies at span ranks from TURN_ROW on

# the shapes the modules are about, on the CPU at collection
assert rs.batches(N) == FULL == 1094 and rs.batches(N - 100) == 1093 and rs.batches(BIG) == 392 and N % 256 == 113 and N > 65536
assert rs.items(NQT, FULL) == 1094000 > rs.GRID_MAX and len(rs.both_turns(NQT, FULL, NQT)) == 45424
assert ls.second_turn_first_row(NQT, FULL, N) == (TURN_ROW - 64, TURN_ROW) == (67072, 67136)
assert rs.slice_count(5000, N) == FULL and rs.slice_count(5000, N - 100) == 1093 and rs.slice_count(5000, BIG) == 392
assert first_graph() == 10938 and sr.trips(NQR, sr.ROUTE_QUERIES) == 3


def dup_ranks(listed):
    """{copy: rank}: the six smallest ids among the copies at ranks from TURN_ROW on, the others spread from rank 3 on"""
    late = [TURN_ROW, TURN_ROW + 63, TURN_ROW + 704, 68500, 69300, listed - 11]
    early = np.linspace(3, 66500, len(DUPS) - LATE).astype(np.int64).tolist()
    return dict(zip(DUPS.tolist(), late + early))


# ---------------------------------------------------------------- columns
@functools.lru_cache(maxsize=None)
def kcol(name):
    """the key of every row, i64 [N] (NONE: no value), constructed; each asserts its own counts"""
    if name == "all":
        keys, rank_of = rs.ranked_column(N, 501, dup_ranks(N))
        assert (keys != NONE).all()
    elif name == "some":
        keys, rank_of = rs.ranked_column(N, 502, dup_ranks(N - 100), NONE_ROWS)
        assert (keys == NONE).sum() == 100
    elif name == "flat":
        keys, flat = rs.plateau_column(N, 503, DUPS, 20000, BIG, NONE_ROWS)
        assert (keys == flat).sum() == BIG and (keys[DUPS] == flat).all() and (keys == NONE).sum() == 100
    elif name == "mix":   # for the labels of MIX: the one row of label 0xFFFFFFFE carries key 0xFFFFFFFE, the largest composite
        from test_gpu_labeled_scale import mix
        top_row = np.nonzero(mix()[0] == TOP)[0]
        assert len(top_row) == 1 and top_row[0] not in DUPS
        keys, rank_of = rs.ranked_column(N, 504, {**dup_ranks(N), int(top_row[0]): N - 1})
        assert keys[top_row[0]] == TOP
    elif name == "part":  # MIX's keys but for 300 rows that carry a label and no value
        from test_gpu_labeled_scale import mix
        keys = kcol("mix").copy()
        pool = np.setdiff1d(np.nonzero(mix()[0] != NONE)[0], DUPS)
        keys[np.random.default_rng(505).permutation(pool)[:300]] = NONE
        assert (keys == NONE).sum() == 300 and not (keys[NONE_ROWS] == NONE).any()
    elif name == "far":   # the far rows of tests/test_gpu_labeled_scale.far_column, label by label, then the others
        lab = far_batch("f32", False)[0]
        o = np.argsort(lab, kind="stable")
        keys = np.empty(N, dtype=np.int64)
        keys[o] = rs.key_of_rank(np.arange(N), N)
        assert [(lab[o[j * first_graph():(j + 1) * first_graph()]] == j + 1).all() for j in range(4)] == [True] * 4
    if name in ("all", "some", "mix"):
        listed = int((keys != NONE).sum())
        ids, skeys = rs.span_order(keys)
        assert (np.diff(skeys) > 0).all() and skeys[0] == 0 and skeys[-1] == TOP
        assert (np.diff(ids) < 0).sum() > 30000                                     # span order is not id order
        assert (rank_of[DUPS] >= TURN_ROW).sum() == LATE and (rank_of[DUPS[:LATE]] >= TURN_ROW).all()
        assert rank_of[DUPS].max() < listed and len(set((rank_of[DUPS] // 64).tolist())) == 39  # (two share batch 1049)
    keys.setflags(write=False)
    return keys


def values_of(keys):
    """the int32 values whose keys these are: the columns are held as int32, whose map covers every u32 key a bound can
    be (INT32_MAX is the key 0xFFFFFFFF, no upper end)"""
    return (np.asarray(keys).astype(np.uint32) ^ np.uint32(0x80000000)).view(np.int32)


def make_handle(stack, hix, col):
    keys = col["keys"]
    missing = keys == NONE
    vals = values_of(np.where(missing, 0, keys))
    if stack == "range":
        return ph.Attribute(hix, vals, missing=missing)
    return ph.LabeledAttribute(hix, col["labels"], vals, missing=missing)


def rcol(name):
    return dict(keys=kcol(name), labels=None)


def index_of(where, kind):
    return {"ring": lambda: lworld(kind)["hix"], "graph": lambda: gworld(kind)["hix"], "half": lambda: half_index(kind, 24)}[where]()


@functools.lru_cache(maxsize=None)
def rhandle(where, kind, name):
    return make_handle("range", index_of(where, kind), rcol(name))


# ---------------------------------------------------------------- a batch of one stack, its masks, its calls
def spec_of(lo, hi, want=None):
    """the filter of every query of a batch: lo, hi u32 keys as i64 [nq]; want: labels i64 [nq] ("label"), a list of nq
    sequences of labels ("set"), None ("range")"""
    return dict(lo=np.asarray(lo, dtype=np.int64), hi=np.asarray(hi, dtype=np.int64), want=want)


def take(spec, idx):
    idx = np.arange(len(spec["lo"]))[idx]
    w = spec["want"]
    if w is not None:
        w = [w[i] for i in idx] if isinstance(w, list) else np.asarray(w)[idx]
    return dict(lo=spec["lo"][idx], hi=spec["hi"][idx], want=w)


def masks_of(stack, col, spec, members=None):
    """the bitmaps the batch stands for, from the yardsticks' modules: the code under test never sees them"""
    if stack == "range":
        return rr.masks_of(col["keys"], spec["lo"], spec["hi"], members)
    if stack == "label":
        return lrr.masks_of(col["labels"], col["keys"], rs.u32(spec["want"]), spec["lo"], spec["hi"], members)
    return srr.masks_of(col["labels"], col["keys"], spec["want"], spec["lo"], spec["hi"], members)


def host(stack, which, hix, h, spec, **kw):
    """search_exact_* ("exact"), search_batch_* ("walk") or the routed search_* ("auto") of the stack, host form"""
    a = dict(attr=h, lo=values_of(spec["lo"]), hi=values_of(spec["hi"]))
    if stack != "range":
        a["want"] = spec["want"]
    name = {"exact": "search_exact_%s", "walk": "search_batch_%s", "auto": "search_%s"}[which] % SUFFIX[stack]
    return getattr(hix, name)(**a, **kw)


def counts_of(stack, h, spec):
    lo, hi = values_of(spec["lo"]), values_of(spec["hi"])
    if stack == "range":
        return h.count(lo, hi)
    return h.count(spec["want"], lo, hi) if stack == "label" else h.count_sets(spec["want"], lo, hi)


def device_call(stack, which, hix, h, spec, k=K, sp=None, queries=None, qids=None, exclude=None, strict=False, scan_below=0,
                stream=None, wide=0):
    """the device form of the stack's exact scan ("exact"), walk ("walk") or routed call ("auto") with torch buffers; 64
    guard words behind every output must come back as they went in.  wide: ldq = ld + wide, the columns past ld filled
    with NaN (those from dim to ld are zero).
    -> ids u64, d, len u64, then status ("exact"); stats, status ("walk"); route, status ("auto")"""
    import torch
    dev = torch.device("cuda", 0)
    keep = []

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr() if t.numel() else 0

    def up32(a):
        return up(np.asarray(a).astype(np.uint32).view(np.int32))

    nq = len(queries) if queries is not None else len(qids)
    width = sp.number_of_candidates if which == "walk" else k
    kw = dict(queries=0, ldq=0, qids=0, exclude=0)
    if queries is not None:
        ld = hix.store.ld
        qp = np.full((nq, ld + wide), np.nan, dtype=np.float32)
        qp[:, :ld] = 0.0
        qp[:, :queries.shape[1]] = queries
        kw["queries"], kw["ldq"] = up(qp), ld + wide
    else:
        kw["qids"] = up32(qids)
    if exclude is not None:
        e = np.asarray(exclude, dtype=np.uint64).copy()
        e[e > 0xFFFFFFFF] = 0xFFFFFFFF
        kw["exclude"] = up32(e)
    kw["lo"], kw["hi"] = up32(spec["lo"]), up32(spec["hi"])
    head = [h, nq]
    if stack == "label":
        kw["want"] = up32(rs.u32(spec["want"]))
    elif stack == "set":
        first, values = rs.csr(spec["want"])
        kw["want_first"], kw["want_values"] = up32(first), up32(values)
        head.append(len(values))
    G = 64
    ids = torch.full((nq * width + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * width + G,), -1.0, dtype=torch.float32, device=dev)
    ln, status, route = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    st = torch.full((2 * nq + G,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    kw["stream"] = 0 if stream is None else stream.cuda_stream
    outs = (ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr())
    if which == "exact":
        getattr(hix, "search_exact_%s_device" % SUFFIX[stack])(*head, k, *outs, **kw)
    elif which == "walk":
        getattr(hix, "search_batch_%s_device" % SUFFIX[stack])(*head, sp, *outs, strict=strict, out_stats=st.data_ptr(), **kw)
    else:
        getattr(hix, "search_%s_device" % SUFFIX[stack])(*head, sp, k, *outs, scan_below=scan_below, out_route=route.data_ptr(), **kw)
    torch.cuda.synchronize()
    assert (ids[nq * width:] == 7).all() and (d[nq * width:] == -1.0).all()
    assert (ln[nq:] == -1).all() and (status[nq:] == -1).all()
    assert (st[2 * nq:] == -1).all() and (which == "walk" or (st == -1).all())
    assert (route[nq:] == -1).all() and (which == "auto" or (route == -1).all())
    i64 = ids[:nq * width].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, width)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    out = (i64, d[:nq * width].cpu().numpy().reshape(nq, width), ln[:nq].cpu().numpy().view(np.uint32).astype(np.uint64))
    if which == "walk":
        out += (st[:2 * nq].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(nq, 2),)
    if which == "auto":
        out += (route[:nq].cpu().numpy().view(np.uint32),)
    return out + (status[:nq].cpu().numpy(),)


def knob(stack, slices):
    return {} if slices is None else {KNOB[stack]: str(slices)}


# ---------------------------------------------------------------- bodies shared by the three stacks
def long_spans_body(stack, monkeypatch, kind, cases):
    """cases: (col, handle, spec of one query, rows of its span, what clamps the slice count).  Every query of the 65
    asks for that span; rows at k = 10 and at k = 1024 under every knob, the device form, exclude in turn the best hit, an id outside the span, an id past n, EMPTY"""
    w = lworld(kind)
    hix = w["hix"]
    for col, h, one, length, clamp in cases:
        allow = masks_of(stack, col, one)[0]
        assert allow.sum() == length == counts_of(stack, h, one)[0] and (allow[DUPS].all() or length < N - 100)
        assert rs.slice_count(5000, clamp) == rs.batches(clamp) >= 392 and rs.batches(length) >= 392
        assert min(b - a for a, b in rs.slice_ranges(length, 3)) * rs.BATCH > 8 * ls.KMAX  # a slice overflows k = 1024
        outside = int(np.nonzero(~allow)[0][7])
        for form, kw, D in forms(w):
            nq = len(next(iter(kw.values())))
            spec = take(one, [0] * nq)
            y1 = None if D is None else xr.exact_topk(D, allow, None, None, 1024)
            y2 = hix.search_exact_filtered(allow=allow, k=10, **kw)
            base = None
            for slices in SLICES:
                with env(monkeypatch, **knob(stack, slices)):
                    got = host(stack, "exact", hix, h, spec, k=10, **kw)
                    dv = device_call(stack, "exact", hix, h, spec, k=10, **kw) if slices in (None, "3", "5000") else None
                padded(got, 10)
                if slices is None:
                    base = got
                    same(got, y2)                      # yardstick 2
                    if y1 is not None:
                        same(got, cut(y1, 10))         # yardstick 1
                else:
                    same(got, base)                    # rows do not depend on the slice count
                if dv is not None:
                    assert not dv[3].any()
                    same(dv, base)
            # k = 1024: under 1 and 3 slices every slice holds more than 8 * 1024 candidates and evicts
            y2 = hix.search_exact_filtered(allow=allow, k=1024, **kw)
            for slices in SLICES:
                with env(monkeypatch, **knob(stack, slices)):
                    got = host(stack, "exact", hix, h, spec, k=1024, **kw)
                same(got, y2)                          # yardstick 2
                if y1 is not None:
                    same(got, y1)                      # yardstick 1
                assert (got[2] == 1024).all()
                if kind not in ("i8q", "pq") and allow[DUPS].all():  # normalised rows: nothing is nearer to a row than its copies
                    np.testing.assert_array_equal(got[0][0, :40], DUPS.astype(np.uint64))  # the 40 copies tie: the ids decide
                    assert len(set(bits(got[1][0, :40]).tolist())) == 1
            best = base[0][:, 0]
            ex = np.array([(int(best[i]), outside, N + 7, EMPTY)[i % 4] for i in range(nq)], dtype=np.uint64)
            y2 = hix.search_exact_filtered(allow=allow, exclude=ex, k=10, **kw)
            for slices in (None, "3"):
                with env(monkeypatch, **knob(stack, slices)):
                    got = host(stack, "exact", hix, h, spec, exclude=ex, k=10, **kw)
                    dv = device_call(stack, "exact", hix, h, spec, k=10, exclude=ex, **kw)
                same(got, y2)                          # yardstick 2
                if y1 is not None:
                    same(got, without(y1, ex, 10))     # yardstick 1
                assert not dv[3].any()
                same(dv, got)
                assert not (got[0][0::4] == best[0::4, None]).any()
                same(tuple(x[1::4] for x in got), tuple(x[1::4] for x in base))  # an id outside the span changes nothing


def turn_world():
    """World A's ring index, the 1000 stored ids of tests/test_gpu_labeled_scale.turn_queries (world()'s 65 first) and the
    same rows as raw queries: raw query 0 is the duplicated row, stored query 0 one of its copies"""
    w = world("f32", 24)
    qids, _ = turn_queries()
    assert (qids[:NQX] == w["qids"]).all() and qids[0] == DUPS[3]
    raw = np.concatenate([w["q"], rows_a(False, 24)[qids[NQX:].astype(np.int64)]])
    assert (raw[0] == rows_a(False, 24)[0]).all()
    return w, qids, raw


def second_turn_body(stack, monkeypatch, col, h, spec, rank_of_dups, k=KT, nq=NQT):
    """nq queries (1000, or the first 400 of them) under the stack's knob at 5000, clamped to 1094 slices: the shape is
    asserted by the caller from the restated rules; here the rows against yardstick 2 (all of them) and yardstick 1 (the
    first 65), the device form on a side stream for both query forms and the host form once"""
    import torch
    w, qids, raw = turn_world()
    qids, raw = qids[:nq], raw[:nq]
    hix = w["hix"]
    masks = masks_of(stack, col, spec)
    assert masks[0][DUPS].all()
    late = DUPS[rank_of_dups >= TURN_ROW]
    assert len(late) == LATE and (late == DUPS[:LATE]).all()
    y2 = {0: hix.search_exact_filtered(queries=raw, allow=masks, k=k), 1: hix.search_exact_filtered(qids=qids, allow=masks, k=k)}
    y1 = {0: xr.exact_topk(w["Dq"], masks[:NQX], None, None, k), 1: xr.exact_topk(w["Ds"], masks[:NQX], None, None, k)}
    stream = torch.cuda.Stream()
    for form, kw in ((1, dict(qids=qids)), (0, dict(queries=raw))):
        with env(monkeypatch, **knob(stack, 5000)):
            dv = device_call(stack, "exact", hix, h, spec, k=k, stream=stream, **kw)
        assert not dv[3].any()
        same(dv, y2[form])                                        # yardstick 2, all 1000
        same(tuple(x[:NQX] for x in dv), y1[form])                # yardstick 1, the first 65
        # the duplicated row (and its copy): the copies tie for the first places, the ids decide, and the smallest ids
        # are those whose span ranks only a second-turn item reads
        np.testing.assert_array_equal(dv[0][0, :min(k, 40)], DUPS[:min(k, 40)].astype(np.uint64))
        assert np.isin(late, dv[0][0].astype(np.int64)).all()
    with env(monkeypatch, **knob(stack, 5000)):
        same(host(stack, "exact", hix, h, spec, qids=qids, k=k), y2[1])   # the host form, once
    # 958 queries: 958 * 1094 <= 2^20, the grid is not clamped -- the same rows
    assert rs.items(958, FULL) <= rs.GRID_MAX
    if stack != "set":
        with env(monkeypatch, **knob(stack, 5000)):
            dv = device_call(stack, "exact", hix, h, take(spec, slice(0, 958)), k=k, qids=qids[:958], stream=stream)
        same(dv, tuple(x[:958] for x in y2[1]))


def routed_check(stack, w, col, h, spec, scan_below=0, exclude=None, stored=False, device=False, q=None, qids=None, sp=SP, k=K):
    """the host form (and the device form on a side stream) against ROWS, ROUTES and COMPLETE as
    tests/test_gpu_ranged_auto.py names them, with compose over the two bitmap calls (yardstick 2); scan_below = 0: the
    library's threshold for the stack decides.  Returns the host result."""
    hix, spp = w["hix"], ph.SearchParameters(*sp)
    kw = dict(qids=w["qids"] if qids is None else qids) if stored else dict(queries=w["q"] if q is None else q)
    below = scan_below or BELOW[stack]
    masks = masks_of(stack, col, spec)
    got = host(stack, "auto", hix, h, spec, sp=spp, exclude=exclude, k=k, scan_below=scan_below, route=True, **kw)
    walk = hix.search_batch_filtered(sp=spp, allow=masks, strict=True, exclude=exclude, **kw)
    scan = hix.search_exact_filtered(allow=masks, exclude=exclude, k=k, **kw)
    ref = ar.compose(walk, scan, N, sp[0], k, N, masks, exclude, None, below)
    print("routes", np.bincount(got[3], minlength=3).tolist(), "expected", np.bincount(ref[3], minlength=3).tolist())
    np.testing.assert_array_equal(got[3], ref[3])      # ROWS: which graph rows the strict bitmap call leaves short
    same(got, ref)                                      # ROWS
    counts = counts_of(stack, h, spec)
    np.testing.assert_array_equal(counts, masks.sum(axis=1))
    np.testing.assert_array_equal(counts, hix.filter_count(masks))
    for i in range(len(counts)):                        # ROUTES
        r = ar.rule(counts[i], below, sp[0], k, N)
        assert got[3][i] == r or (got[3][i] == ar.GRAPH_THEN_SCAN and r == ar.GRAPH), (i, got[3][i], r)
    ar.assert_complete(got, N, k, masks, exclude, None)  # COMPLETE
    if device:
        import torch
        dv = device_call(stack, "auto", hix, h, spec, k=k, sp=spp, exclude=exclude, scan_below=scan_below,
                         stream=torch.cuda.Stream(), **kw)
        assert not dv[4].any()
        same(dv, got)
        np.testing.assert_array_equal(dv[3], got[3])
    return got


def nearest_exclude(stack, w, h, spec, **kw):
    return host(stack, "exact", w["hix"], h, spec, k=1, **kw)[0][:, 0].copy()


def three_blocks_body(stack, col, h, scans, mixed, walks_at, sp=SP, k=K):
    """scans: a spec whose 600 queries all scan; mixed: one with both routes in every wave, walks_at bool [600] the
    queries that walk.  Host and device form, raw and stored, with and without the nearest candidate as exclude"""
    w = gworld("f32")
    got = routed_check(stack, w, col, h, scans, device=True, sp=sp, k=k)
    assert (got[3] == ar.SCAN).all()
    for stored in (False, True):
        got = routed_check(stack, w, col, h, mixed, stored=stored, device=not stored, sp=sp, k=k)
        np.testing.assert_array_equal(got[3] == ar.SCAN, ~walks_at)
        both_routes_in_every_wave(got[3])
    ex = nearest_exclude(stack, w, h, mixed, queries=w["q"])   # exclude: each query's nearest candidate, EMPTY where none
    got = routed_check(stack, w, col, h, mixed, exclude=ex, device=True, sp=sp, k=k)
    assert not ((got[0] == ex[:, None]) & (ex[:, None] != EMPTY)).any() and (ex == EMPTY).any() and (ex != EMPTY).any()


def scans_next_to_walks_body(stack, col, h, scan_specs, walk_spec, scan_first, sp=SP, k=K):
    """a block of 256 scans next to blocks of walks (scan_first) or 256 walks in front of 344 scans.  scan_specs /
    walk_spec: one-query specs the batch cycles through"""
    w = gworld("f32")
    ns = sr.ROUTE_QUERIES if scan_first else NQR - sr.ROUTE_QUERIES
    parts = [[scan_specs[i % len(scan_specs)] for i in range(ns)], [walk_spec] * (NQR - ns)]
    walks_at = np.arange(NQR) >= ns if scan_first else np.arange(NQR) < NQR - ns
    spec = join(parts[0] + parts[1] if scan_first else parts[1] + parts[0])
    got = routed_check(stack, w, col, h, spec, stored=not scan_first, device=scan_first, sp=sp, k=k)
    np.testing.assert_array_equal(got[3] == ar.SCAN, ~walks_at)
    head = got[3][:sr.ROUTE_QUERIES] == ar.SCAN
    assert head.all() == scan_first and head.any() == scan_first


def join(ones):
    """one batch of one-query specs"""
    w = None
    if ones[0]["want"] is not None:
        w = [o["want"][0] for o in ones]
        w = w if isinstance(ones[0]["want"], list) else np.array(w, dtype=np.int64)
    return dict(lo=np.array([o["lo"][0] for o in ones], dtype=np.int64), hi=np.array([o["hi"][0] for o in ones], dtype=np.int64), want=w)


def far_body(stack, col, h, spec, stored):
    """scan_below = 100, so e = 10 938 decides.  The far-rows construction of tests/test_gpu_labeled_scale.far_column: a
    query that wants the e rows farthest from itself walks towards rows it may not return, comes back short of k and is
    scanned again (GRAPH_THEN_SCAN), at 20 places past the first 256 queries.  The precondition is asserted on the
    established strict bitmap call"""
    w = gworld("f32")
    _, _, q, qids, places = far_batch("f32", stored)
    e = first_graph()
    assert ar.rule(e, 100, SP[0], K, N) == ar.GRAPH and ar.rule(e - 1, 100, SP[0], K, N) == ar.SCAN and places.min() >= sr.ROUTE_QUERIES
    kw = dict(qids=qids) if stored else dict(queries=q)
    masks = masks_of(stack, col, spec)
    assert (masks[places].sum(axis=1) == e).all()
    strict = w["hix"].search_batch_filtered(sp=ph.SearchParameters(*SP), allow=masks, strict=True, **kw)
    print("strict bitmap rows shorter than k at the far places:", (strict[2][places] < K).sum(), "of", len(places))
    assert (strict[2][places] < K).any()  # the precondition, on the established call
    got = routed_check(stack, w, col, h, spec, scan_below=100, stored=stored, device=True, q=q, qids=qids)
    assert (got[3][places] == ar.GRAPH_THEN_SCAN).any() and (got[3] == ar.GRAPH).any() and (got[3] == ar.SCAN).any()
    assert (got[3][places] != ar.SCAN).all()
    ex = nearest_exclude(stack, w, h, spec, **kw)
    got = routed_check(stack, w, col, h, spec, scan_below=100, exclude=ex, stored=stored, q=q, qids=qids)
    assert not ((got[0] == ex[:, None]) & (ex[:, None] != EMPTY)).any()
    assert (got[3][places] == ar.GRAPH_THEN_SCAN).any()


def walk_body(stack, col, h, spec, empty_at):
    """rows, lengths and stats of search_batch_filtered with the masks, bit for bit (yardstick 2); empty_at bool [600]: the
    queries whose filter holds nothing (a wanted NONE, an absent label, lo > hi, an empty set): nothing under strict"""
    w = gworld("f32")
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    masks = masks_of(stack, col, spec)
    assert N > 65536 and empty_at.any() and not masks[empty_at].any() and masks[~empty_at].any(axis=1).all()
    assert (np.nonzero(masks.any(axis=0))[0] > 65536).any()
    ex = (w["qids"] + 1) % N
    for kw in (dict(queries=w["q"]), dict(qids=w["qids"])):
        for strict in (False, True):
            for e in (None, ex):
                ref = hix.search_batch_filtered(sp=spp, allow=masks, strict=strict, exclude=e, stats=True, **kw)
                got = host(stack, "walk", hix, h, spec, sp=spp, strict=strict, exclude=e, stats=True, **kw)
                same(got, ref)
                np.testing.assert_array_equal(got[3], ref[3])
                dv = device_call(stack, "walk", hix, h, spec, sp=spp, strict=strict, exclude=e, **kw)
                assert not dv[4].any()
                same(dv, ref)
                np.testing.assert_array_equal(dv[3], ref[3])
            if strict:  # nothing, not even the entry vector
                assert (got[2] > 0).any() and not got[2][empty_at].any()


def wide_body(stack, col, h, spec):
    """ldq = ld + 8: the rows of the ldq == ld call.  NaN fills the columns past ld: a kernel that read a query row at
    the store's stride, or past ld, would return other rows"""
    w = gworld("f32")
    hix, q, spp = w["hix"], w["q"], ph.SearchParameters(*SP)
    assert hix.store.ld >= 24 and hix.store.ld % 4 == 0
    for which, kw in (("exact", dict(k=K)), ("walk", dict(sp=spp, strict=True)), ("auto", dict(sp=spp, k=K, scan_below=100))):
        narrow = device_call(stack, which, hix, h, spec, queries=q, **kw)
        wide = device_call(stack, which, hix, h, spec, queries=q, wide=8, **kw)
        assert not narrow[-1].any() and not wide[-1].any() and narrow[2].any()
        same(wide, narrow)
        for a, b in zip(wide[3:], narrow[3:]):  # stats or routes, status
            np.testing.assert_array_equal(a, b)
        if which == "exact":  # and the narrow rows are the established scan's (yardstick 2)
            same(narrow, hix.search_exact_filtered(queries=q, allow=masks_of(stack, col, spec), k=K))
        if which == "walk":
            same(narrow, hix.search_batch_filtered(queries=q, sp=spp, allow=masks_of(stack, col, spec), strict=True, stats=True))


# ---------------------------------------------------------------- the range stack's inputs
def span(name, r, c):
    return rs.span(r, c, int((kcol(name) != NONE).sum()))


def rspec(name, spans):
    """the batch whose query i wants the c rows from rank r, (r, c) = spans[i]; c < 0: (r, -c) with no upper end"""
    b = [span(name, r, abs(c)) for r, c in spans]
    return spec_of([x[0] for x in b], [NONE if c < 0 else x[1] for x, (_, c) in zip(b, spans)])


def sample_ranges(keys, count, seed):
    """`count` ranges over a column: spans cut at random ranks, then what a lookup must get right -- lo > hi with keys
    between, bounds in gaps, hi = NONE, lo = NONE, the first and the last key alone, everything"""
    ids, skeys = rs.span_order(keys)
    rng = np.random.default_rng(seed)
    a, b = np.sort(rng.integers(0, len(skeys), (2, count - 12)), axis=0)
    lo, hi = skeys[a].copy(), skeys[b].copy()
    lo[0::5] += 1                      # a bound in the gap above a key
    hi[1::5] = np.maximum(hi[1::5] - 1, 0)  # ... and below one
    hi[2::7] = NONE
    edge = [(int(skeys[900]), int(skeys[100])), (int(skeys[5]) + 1, int(skeys[5]) + 2), (NONE, NONE), (NONE, 0), (0, 0), (TOP, NONE),
            (TOP, TOP), (0, TOP), (0, NONE), (int(skeys[-2]) + 1, TOP - 1), (1, 6), (int(skeys[40000]), int(skeys[40000]))]
    lo, hi = np.concatenate([lo, [x[0] for x in edge]]), np.concatenate([hi, [x[1] for x in edge]])
    p = rng.permutation(count)
    return spec_of(lo[p], hi[p])


def numpy_counts(keys, spec, members=None):
    ids, skeys = rs.span_order(keys, members)
    return rs.spans_of(skeys, spec["lo"], spec["hi"])[1]


def info_of(keys, members=None):
    """(n, listed, key_min, key_max) as phnsw_attr_info reports them"""
    ids, skeys = rs.span_order(keys, members)
    return N, len(skeys), int(skeys[0]), int(skeys[-1])


ROUTE_SCANS = (0, 1, K - 1, K, 10937, 19999, 20000, 10938)   # rows of the spans that scan: 10 938 = e by the first rule
ROUTE_WALK = 20001


# ---------------------------------------------------------------- 1: the handle
@pytest.mark.parametrize("name", ["all", "some", "flat", "far"])
def test_the_handles_describe_the_columns(name):
    w, keys, h = world("f32", 24), kcol(name), rhandle("ring", "f32", name)
    hix = w["hix"]
    assert h.info() == info_of(keys) and h.listed == {"all": N, "some": N - 100, "flat": N - 100, "far": N}[name]   # numpy
    spec = sample_ranges(keys, 1000, 511)
    counts = counts_of("range", h, spec)
    masks = masks_of("range", rcol(name), spec)
    np.testing.assert_array_equal(counts, numpy_counts(keys, spec))                  # numpy: two binary searches
    np.testing.assert_array_equal(counts, masks.sum(axis=1))                         # the yardstick's masks
    np.testing.assert_array_equal(counts, hix.filter_count(masks))                   # yardstick 2
    assert (counts == 0).sum() >= 5 and (counts == 1).any() and counts.max() == h.listed
    if name in ("all", "flat"):  # the handle made from a device column: the same figures and the same rows
        import torch
        t = torch.from_numpy(keys.astype(np.uint32).view(np.int32)).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        dv = ph.Attribute.from_device(hix, t.data_ptr(), dtype=np.int32)
        assert dv.info() == h.info()
        np.testing.assert_array_equal(counts_of("range", dv, spec), counts)
        sq = take(spec, slice(0, NQX))
        for form, kw, D in forms(w):
            a = host("range", "exact", hix, h, sq, k=K, **kw)
            same(host("range", "exact", hix, dv, sq, k=K, **kw), a)
            same(a, xr.exact_topk(D, masks[:NQX], None, None, K))                    # yardstick 1
        dv.close()


@pytest.mark.parametrize("name", ["all", "flat"])
def test_a_handle_over_every_second_vector(name):
    """vec2node is not the identity: odd ids carry values and are listed nowhere"""
    w, keys, half = world("f32", 24), kcol(name), half_index("f32", 24)
    h = make_handle("range", half, rcol(name))
    assert h.info() == info_of(keys, EVEN) and h.listed <= (N + 1) // 2 and h.listed > 32768
    spec = sample_ranges(keys, NQR, 512)
    masks = masks_of("range", rcol(name), spec)
    counts = counts_of("range", h, spec)
    np.testing.assert_array_equal(counts, numpy_counts(keys, spec, EVEN))            # numpy
    np.testing.assert_array_equal(counts, half.filter_count(masks))                  # yardstick 2
    np.testing.assert_array_equal(counts, (masks & EVEN).sum(axis=1))
    sq = take(spec, slice(0, NQX))
    sq["lo"][0], sq["hi"][0] = 0, NONE  # query 0 is the duplicated row: the even copies tie
    masks = masks_of("range", rcol(name), sq)
    for form, kw, D in forms(w):
        got = host("range", "exact", half, h, sq, k=64, **kw)
        same(got, xr.exact_topk(D, masks, None, EVEN, 64))                           # yardstick 1
        same(got, half.search_exact_filtered(allow=masks, k=64, **kw))               # yardstick 2
        dv = device_call("range", "exact", half, h, sq, k=64, **kw)
        assert not dv[3].any()
        same(dv, got)
        assert not (got[0][got[0] != EMPTY] % 2).any() and got[2][0] == 64
    h.close()


def test_spans_of_one_row_and_of_none():
    """600 queries, each its own span start: in turn the row itself (lo == hi == its key), the gap above its key, its key
    and the next (two rows), lo > hi around it"""
    w, keys, h = gworld("f32"), kcol("some"), rhandle("graph", "f32", "some")
    hix, qids = w["hix"], w["qids"]
    assert not np.isin(qids.astype(np.int64), NONE_ROWS).any()
    ids, skeys = rs.span_order(keys)
    mine = keys[qids.astype(np.int64)]
    rank = np.searchsorted(skeys, mine)
    assert (rank < len(skeys) - 2).all() and len(set(rank.tolist())) == NQR
    turn = np.arange(NQR) % 4
    lo = np.select([turn == 0, turn == 1, turn == 2], [mine, mine + 1, mine], skeys[rank + 1])
    hi = np.select([turn == 0, turn == 1, turn == 2], [mine, mine + 5, skeys[rank + 1]], mine)
    spec = spec_of(lo, hi)
    at, ln = rs.spans_of(skeys, lo, hi)
    assert (ln == np.array([1, 0, 2, 0])[turn]).all() and len(set(at[ln > 0].tolist())) == 300
    order = rs.batch_order(at, ln)
    assert (ln[order[:300]] > 0).all() and not ln[order[300:]].any() and (np.diff(order[:300]) < 0).any()
    masks = masks_of("range", rcol("some"), spec)
    for kw in (dict(queries=w["q"]), dict(qids=qids)):
        dv = device_call("range", "exact", hix, h, spec, k=10, **kw)
        assert not dv[3].any() and (dv[2] == ln.astype(np.uint64)).all()
        same(dv, hix.search_exact_filtered(allow=masks, k=10, **kw))                 # yardstick 2
        same(host("range", "exact", hix, h, spec, k=10, **kw), dv)
    np.testing.assert_array_equal(dv[0][turn == 0, 0], qids[turn == 0])              # a stored query finds its own row
    dv = device_call("range", "exact", hix, h, spec, k=10, qids=qids, exclude=qids)  # its own row taken out
    assert not dv[3].any() and (dv[2] == (ln - (ln > 0)).astype(np.uint64)).all()
    same(dv, hix.search_exact_filtered(qids=qids, allow=masks, exclude=qids, k=10))


# ---------------------------------------------------------------- 2: long spans, whatever the slices
@pytest.mark.parametrize("kind", KINDS)
def test_long_spans_whatever_the_slices(monkeypatch, kind):
    """the plateau (lo == hi, 25 040 rows with one key, the ids ascending), 25 040 rows by distinct keys, all 69 901 rows"""
    flat = int(kcol("flat")[DUPS[0]])
    cases = [(rcol("flat"), rhandle("ring", kind, "flat"), spec_of([flat], [flat]), BIG, N - 100),
             (rcol("some"), rhandle("ring", kind, "some"), rspec("some", [(44000, BIG)]), BIG, N - 100),
             (rcol("some"), rhandle("ring", kind, "some"), spec_of([0], [NONE]), N - 100, N - 100)]
    assert rhandle("ring", kind, "flat").listed == N - 100 == rhandle("ring", kind, "some").listed
    long_spans_body("range", monkeypatch, kind, cases)


# ---------------------------------------------------------------- 3: the second turn of the item loop
def turn_spec():
    """every second query asks for everything, the others for everything from rank 3200 on"""
    return rspec("all", [(0, N) if i % 2 == 0 else (3200, -(N - 3200)) for i in range(NQT)])


def test_the_second_turn_of_the_item_loop(monkeypatch):
    """see the module docstring, gap 1"""
    keys, h = kcol("all"), rhandle("ring", "f32", "all")
    spec = turn_spec()
    ids, skeys = rs.span_order(keys)
    at, ln = rs.spans_of(skeys, spec["lo"], spec["hi"])
    assert h.listed == N and rs.slice_count(5000, h.listed) == FULL and rs.items(NQT, FULL) > rs.GRID_MAX
    assert set(zip(at.tolist(), ln.tolist())) == {(0, N), (3200, N - 3200)}
    order = rs.batch_order(at, ln)
    assert (order != np.arange(NQT)).sum() > 900 and order[:500].tolist() == list(range(0, NQT, 2))   # sorted[] is no identity
    assert len(rs.carrying_blocks(ln[order] > 0, FULL)) == 45424                     # every item is live
    rows = rs.second_turn_rows(order, at, ln, FULL)
    assert rows[0].tolist() == [TURN_ROW, N] and (rows[:, 1] > rows[:, 0]).all()    # every query has second-turn rows
    rank_of_dups = np.searchsorted(skeys, keys[DUPS])
    assert ((rank_of_dups >= rows[0, 0]) & (rank_of_dups < rows[0, 1])).sum() == LATE
    second_turn_body("range", monkeypatch, rcol("all"), h, spec, rank_of_dups)


# ---------------------------------------------------------------- 4: the routed call past 256 queries
def route_one(c):
    return rspec("all", [(30000, c)])


def test_the_routed_call_over_three_blocks_of_queries():
    """scan_below = 0: spans of 20 000 rows scan and spans of 20 001 walk; 10 938 = e rows scan by the first rule although
    the second would let them go"""
    e = first_graph()
    assert e == ROUTE_SCANS[-1] <= BELOW["range"] and ar.rule(e, 100, SP[0], K, N) == ar.GRAPH
    assert [ar.rule(c, BELOW["range"], SP[0], K, N) for c in ROUTE_SCANS + (ROUTE_WALK,)] == [ar.SCAN] * 8 + [ar.GRAPH]
    h = rhandle("graph", "f32", "all")
    scans = join([route_one(ROUTE_SCANS[i % 8]) for i in range(NQR)])
    turn = [ROUTE_WALK, e, 20000, 0, ROUTE_WALK, 19999, 1]
    mixed = join([route_one(turn[i % 7]) for i in range(NQR)])
    walks_at = np.array([turn[i % 7] == ROUTE_WALK for i in range(NQR)])
    assert sorted(set(counts_of("range", h, scans).tolist())) == sorted(ROUTE_SCANS)
    three_blocks_body("range", rcol("all"), h, scans, mixed, walks_at)


@pytest.mark.parametrize("scan_first", [True, False])
def test_a_block_of_scans_next_to_blocks_of_walks(scan_first):
    scans = [route_one(c) for c in (20000, 10938, 0, 19999, 1)]
    scans_next_to_walks_body("range", rcol("all"), rhandle("graph", "f32", "all"), scans, route_one(ROUTE_WALK), scan_first)


def far_spec(want):
    """the range of every wanted label of far_batch: label j + 1 holds the ranks [j * e, (j + 1) * e) of the FAR column,
    label 9 the others, an absent label and NONE an empty range"""
    e = first_graph()
    r = {1: (0, e), 2: (e, e), 3: (2 * e, e), 4: (3 * e, e), 9: (4 * e, N - 4 * e), ABSENT_ROUTE: (5, 0), NONE: (e + 1, 0)}
    return rspec("far", [r[int(x)] for x in want])


@pytest.mark.parametrize("stored", [False, True])
def test_an_explicit_threshold_and_the_rescan_past_256_queries(stored):
    want = far_batch("f32", stored)[1]
    far_body("range", rcol("far"), rhandle("graph", "f32", "far"), far_spec(want), stored)


@pytest.mark.parametrize("kind", ["i8q", "pq"])
def test_the_routed_call_on_the_other_kinds(kind):
    turn = [ROUTE_WALK, 10938, 20000, 0, ROUTE_WALK]
    spec = join([route_one(turn[i % 5]) for i in range(NQR)])
    got = routed_check("range", gworld(kind), rcol("all"), rhandle("graph", kind, "all"), spec, device=True)
    both_routes_in_every_wave(got[3])
    np.testing.assert_array_equal(got[3] == ar.SCAN, np.array([turn[i % 5] != ROUTE_WALK for i in range(NQR)]))


# ---------------------------------------------------------------- 5: the walk by range at N > 65 536
def walk_spec():
    turn = [(30000, ROUTE_WALK), (9, 0), (100, 10938), (0, -N), (65000, 5001), (20, 1)]
    spec = join([rspec("all", [turn[i % 6]]) for i in range(NQR)])
    spec["lo"][5::6], spec["hi"][5::6] = spec["hi"][5::6] + 900000, spec["lo"][5::6] - 900000  # lo > hi with keys between
    return spec, np.isin(np.arange(NQR) % 6, (1, 5))


def test_the_walk_by_range_at_scale():
    spec, empty_at = walk_spec()
    assert (spec["lo"][5::6] > spec["hi"][5::6]).all()
    walk_body("range", rcol("all"), rhandle("graph", "f32", "all"), spec, empty_at)


# ---------------------------------------------------------------- 6: wide queries
def test_wide_queries():
    wide_body("range", rcol("all"), rhandle("graph", "f32", "all"), walk_spec()[0])
