"""Run time on an MI355X: 18 s (26 cases, first clean run, the slowest 2.6 s); run it under `timeout -k 10 54`, three times that.

The label stack (phnsw_labels_*, filter_labeled.hip, label_plan.h, the search kernels' label mode, phnsw_search_labeled_auto)
at the smallest shapes where its loops turn more than once, on the worlds of tests/test_gpu_filter_scale.py: World A,
N = 70 001 rows with 40 copies of row 0 at DUPS, and its built graph.  tests/test_gpu_exact_labeled.py,
test_gpu_labeled_walk.py and test_gpu_labeled_auto.py cover kinds, dimensions, metrics and refusals on 2000 and 5000 rows
with at most 13 labels and 70 queries.  Every comparison here is on ids, distance bits, lengths, status, routes and
stats, no tolerance anywhere.

The six gaps, each with the test that closes it and the shape it asserts (tests/labeled_scale_reference.py restates
label_plan.h's rules, pinned by tests/test_labeled_scale_cpu.py):
  1. the item loop of ph_labeled_scan_kernel / ph_labeled_tile_kernel past the 2^20-block clamp --
     test_the_second_turn_of_the_item_loop: 1000 queries x 1094 slices = 1 094 000 items > 1 048 576, so 45 424 blocks
     take a second item (slices >= 1049 for every position, slice 1048 from position 576 on: list rows >= 67 072).  With
     PHNSW_LABEL_TILE=1 (the scan kernel) every one of them has two live items.  The tile kernel skips items at or past
     its tile count: at the default T = 16 the 1000 queries make 63 tiles, block b meets tile b % 1000 and then tile
     (b + 576) % 1000, and both are live for NO b -- that run turns the loop but carries nothing.  So the tile kernel
     runs a third time at T = 2 (500 tiles): the 3420 blocks with b % 1000 in 424 .. 499 carry their LDS (state[],
     qrow, the flip bit) from a live item into a live item.  All three are asserted from the restated rule.
  2. construction past one sort tile and 2^16 -- test_the_handles_describe_the_lists and test_every_row_its_own_label:
     69 901 labels spread over all four bytes (OWN), one list of 69 901 and one of 70 001 ids (ONE; n % 256 = 113), head[1]
     written at p == n, about 1400 scrambled labels of 1 .. 129 and 25 040 rows (MIX).
  3. lookup and grouping per call -- the same two tests (a lookup among 69 901 values: depth 17) and
     test_many_labels_in_one_batch: 600 (slot, query) pairs, more than 64 tiles at T = 16 with tiles of 1, 15 and 16, another
     cut at T = 3.
  4. a slice that overflows k = 1024 -- test_long_lists_whatever_the_slices: k = 1024 under 1 and 3 slices of 1093 and
     392 batches; every slice sees more than 8000 candidates and evicts.
  5. the routed call by label past 256 queries -- test_the_routed_call_*: 600 queries = 3 trips of ph_auto_route_kernel,
     both routes in every wave of 64; scan_below = 0 parts 20 000 from 20 001 rows.
  6. a wide query matrix -- test_wide_queries: ldq = ld + 8 with NaN behind every row, the three device calls.
test_the_walk_by_label_at_scale runs the search kernels' label mode over label_of[] at N > 65 536.

Yardsticks, named where they are applied: (1) tests/exact_filter_reference.exact_topk over World A's oracle distances
with the masks tests/labeled_reference.masks_of makes of the column, which the code under test never sees (the 65 queries
of world() on f32, i8q and pq); (2) the established bitmap calls on the same masks -- search_exact_filtered for the scan,
search_batch_filtered for the walk, filter_auto_reference.compose / rule / assert_complete over both for the routed call,
filter_count and numpy for Labels.count -- which tests/test_gpu_filter_scale.py pins against the oracle on this very
world; it carries the 600- and 1000-query cases and the f16 / i8 stores.

Not exercised: the 65 536-block clamp of grid1 (n or nq past 16.7 M), the 2^20 clamp of ph_labeled_merge_kernel (more than
1 048 576 queries), the clamp of ph_auto_finish_kernel, nq near PH_LABEL_NQ_MAX, a third turn of the item loop (items past
2^21), and a live tile carried into a NONE-slot tile inside the tile kernel (the scan kernel's second turn has that
order)."""
import functools

import numpy as np
import pytest

import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import filter_auto_reference as ar
import labeled_auto_reference as lar
import labeled_reference as lr
import labeled_scale_reference as ls
import filter_scale_reference as sr
from test_gpu_exact_filter import ring, same
from test_gpu_filter_scale import (DUPS, EVEN, K, N, NQR, NQX, SP, both_routes_in_every_wave, first_graph, gworld, half_index,
                                   rows_a, store_of, stored_ids, world)
from test_gpu_i8 import bits
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

EMPTY, NONE = xr.EMPTY, lr.LABEL_NONE
V_ONE = 0x80000001
TURN_ROW = 67136  # a list of every row: from here on, every position reads its rows in a block's second turn
NQT, FULL = 1000, 1094
SLICES = (None, "1", "2", "3", "7", "391", "392", "1093", "5000")
COMBOS = [(s, None) for s in SLICES] + [(s, t) for t in ("1", "3") for s in ("1", "3")]  # (PHNSW_LABEL_SLICES, _TILE)
ORACLE_KINDS = ("f32", "i8q", "pq")

# the shapes the module is about, on the CPU at collection
assert ls.batches(N) == FULL and ls.last_batch_ids(N) == 49 and ls.batches(N - 100) == 1093 and N % 256 == 113
assert 959 * FULL > ls.GRID_MAX >= 958 * FULL and ls.items(NQT, FULL) > 2 ** 20 >= ls.items(958, FULL)
_past = ls.past_clamp(NQT, FULL)
assert _past[1049:].all() and not _past[:1048].any() and not _past[1048, :576].any() and _past[1048, 576:].all()
assert ls.second_turn_first_row(NQT, FULL, N) == (TURN_ROW - 64, TURN_ROW)
assert len(ls.both_turns(NQT, FULL, NQT)) == 45424 and len(ls.both_turns(NQT, FULL, 63)) == 0
assert len(ls.both_turns(NQT, FULL, 500)) == 3420
NONE_ROWS = ls.none_rows(N, 100, np.concatenate([DUPS, stored_ids(N, DUPS, NQX).astype(np.int64)]), TURN_ROW, 401)
assert len(NONE_ROWS) == 100 and NONE_ROWS.max() < TURN_ROW and not np.isin(NONE_ROWS, DUPS).any()


# ---------------------------------------------------------------- columns, worlds, handles
@functools.lru_cache(maxsize=None)
def mix():
    """(MIX, its info): BIG on all 40 DUPS and 25 000 other rows"""
    lab, info = ls.column_mix(N, DUPS, 25000, NONE_ROWS, 402)
    assert info["sizes"][info["big"]] == 25040 and ls.batches(25040) == 392 and (lab[DUPS] == info["big"]).all()
    assert ls.info_of(lab, N)[1] == len(info["sizes"]) > 1200 and (lab == NONE).sum() == 100
    lab.setflags(write=False)
    return lab, info


def route_sizes():
    e = first_graph()
    assert e == 10938
    return [1, K - 1, K, lar.SCAN_BELOW_LABELED - 1, lar.SCAN_BELOW_LABELED, e - 1], [lar.SCAN_BELOW_LABELED + 1, e, lar.SCAN_BELOW_LABELED]


@functools.lru_cache(maxsize=None)
def col(name):
    """the label of every row, i64 [N], constructed; each asserts its own counts"""
    if name == "mix":
        return mix()[0]
    if name == "one":    # one list of 69 901 ids; the 100 unlabelled rows are no DUPS, below TURN_ROW
        lab = ls.column_one(N, V_ONE, NONE_ROWS)
        assert ls.info_of(lab, N) == (N, 1, 69901, 69901) and (lab[DUPS] == V_ONE).all() and (lab[TURN_ROW:] == V_ONE).all()
    elif name == "all":  # no unlabelled row: NONE starts nowhere in the sorted keys, head[1] is written at p == n
        lab = ls.column_one(N, V_ONE)
        assert ls.info_of(lab, N) == (N, 1, N, N)
    elif name == "own":
        lab = ls.column_own(N, NONE_ROWS)
        assert ls.info_of(lab, N) == (N, 69901, 69901, 1) and 69901 > 65536
        listed = lab[lab != NONE]
        assert all(len(np.unique((listed >> s) & 0xFF)) == 256 for s in (0, 8, 16, 24))
    elif name in ("route1", "route2"):  # a column is a partition: the rule's edges need two
        sizes = route_sizes()[name == "route2"]
        lab = ls.sized_column(N, sizes, 403 + (name == "route2"), first=1 if name == "route1" else 11)
        assert sorted(np.unique(lab[lab != NONE], return_counts=True)[1].tolist()) == sorted(sizes)
    lab.setflags(write=False)
    return lab


ABSENT_ROUTE = 77  # in neither route column


@functools.lru_cache(maxsize=None)
def lworld(kind):
    """World A over the store of `kind` at 24: world()'s for the kinds that have the oracle's distances, else (f16, i8)
    a ring index and the f32 world's queries, for yardstick 2 alone"""
    if kind in ORACLE_KINDS:
        return world(kind, 24)
    base, store = world("f32", 24), store_of(kind, 24)
    return dict(store=store, hix=ph.Hnsw.from_layers(store, ring(np.arange(N))), q=base["q"], qids=base["qids"], Dq=None, Ds=None)


@functools.lru_cache(maxsize=None)
def handle(kind, name):
    return ph.Labels(lworld(kind)["hix"], col(name))


@functools.lru_cache(maxsize=None)
def ghandle(kind, name):
    return ph.Labels(gworld(kind)["hix"], col(name) if isinstance(name, str) else far_column(kind)[0])


def forms(w):
    """(form, keyword arguments, the oracle's distances or None) for raw and stored queries"""
    return [(0, dict(queries=w["q"]), w["Dq"]), (1, dict(qids=w["qids"]), w["Ds"])]


def cut(res, k):
    """the first k columns of rows computed at a larger k"""
    return res[0][:, :k], res[1][:, :k], np.minimum(res[2], np.uint64(k))


def without(res, exclude, k):
    """rows at k of rows computed at k0 > k with exclude[q] taken out: the candidates but one, in the same order (every
    row here holds at least k + 1 entries or the whole list)"""
    ids, d, ln = (np.full((len(res[2]), k), EMPTY, dtype=np.uint64), np.full((len(res[2]), k), xr.FMAX, dtype=np.float32),
                  np.zeros(len(res[2]), dtype=np.uint64))
    for q in range(len(ln)):
        m = int(res[2][q])
        keep = res[0][q, :m] != np.uint64(int(exclude[q]))
        assert keep.sum() >= min(k, m - 1)
        i, x = res[0][q, :m][keep][:k], res[1][q, :m][keep][:k]
        ids[q, :len(i)], d[q, :len(i)], ln[q] = i, x, len(i)
    return ids, d, ln


def padded(got, k):
    pad = np.arange(k)[None, :] >= got[2][:, None]
    assert (got[0][pad] == EMPTY).all() and (bits(got[1])[pad] == bits(xr.FMAX)).all()


def knobs(slices=None, tile=None):
    kv = {}
    if slices is not None:
        kv["PHNSW_LABEL_SLICES"] = str(slices)
    if tile is not None:
        kv["PHNSW_LABEL_TILE"] = str(tile)
    return kv


def device_call(which, hix, lb, k=K, sp=None, queries=None, qids=None, want=None, exclude=None, strict=False, scan_below=0,
                stream=None, wide=0):
    """phnsw_search_exact_labeled_device ("exact"), phnsw_search_batch_labeled_device ("walk") or
    phnsw_search_labeled_auto_device ("auto") with torch buffers; 64 guard words behind every output must come back as
    they went in.  wide: ldq = ld + wide, the columns past ld filled with NaN (those from dim to ld are zero).
    -> ids u64, d, len u64, then status ("exact"); stats, status ("walk"); route, status ("auto")"""
    import torch
    dev = torch.device("cuda", 0)
    keep = []

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t.data_ptr()

    nq = len(queries) if queries is not None else len(qids)
    width = sp.number_of_candidates if which == "walk" else k
    qd = qi = ex = ldq = 0
    if queries is not None:
        ld = hix.store.ld
        ldq = ld + wide
        qp = np.full((nq, ldq), np.nan, dtype=np.float32)
        qp[:, :ld] = 0.0
        qp[:, :queries.shape[1]] = queries
        qd = up(qp)
    else:
        qi = up(np.asarray(qids, dtype=np.uint32).view(np.int32))
    if exclude is not None:
        e = np.asarray(exclude, dtype=np.uint64).copy()
        e[e > 0xFFFFFFFF] = 0xFFFFFFFF
        ex = up(e.astype(np.uint32).view(np.int32))
    wd = up(ph.hnsw.pack_labels(want, nq, "want").view(np.int32))
    G = 64
    ids = torch.full((nq * width + G,), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq * width + G,), -1.0, dtype=torch.float32, device=dev)
    ln, status, route = (torch.full((nq + G,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    st = torch.full((2 * nq + G,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    s = 0 if stream is None else stream.cuda_stream
    if which == "exact":
        hix.search_exact_labeled_device(lb, nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd,
                                        ldq=ldq, qids=qi, exclude=ex, want=wd, stream=s)
    elif which == "walk":
        hix.search_batch_labeled_device(lb, nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd,
                                        ldq=ldq, qids=qi, exclude=ex, want=wd, strict=strict, out_stats=st.data_ptr(), stream=s)
    else:
        hix.search_labeled_device(lb, nq, sp, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd,
                                  ldq=ldq, qids=qi, exclude=ex, want=wd, scan_below=scan_below, out_route=route.data_ptr(),
                                  stream=s)
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


def sample_wants(lab, count, seed, extra=()):
    """`count` wanted labels: present values in a random order, then what a lookup must miss -- below the smallest value,
    above the largest (where u32 has room), between two present values, NONE and -1 -- and `extra`"""
    values = np.unique(lab[lab != NONE])
    miss = [int(values[0]) - 1] if values[0] > 0 else []
    if values[-1] + 1 < NONE:
        miss.append(int(values[-1]) + 1)
    gaps = np.nonzero(np.diff(values) > 1)[0]
    miss += [int(values[g]) + 1 for g in gaps[:: max(1, len(gaps) // 8)][:8]]
    miss += [NONE, -1] + list(extra)
    rng = np.random.default_rng(seed)
    present = values[rng.permutation(len(values))[:count - len(miss)]]
    if len(present) < count - len(miss):
        present = np.resize(present, count - len(miss))
    want = np.concatenate([present, np.array(miss, dtype=np.int64)])[rng.permutation(count)]
    assert len(want) == count and (ls.counts_of(lab, want) == 0).sum() >= len(miss) - len(extra)
    return want


# ---------------------------------------------------------------- 1: the handle
@pytest.mark.parametrize("name", ["one", "all", "own", "mix", "route1", "route2"])
def test_the_handles_describe_the_lists(name):
    w, lab, lb = world("f32", 24), col(name), handle("f32", name)
    hix = w["hix"]
    assert lb.info() == ls.info_of(lab, N)                                    # numpy
    extra = (mix()[1]["between"], mix()[1]["below"], mix()[1]["top"]) if name == "mix" else ()
    want = sample_wants(lab, NQR, 411, extra)
    counts = lb.count(want)
    np.testing.assert_array_equal(counts, ls.counts_of(lab, want))            # numpy
    np.testing.assert_array_equal(counts, hix.filter_count(lr.masks_of(lab, want)))  # yardstick 2
    assert (counts == 0).any() and (counts > 0).any()
    if name in ("own", "mix", "all"):  # the handle made from a device column: the same figures and the same rows
        import torch
        t = torch.from_numpy(ph.hnsw.pack_labels(lab, N, "labels").view(np.int32)).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        dv = ph.Labels.from_device(hix, t.data_ptr())
        assert dv.info() == lb.info()
        np.testing.assert_array_equal(dv.count(want), counts)
        for form, kw, D in forms(w):
            wq = want[:NQX]
            a = hix.search_exact_labeled(labels=lb, want=wq, k=K, **kw)
            same(hix.search_exact_labeled(labels=dv, want=wq, k=K, **kw), a)
            same(a, xr.exact_topk(D, lr.masks_of(lab, wq), None, None, K))    # yardstick 1
        dv.close()


@pytest.mark.parametrize("name", ["mix", "all"])
def test_a_handle_over_every_second_vector(name):
    """vec2node is not the identity: odd ids carry labels and are listed nowhere"""
    w, lab, half = world("f32", 24), col(name), half_index("f32", 24)
    lb = ph.Labels(half, lab)
    assert lb.info() == ls.info_of(lab, N, EVEN) and lb.listed <= (N + 1) // 2
    want = sample_wants(lab, NQR, 412)
    masks = lr.masks_of(lab, want)
    np.testing.assert_array_equal(lb.count(want), ls.counts_of(lab, want, EVEN))      # numpy
    np.testing.assert_array_equal(lb.count(want), half.filter_count(masks))           # yardstick 2
    np.testing.assert_array_equal(lb.count(want), (masks & EVEN).sum(axis=1))
    wq = want[:NQX].copy()
    wq[0] = lab[0]  # query 0 is the duplicated row: the even copies tie
    masks = lr.masks_of(lab, wq)
    for form, kw, D in forms(w):
        got = half.search_exact_labeled(labels=lb, want=wq, k=64, **kw)
        same(got, xr.exact_topk(D, masks, None, EVEN, 64))                            # yardstick 1
        same(got, half.search_exact_filtered(allow=masks, k=64, **kw))                # yardstick 2
        dv = device_call("exact", half, lb, k=64, want=wq, **kw)
        assert not dv[3].any()
        same(dv, got)
        assert not (got[0][got[0] != EMPTY] % 2).any() and got[2][0] == min(64, (masks[0] & EVEN).sum())
    lb.close()


def test_every_row_its_own_label():
    """OWN: 69 901 lists of one id.  A stored query that wants its own row's label gets exactly that row"""
    w, lab, lb = world("f32", 24), col("own"), handle("f32", "own")
    hix, qids = w["hix"], w["qids"]
    assert not np.isin(qids.astype(np.int64), NONE_ROWS).any()
    want = lab[qids.astype(np.int64)]
    assert ls.slots_of(np.unique(lab[lab != NONE]), want).max() < 69901
    dv = device_call("exact", hix, lb, k=10, qids=qids, want=want)
    assert not dv[3].any() and (dv[2] == 1).all() and (dv[0][:, 0] == qids).all() and (dv[0][:, 1:] == EMPTY).all()
    same(dv, xr.exact_topk(w["Ds"], lr.masks_of(lab, want), None, None, 10))                  # yardstick 1
    same(dv, hix.search_exact_filtered(qids=qids, allow=lr.masks_of(lab, want), k=10))        # yardstick 2
    dv = device_call("exact", hix, lb, k=10, qids=qids, want=want, exclude=qids)
    assert not dv[3].any() and not dv[2].any() and (dv[0] == EMPTY).all() and (bits(dv[1]) == bits(xr.FMAX)).all()
    gone = ls.own_label(NONE_ROWS[:NQX])  # the label an unlabelled row would carry: listed nowhere
    assert not ls.counts_of(lab, gone).any()
    for got in (device_call("exact", hix, lb, k=10, queries=w["q"], want=gone),
                hix.search_exact_labeled(queries=w["q"], labels=lb, want=gone, k=10)):
        assert not got[2].any() and (got[0] == EMPTY).all()


# ---------------------------------------------------------------- 2: long lists, whatever the slices
def long_lists():
    return {"ONE": ("one", V_ONE, 69901), "BIG": ("mix", mix()[1]["big"], 25040)}


@pytest.mark.parametrize("kind", ["f32", "i8q", "pq", "f16", "i8"])
def test_long_lists_whatever_the_slices(monkeypatch, kind):
    w = lworld(kind)
    hix = w["hix"]
    for name, (cname, value, length) in long_lists().items():
        lab, lb = col(cname), handle(kind, cname)
        allow = lab == value
        assert allow.sum() == length == lb.count([value])[0] and allow[DUPS].all()
        assert ls.slice_count(5000, lb.longest) == ls.batches(length) == {"ONE": 1093, "BIG": 392}[name]
        assert min(b - a for a, b in ls.slice_ranges(length, 3)) * ls.BATCH > 8 * ls.KMAX  # a slice overflows k = 1024
        outside = int(NONE_ROWS[5]) if name == "ONE" else int(np.nonzero(~allow & (lab != NONE))[0][7])
        for form, kw, D in forms(w):
            nq = len(next(iter(kw.values())))
            want = np.full(nq, value, dtype=np.int64)
            y1 = None if D is None else xr.exact_topk(D, allow, None, None, 1024)
            base = {}
            for k in (1, 10, 64):
                y2 = hix.search_exact_filtered(allow=allow, k=k, **kw)
                for slices, tile in COMBOS:
                    with env(monkeypatch, **knobs(slices, tile)):
                        got = hix.search_exact_labeled(labels=lb, want=want, k=k, **kw)
                        dv = device_call("exact", hix, lb, k=k, want=want, **kw) if k == 10 and tile is None and slices in (None, "3") else None
                    padded(got, k)
                    if slices is None and tile is None:
                        base[k] = got
                        same(got, y2)                      # yardstick 2
                        if y1 is not None:
                            same(got, cut(y1, k))          # yardstick 1
                    else:
                        same(got, base[k])                 # rows do not depend on the slice count or on T
                    if dv is not None:
                        assert not dv[3].any()
                        same(dv, base[k])
            # k = 1024: every slice holds more than 1024 candidates and evicts
            y2 = hix.search_exact_filtered(allow=allow, k=1024, **kw)
            for slices, tile in (("1", None), ("3", None), ("1", "1"), ("3", "1")):
                with env(monkeypatch, **knobs(slices, tile)):
                    got = hix.search_exact_labeled(labels=lb, want=want, k=1024, **kw)
                same(got, y2)                              # yardstick 2
                if y1 is not None:
                    same(got, y1)                          # yardstick 1
                assert (got[2] == 1024).all()
                if kind not in ("i8q", "pq"):  # normalised rows: nothing is nearer to a row than its copies
                    np.testing.assert_array_equal(got[0][0, :40], DUPS.astype(np.uint64))
                    assert len(set(bits(got[1][0, :40]).tolist())) == 1
            # exclude, in turn: the query's best hit, an id outside the list, an id past n, EMPTY
            best = base[10][0][:, 0]
            ex = np.array([(int(best[i]), outside, N + 7, EMPTY)[i % 4] for i in range(nq)], dtype=np.uint64)
            y2 = hix.search_exact_filtered(allow=allow, exclude=ex, k=10, **kw)
            for slices in (None, "3"):
                with env(monkeypatch, **knobs(slices)):
                    got = hix.search_exact_labeled(labels=lb, want=want, exclude=ex, k=10, **kw)
                    dv = device_call("exact", hix, lb, k=10, want=want, exclude=ex, **kw)
                same(got, y2)                              # yardstick 2
                if y1 is not None:
                    same(got, without(y1, ex, 10))         # yardstick 1
                assert not dv[3].any()
                same(dv, got)
                assert not (got[0][0::4] == best[0::4, None]).any()
                same(tuple(x[1::4] for x in got), tuple(x[1::4] for x in base[10]))  # an id outside the list changes nothing


# ---------------------------------------------------------------- 3: the second turn of the item loop
def turn_queries():
    """1000 stored ids: world()'s 65 first; at positions 570 .. 674, 105 ids from TURN_ROW on, two or three in each of
    slices 1049 .. 1093 of a list that holds every row; an even spread elsewhere"""
    late = np.array([s * 64 + o for s in range(1049, FULL) for o in (5, 40)] + [s * 64 + 20 for s in range(1049, 1064)], dtype=np.int64)
    assert len(late) == 105 and late.min() >= TURN_ROW and late.max() < N and not np.isin(late, DUPS).any()
    assert set((late // ls.BATCH).tolist()) == set(range(1049, FULL))
    rest = np.linspace(3, N - 3, NQT - NQX - len(late)).astype(np.int64)
    qids = np.concatenate([stored_ids(N, DUPS, NQX).astype(np.int64), rest[:505], late, rest[505:]]).astype(np.uint64)
    at = np.arange(570, 675)
    assert len(qids) == NQT and (qids[at] == late.astype(np.uint64)).all() and {575, 576, 577} <= set(at.tolist())
    return qids, at


def test_the_second_turn_of_the_item_loop(monkeypatch):
    """see the module docstring, gap 1.  Sensitivity, checked once on a copy of filter_labeled.hip and not kept: with
    state[4t], state[4t + 1] reset only while the block has had no live item yet, the T = 1 and T = 16 runs pass and the
    first T = 2 run fails (250 of 10 000 ids differ from yardstick 2) -- the T = 2 run is what reads the carried LDS.  The
    `__syncthreads()` at the top of the item loop separates nothing in a block of one wave64, so dropping it cannot be
    shown to fail and was not tried"""
    import torch
    w, lab, lb = world("f32", 24), col("all"), handle("f32", "all")
    hix = w["hix"]
    qids, at = turn_queries()
    assert (qids[:NQX] == w["qids"]).all()
    raw = np.concatenate([w["q"], rows_a(False, 24)[qids[NQX:].astype(np.int64)]])
    T = ls.tile_of(K, hix.store.ld)
    assert lb.longest == N and ls.slice_count(FULL, lb.longest) == FULL and ls.items(NQT, FULL) > 2 ** 20
    assert T == 16 and len(ls.tiles([0] * NQT, T)) == 63 and ls.tile_of(K, hix.store.ld, 2) == 2
    ones = np.ones(N, dtype=bool)
    want = np.full(NQT, V_ONE, dtype=np.int64)
    np.testing.assert_array_equal(lr.masks_of(lab, want[:1])[0], ones)
    y2 = {0: hix.search_exact_filtered(queries=raw, allow=ones, k=K), 1: hix.search_exact_filtered(qids=qids, allow=ones, k=K)}
    y1 = {0: xr.exact_topk(w["Dq"], None, None, None, K), 1: xr.exact_topk(w["Ds"], None, None, None, K)}
    stream = torch.cuda.Stream()
    runs = {}
    for tile in ("1", None, "2"):  # the scan kernel; the tile kernel at T = 16 (no block with two live items) and at T = 2
        for form, kw in ((1, dict(qids=qids)), (0, dict(queries=raw))):
            with env(monkeypatch, **knobs(FULL, tile)):
                dv = device_call("exact", hix, lb, k=K, want=want, stream=stream, **kw)
            assert not dv[3].any()
            same(dv, y2[form])                                        # yardstick 2, all 1000
            same(tuple(x[:NQX] for x in dv), y1[form])                # yardstick 1, the first 65
            runs[tile, form] = dv
        np.testing.assert_array_equal(runs[tile, 1][0][at, 0], qids[at])  # its own row first, read in a second turn
    with env(monkeypatch, **knobs(FULL, "1")):
        same(hix.search_exact_labeled(qids=qids, labels=lb, want=want, k=K), y2[1])   # the host form, once
    # 300 queries want the label and 700 an absent one, interleaved: the NONE-slot positions sort last and write empty rows
    some = np.isin(np.arange(NQT) % 10, (0, 3, 7))
    want2 = np.where(some, V_ONE, 5).astype(np.int64)
    sslot, order = ls.sorted_slots(ls.slots_of([V_ONE], want2))
    assert some.sum() == 300 and (sslot[300:] == ls.SLOT_NONE).all() and not sslot[:300].any() and some[order[:300]].all()
    assert [len(ls.tiles(sslot, t)) for t in (16, 2)] == [19 + 44, 500]
    expect = tuple(x.copy() for x in y2[1])
    expect[0][~some], expect[1][~some], expect[2][~some] = EMPTY, xr.FMAX, 0
    for tile in ("1", None, "2"):
        with env(monkeypatch, **knobs(FULL, tile)):
            dv = device_call("exact", hix, lb, k=K, qids=qids, want=want2, stream=stream)
        assert not dv[3].any() and not dv[2][~some].any()
        same(dv, expect)                                              # yardstick 2
    # 958 queries: 958 * 1094 <= 2^20, the grid is not clamped -- the same rows
    assert ls.items(958, FULL) <= 2 ** 20 and len(ls.both_turns(958, FULL, 958)) == 0
    for tile in ("1", None):
        with env(monkeypatch, **knobs(FULL, tile)):
            dv = device_call("exact", hix, lb, k=K, qids=qids[:958], want=want[:958], stream=stream)
        same(dv, tuple(x[:958] for x in runs[tile, 1][:3]))


# ---------------------------------------------------------------- 4: many labels in one batch
@functools.lru_cache(maxsize=None)
def batch_wants():
    """600 wanted labels over MIX: groups of 15, 16, 17, 33 and 100 queries of one label, 151 labels wanted once (one of
    them the group of 1), 40 absent labels or NONE, BIG for the rest; spread over the batch"""
    lab, info = mix()
    sizes = info["sizes"]
    pool = [v for v in sizes if v != info["big"]]
    groups = list(zip(pool[:5], (15, 16, 17, 33, 100))) + [(v, 1) for v in pool[5:156]]
    miss = [info["between"], info["below"], NONE, -1, info["adjacent"][1] + 1, 0]
    groups += [(miss[i % len(miss)], 1) for i in range(40)]
    want = ls.spread_groups(NQR, groups, info["big"], 421)
    assert not ls.counts_of(lab, miss).any() and (ls.counts_of(lab, want) == 0).sum() == 40
    assert (want == info["big"]).sum() == NQR - 181 - 151 - 40
    return want


def test_many_labels_in_one_batch(monkeypatch):
    lab, info = mix()
    w, lb = gworld("f32"), ghandle("f32", "mix")
    hix = w["hix"]
    want = batch_wants()
    values = np.unique(lab[lab != NONE])
    sslot, order = ls.sorted_slots(ls.slots_of(values, want))
    T = ls.tile_of(K, hix.store.ld)
    cut16, cut3 = ls.tiles(sslot, T), ls.tiles(sslot, 3)
    assert T == 16 and len(cut16) > 64 and {1, 15, 16} <= {c for _, c in cut16} and cut16 != cut3 and len(cut3) > len(cut16)
    g100 = [v for v in info["sizes"] if v != info["big"]][4]
    assert (want == g100).sum() == 100 and (np.diff(np.nonzero(want == g100)[0]) > 1).sum() > 50  # spread, not adjacent
    masks = lr.masks_of(lab, want)
    base = {}
    for form, kw in ((0, dict(queries=w["q"])), (1, dict(qids=w["qids"]))):
        y2 = hix.search_exact_filtered(allow=masks, k=K, **kw)
        for tile in (None, "1", "3"):
            for slices in (None, "1", "3"):
                with env(monkeypatch, **knobs(slices, tile)):
                    got = hix.search_exact_labeled(labels=lb, want=want, k=K, **kw)
                same(got, y2)                                         # yardstick 2
        base[form] = y2
    bad = [7, 300, 599]  # on the device form, three stored ids past n: status 4, an empty row, nobody else harmed
    qids = w["qids"].copy()
    qids[bad] = [N, N + 12345, 0xFFFFFFFE]
    good = np.setdiff1d(np.arange(NQR), bad)
    for tile, slices in ((None, None), ("1", None), ("3", "3"), (None, "3")):
        with env(monkeypatch, **knobs(slices, tile)):
            dv = device_call("exact", hix, lb, k=K, qids=qids, want=want)
        same(tuple(x[good] for x in dv[:3]), tuple(x[good] for x in base[1]))   # yardstick 2
        assert (dv[3][bad] == 4).all() and not dv[3][good].any()
        assert (dv[0][bad] == EMPTY).all() and (bits(dv[1][bad]) == bits(xr.FMAX)).all() and not dv[2][bad].any()


# ---------------------------------------------------------------- 5: the routed call past 256 queries
BELOW = lar.SCAN_BELOW_LABELED


def routed_check(w, lab, lb, want, scan_below=0, exclude=None, stored=False, device=False, q=None, qids=None):
    """the host form (and the device form on a side stream) against ROWS, ROUTES and COMPLETE as
    tests/test_gpu_labeled_auto.py names them, with compose over the two bitmap calls (yardstick 2); scan_below = 0:
    the library's 20 000 decides.  Returns the host result."""
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    kw = dict(qids=w["qids"] if qids is None else qids) if stored else dict(queries=w["q"] if q is None else q)
    below = scan_below or BELOW
    masks = lr.masks_of(lab, want)
    got = hix.search_labeled(sp=spp, labels=lb, want=want, exclude=exclude, k=K, scan_below=scan_below, route=True, **kw)
    walk = hix.search_batch_filtered(sp=spp, allow=masks, strict=True, exclude=exclude, **kw)
    scan = hix.search_exact_filtered(allow=masks, exclude=exclude, k=K, **kw)
    ref = ar.compose(walk, scan, N, SP[0], K, N, masks, exclude, None, below)
    print("routes", np.bincount(got[3], minlength=3).tolist(), "expected", np.bincount(ref[3], minlength=3).tolist())
    np.testing.assert_array_equal(got[3], ref[3])      # ROWS: which graph rows the strict bitmap call leaves short
    same(got, ref)                                      # ROWS
    counts = lb.count(want)
    np.testing.assert_array_equal(counts, masks.sum(axis=1))
    for i in range(NQR):                                # ROUTES
        r = ar.rule(counts[i], below, SP[0], K, N)
        assert got[3][i] == r or (got[3][i] == ar.GRAPH_THEN_SCAN and r == ar.GRAPH), (i, got[3][i], r)
    ar.assert_complete(got, N, K, masks, exclude, None)  # COMPLETE
    if device:
        import torch
        dv = device_call("auto", hix, lb, k=K, sp=spp, want=want, exclude=exclude, scan_below=scan_below,
                         stream=torch.cuda.Stream(), **kw)
        assert not dv[4].any()
        same(dv, got)
        np.testing.assert_array_equal(dv[3], got[3])
    return got


def cycle(values, nq=NQR):
    return np.array([values[i % len(values)] for i in range(nq)], dtype=np.int64)


def nearest_exclude(w, lb, want, **kw):
    return w["hix"].search_exact_labeled(labels=lb, want=want, k=1, **kw)[0][:, 0].copy()


def test_the_routed_call_over_three_blocks_of_queries():
    """scan_below = 0: lists of 20 000 rows scan and lists of 20 001 walk; 10 938 = e rows scan by the first rule although
    the second would let them go"""
    w = gworld("f32")
    e = first_graph()
    assert sr.trips(NQR, sr.ROUTE_QUERIES) == 3 and e - 1 < e <= BELOW and ar.rule(e, 100, SP[0], K, N) == ar.GRAPH
    # every list the first column has scans: 0 (absent, NONE), 1, K - 1, K, 19 999, 20 000, e - 1 rows
    lab, lb = col("route1"), ghandle("f32", "route1")
    want = cycle([ABSENT_ROUTE, NONE, 1, 2, 3, 4, 5, 6])
    assert sorted(set(lb.count(want).tolist())) == [0, 1, K - 1, K, e - 1, BELOW - 1, BELOW]
    got = routed_check(w, lab, lb, want, device=True)
    assert (got[3] == ar.SCAN).all()
    # 20 001, e and 20 000 rows, an absent label and NONE in turn: both routes in every wave of every block of 256
    lab, lb = col("route2"), ghandle("f32", "route2")
    want = cycle([11, 12, 13, ABSENT_ROUTE, NONE])
    assert sorted(set(lb.count(want).tolist())) == [0, e, BELOW, BELOW + 1]
    for stored in (False, True):
        got = routed_check(w, lab, lb, want, stored=stored, device=not stored)
        np.testing.assert_array_equal(got[3] == ar.SCAN, want != 11)
        both_routes_in_every_wave(got[3])
    ex = nearest_exclude(w, lb, want, queries=w["q"])   # exclude: each query's nearest candidate, EMPTY where none
    got = routed_check(w, lab, lb, want, exclude=ex, device=True)
    assert not ((got[0] == ex[:, None]) & (ex[:, None] != EMPTY)).any() and (ex == EMPTY).sum() == 2 * NQR // 5


@pytest.mark.parametrize("scan_first", [True, False])
def test_a_block_of_scans_next_to_blocks_of_walks(scan_first):
    w, lab, lb = gworld("f32"), col("route2"), ghandle("f32", "route2")
    scans, walks = cycle([12, 13, ABSENT_ROUTE, NONE], sr.ROUTE_QUERIES), cycle([11], NQR - sr.ROUTE_QUERIES)
    if not scan_first:
        scans, walks = cycle([12, 13, ABSENT_ROUTE, NONE], NQR - sr.ROUTE_QUERIES), cycle([11], sr.ROUTE_QUERIES)
    want = np.concatenate([scans, walks] if scan_first else [walks, scans])
    got = routed_check(w, lab, lb, want, stored=not scan_first, device=scan_first)
    np.testing.assert_array_equal(got[3] == ar.SCAN, want != 11)
    head = got[3][:sr.ROUTE_QUERIES] == ar.SCAN
    assert head.all() == scan_first and head.any() == scan_first


FAR_US = (300, 301, 302, 303)  # the raw queries of gworld whose far rows get a label each


@functools.lru_cache(maxsize=None)
def far_column(kind="f32"):
    """(FAR, nearest): label j + 1 on the e rows FARTHEST (smallest cosine; numpy on the rows, as test_gpu_filter_scale's
    cycled_bitmaps) from raw query FAR_US[j] among the rows no earlier j took, label 9 on the rest; nearest[j] = the
    stored row nearest that query"""
    w, e = gworld(kind), first_graph()
    rows = rows_a(kind == "i8q", 24).astype(np.float64)
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    lab = np.full(N, 9, dtype=np.int64)
    nearest = []
    for j, qi in enumerate(FAR_US):
        v = w["q"][qi].astype(np.float64)
        cos = unit @ (v / np.linalg.norm(v))
        free = np.nonzero(lab == 9)[0]
        lab[free[np.argsort(-cos[free], kind="stable")[len(free) - e:]]] = j + 1
        nearest.append(int(np.argmax(cos)))
    assert [(lab == j + 1).sum() for j in range(4)] == [e] * 4 and (lab == 9).sum() == N - 4 * e > e
    lab.setflags(write=False)
    return lab, nearest


def far_batch(kind, stored):
    """wants cycling through the FAR labels, label 9, an absent one and NONE; past the first 256 queries, at 20 places,
    copies of the raw query FAR_US[j] (stored form: the row nearest it) wanting label j + 1"""
    w = gworld(kind)
    lab, nearest = far_column(kind)
    want = cycle([9, 1, ABSENT_ROUTE, 2, NONE, 3, 9, 4])
    q, qids = w["q"].copy(), w["qids"].copy()
    places = []
    for j, qi in enumerate(FAR_US):
        for p in (256 + j, 317 + 9 * j, 511 + j, 520 + 11 * j, 596 + j):
            q[p], qids[p], want[p] = w["q"][qi], nearest[j], j + 1
            places.append(p)
    assert min(places) >= sr.ROUTE_QUERIES and len(set(places)) == 20
    return lab, want, q, qids, np.array(places)


@pytest.mark.parametrize("stored", [False, True])
def test_an_explicit_threshold_and_the_rescan_past_256_queries(stored):
    """scan_below = 100, so e = 10 938 decides.  Reached on this graph: a query that wants the e rows farthest from
    itself (raw), or from the raw query it is the nearest row of (stored), walks towards rows it may not return, comes
    back short of k and is scanned again (GRAPH_THEN_SCAN) -- with one direction per label, four labels, each wanted by
    five queries past the first 256.  The precondition is asserted on the established strict bitmap call"""
    w = gworld("f32")
    lab, want, q, qids, places = far_batch("f32", stored)
    lb = ghandle("f32", ("far",))
    e = first_graph()
    assert ar.rule(e, 100, SP[0], K, N) == ar.GRAPH and ar.rule(e - 1, 100, SP[0], K, N) == ar.SCAN
    kw = dict(qids=qids) if stored else dict(queries=q)
    strict = w["hix"].search_batch_filtered(sp=ph.SearchParameters(*SP), allow=lr.masks_of(lab, want), strict=True, **kw)
    print("strict bitmap rows shorter than k at the far places:", (strict[2][places] < K).sum(), "of", len(places))
    assert (strict[2][places] < K).any()  # the precondition, on the established call
    got = routed_check(w, lab, lb, want, scan_below=100, stored=stored, device=True, q=q, qids=qids)
    assert (got[3][places] == ar.GRAPH_THEN_SCAN).any() and (got[3] == ar.GRAPH).any() and (got[3] == ar.SCAN).any()
    assert (got[3][places] != ar.SCAN).all()
    ex = nearest_exclude(w, lb, want, **kw)
    got = routed_check(w, lab, lb, want, scan_below=100, exclude=ex, stored=stored, q=q, qids=qids)
    assert not ((got[0] == ex[:, None]) & (ex[:, None] != EMPTY)).any()
    assert (got[3][places] == ar.GRAPH_THEN_SCAN).any()


@pytest.mark.parametrize("kind", ["i8q", "pq"])
def test_the_routed_call_on_the_other_kinds(kind):
    w, lab, lb = gworld(kind), col("route2"), ghandle(kind, "route2")
    want = cycle([11, 12, 13, ABSENT_ROUTE, NONE])
    got = routed_check(w, lab, lb, want, device=True)
    both_routes_in_every_wave(got[3])
    np.testing.assert_array_equal(got[3] == ar.SCAN, want != 11)


# ---------------------------------------------------------------- 6: the walk by label at N > 65 536
def test_the_walk_by_label_at_scale():
    """rows, lengths and stats of search_batch_filtered with the masks, bit for bit (yardstick 2)"""
    w, lab, lb = gworld("f32"), col("route2"), ghandle("f32", "route2")
    hix, spp = w["hix"], ph.SearchParameters(*SP)
    want = cycle([11, 12, 13, ABSENT_ROUTE, NONE, 12])
    masks = lr.masks_of(lab, want)
    assert N > 65536 and masks.sum(axis=1).max() == BELOW + 1
    ex = (w["qids"] + 1) % N
    for kw in (dict(queries=w["q"]), dict(qids=w["qids"])):
        for strict in (False, True):
            for e in (None, ex):
                ref = hix.search_batch_filtered(sp=spp, allow=masks, strict=strict, exclude=e, stats=True, **kw)
                got = hix.search_batch_labeled(sp=spp, labels=lb, want=want, strict=strict, exclude=e, stats=True, **kw)
                same(got, ref)
                np.testing.assert_array_equal(got[3], ref[3])
                if e is None:
                    dv = device_call("walk", hix, lb, sp=spp, want=want, strict=strict, **kw)
                    assert not dv[4].any()
                    same(dv, ref)
                    np.testing.assert_array_equal(dv[3], ref[3])
            if strict:  # a wanted NONE returns nothing, not even the entry vector
                assert (got[2] > 0).any() and not got[2][want == NONE].any() and not got[2][want == ABSENT_ROUTE].any()


# ---------------------------------------------------------------- 7: wide queries
@pytest.mark.parametrize("dim", [24, 256])
def test_wide_queries(monkeypatch, dim):
    """ldq = ld + 8: the rows of the ldq == ld call.  NaN fills the columns past ld: a kernel that read a query row at
    the store's stride, or past ld, would return other rows"""
    if dim == 24:
        w, lab, lb = gworld("f32"), col("route2"), ghandle("f32", "route2")
        hix, q = w["hix"], w["q"]
        want = cycle([11, 12, 13, ABSENT_ROUTE, NONE])
    else:  # N = 5000, a ring index: the walk over it is no search, but it reads the query all the same
        import test_gpu_exact_labeled as tl
        from test_gpu_exact_shared import sworld
        w, lab, lb = sworld("f32", 256), tl.column(), tl.handle("f32", 256)
        hix, q = w["hix"], w["q"]
        want = tl.cycle_want()
    spp = ph.SearchParameters(*SP)
    assert hix.store.ld >= dim and hix.store.ld % 4 == 0
    for tile in (None, "1"):
        with env(monkeypatch, **knobs(None, tile)):
            for which, kw in (("exact", dict(k=K)), ("walk", dict(sp=spp, strict=True)), ("auto", dict(sp=spp, k=K, scan_below=100))):
                narrow = device_call(which, hix, lb, queries=q, want=want, **kw)
                wide = device_call(which, hix, lb, queries=q, want=want, wide=8, **kw)
                assert not narrow[-1].any() and not wide[-1].any() and (which == "walk" or narrow[2].any())
                same(wide, narrow)
                for a, b in zip(wide[3:], narrow[3:]):  # stats or routes, status
                    np.testing.assert_array_equal(a, b)
        if tile is None:  # and the narrow rows are the established scan's (yardstick 2)
            same(device_call("exact", hix, lb, queries=q, want=want, k=K),
                 hix.search_exact_filtered(queries=q, allow=lr.masks_of(lab, want), k=K))
