"""Run time on an MI355X: 22 s (59 cases, first clean run); run it under `timeout -k 10 66`, three times that.

The filter stack (filter_exact.hip, filter_dense.hip, filter_auto.hip, the exact scan through hostpath.hip) at the
smallest shapes where every loop over the bitmap or the batch turns more than once.  tests/test_gpu_exact_filter.py,
test_gpu_exact_shared.py and test_gpu_filter_auto.py cover kinds, dimensions, k, exclude, ties and refusals on one world
of 5000 rows (157 bitmap words, at most 70 queries), where each of those loops turns at most once and what they carry
from turn to turn is never read.  Every comparison is on ids, distance bits, lengths, status and routes, no tolerance
anywhere.

World A, N = 70 001 rows: 2188 = 2 * 1024 + 140 bitmap words, so 9 trips of the count loop (256 words), 3 of the prefix
kernel (1024 words), 35 passes of the scan (64 words, the last of 12), N % 32 == 17 and N > 65 536, the clamp of the
table's node chunks.  40 copies of row 0 at linspace(0, N - 1, 40): ties cross pass, slice, prefix-block and node-chunk
borders and the ids decide; query 0 is the duplicated row, stored query 0 one of its copies.
World B, f32 rows of 24 floats at n = 32 768 (exactly 1024 words: one full trip, 16 passes) and n = 32 769 (word 1024
holds one valid bit, pass 17 one word).

Yardstick: tests/exact_filter_reference.py over the oracle's ORC_SUM_BLOCKED64 distances of store.read() (lattice rows
on i8q), which the code under test did not make; compare_vec for PQ, as tests/test_gpu_exact_filter.py; for the graph
rows of the routed call tests/filter_auto_reference.compose over search_exact_filtered and
search_batch_filtered(strict=True) on the same inputs -- the scan half is pinned against the oracle on this very world
by section 1.  Where a test claims that a loop turns again it asserts the shape that makes it turn
(tests/filter_scale_reference.py restates the integer rules, pinned by tests/test_filter_scale_cpu.py).

Not exercised: nothing here asks for more than 600 queries, so the 65 536-block clamp of ph_auto_finish_kernel and the
2^20 grid clamps of the scan, the merge, the count and the select stay unexercised."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import filter_auto_reference as ar
import filter_reference as fr
import filter_scale_reference as sr
from test_gpu_exact_filter import device_exact, mask, ring, same
from test_gpu_exact_shared import check as shared_check
from test_gpu_filter_auto import device_auto
from test_gpu_i8 import adopt, bits, oracle_over
from test_gpu_i8q import env, lattice_rows

pytestmark = pytest.mark.gpu

N, NW, PASSES = 70001, 2188, 35
NB = (32768, 32769)
NQ, NS, NQX, NQR = 16, 8, 65, 600
COS = oracle.METRIC_COSINE_HALF
EMPTY = xr.EMPTY
DUPS = np.linspace(0, N - 1, 40).astype(np.int64)  # ids of the 40 copies of row 0: first and last id among them
PQ_M = 12
SP, K = (64, 64, 2), 10
SLICES = (None, "1", "2", "3", "4", "6", "34", "35", "1000")
WHOLE, CHUNKED = "4000000000,1024,4096", "0,5,7"  # PHNSW_HOST_CHUNKS: the list whole; a chunk of 5, then pieces of <= 7
EVEN = np.arange(N) % 2 == 0

# the shapes the module is about, on the CPU at collection
assert sr.words_of(N) == NW == 2 * 1024 + 140 and sr.passes_of(N) == PASSES and NW - 34 * sr.PASS_WORDS == 12
assert sr.trips(NW, sr.COUNT_THREADS) == 9 and sr.trips(NW, sr.PREFIX_WORDS) == 3
assert N % 32 == 17 and N > sr.DENSE_NODES_MAX
assert sr.words_of(NB[0]) == 1024 and sr.passes_of(NB[0]) == 16 and NB[0] % 32 == 0
assert sr.words_of(NB[1]) == 1025 and sr.passes_of(NB[1]) == 17 and NB[1] % 32 == 1
assert NQR == 2 * sr.ROUTE_QUERIES + 88 and sr.trips(NQR, sr.ROUTE_QUERIES) == 3
assert len(np.unique(DUPS // sr.PASS_IDS)) == PASSES          # a copy in every pass of the scan
assert len(np.unique(DUPS // (32 * sr.PREFIX_WORDS))) == 3    # ... and in every trip of the prefix kernel


# ---------------------------------------------------------------- the worlds
@functools.lru_cache(maxsize=None)
def rows_a(lattice, dim):
    rows = lattice_rows(N, dim, 7919 + dim) if lattice else oracle.synth_rows(0, N, dim)[:, :dim].copy()
    rows[DUPS] = rows[0]
    return rows


@functools.lru_cache(maxsize=None)
def full_store(lattice, dim):
    return ph.VectorStore(rows_a(lattice, dim), metric=COS)


@functools.lru_cache(maxsize=None)
def store_of(kind, dim):
    full = full_store(kind == "i8q", dim)
    return {"f32": lambda f: f, "f16": ph.F16Store.from_full, "i8": ph.I8Store.from_full, "i8q": ph.I8QStore.from_full,
            "pq": lambda f: ph.PqStore(f, PQ_M)}[kind](full)


def stored_ids(n, dups, count):
    """one of the copies, ids either side of pass borders, the last id, then an even spread"""
    head = [int(dups[3]), 1, 77, 2047, 2048, 4095, n // 2, n - 1]
    return np.array(head + np.linspace(2, n - 2, count - len(head)).astype(np.int64).tolist(), dtype=np.uint64)


def distances(store, kind, q, qids):
    if kind == "pq":
        every = np.arange(store.n, dtype=np.uint64)
        return (np.stack([store.compare_vec(ph.Unstored(np.ascontiguousarray(v)), every) for v in q]),
                np.stack([store.compare_vec(ph.Stored(int(v)), every) for v in qids]))
    oix = oracle_over(store, COS)
    return (fr.distance_rows(oix, queries=q, mode=oracle.SUM_BLOCKED64),
            fr.distance_rows(oix, qids=qids, mode=oracle.SUM_BLOCKED64))


@functools.lru_cache(maxsize=None)
def world(kind, dim):
    """World A: store of `kind`, a ring index over all of it, 65 raw and 65 stored queries (8 stored ones on PQ) and the
    yardstick's distance of each to every row; made once per (kind, dim), changed by no test"""
    store = store_of(kind, dim)
    q = lattice_rows(NQX, dim, 104729 + dim) if kind == "i8q" else oracle.synth_rows(2 ** 32, NQX, dim)[:, :dim].copy()
    q[0] = rows_a(kind == "i8q", dim)[0]  # the duplicated row itself: 40 candidates tie for the first place
    qids = stored_ids(N, DUPS, NS if kind == "pq" else NQX)
    Dq, Ds = distances(store, kind, q, qids)
    return dict(store=store, hix=ph.Hnsw.from_layers(store, ring(np.arange(N))), q=q, qids=qids, Dq=Dq, Ds=Ds)


@functools.lru_cache(maxsize=None)
def half_index(kind, dim):
    """a ring over every second vector of World A: vec2node is not the identity"""
    return ph.Hnsw.from_layers(store_of(kind, dim), ring(np.arange(0, N, 2)))


@functools.lru_cache(maxsize=None)
def world_b(n):
    """World B: f32 rows of 24 floats, a ring index, 16 raw and 16 stored queries"""
    dups = np.linspace(0, n - 1, 40).astype(np.int64)
    rows = oracle.synth_rows(0, n, 24)[:, :24].copy()
    rows[dups] = rows[0]
    store = ph.VectorStore(rows, metric=COS)
    q = oracle.synth_rows(2 ** 32, NQ, 24)[:, :24].copy()
    q[0] = rows[0]
    qids = stored_ids(n, dups, NQ)
    Dq, Ds = distances(store, "f32", q, qids)
    return dict(store=store, hix=ph.Hnsw.from_layers(store, ring(np.arange(n))), q=q, qids=qids, Dq=Dq, Ds=Ds, n=n)


@functools.lru_cache(maxsize=None)
def graph():
    return ph.Hnsw.generate(full_store(False, 24), np.arange(N, dtype=np.uint64), ph.BuildParameters(seed=1))


@functools.lru_cache(maxsize=None)
def gworld(kind):
    """World A's built graph (over the f32 rows of 24 floats) adopted onto the store of `kind`, 600 raw queries and
    600 stored ones"""
    g = graph()
    hix = g if kind == "f32" else adopt(store_of(kind, 24), g)
    q = lattice_rows(NQR, 24, 1299709) if kind == "i8q" else oracle.synth_rows(2 ** 34, NQR, 24)[:, :24].copy()
    qids = (np.arange(NQR, dtype=np.uint64) * 113 + 5) % N
    return dict(hix=hix, q=q, qids=qids)


# ---------------------------------------------------------------- 1: the scan over many passes
def scan_check(w, allow=None, exclude=None, k=10, nq=NQ, ns=NS, members=None, hix=None, ref_allow=None, device=False,
               keep=None):
    """raw and stored queries, host (and device) form, against the restatement over the yardstick's distances.  allow:
    what the call gets (a bool mask or packed words); ref_allow: the same as a bool mask where `allow` is packed or
    None with a default filter.  Per-query arrays have at least nq rows; the stored queries use the first ns.  keep: a
    dict that holds the restatement's rows from one call to the next (they do not depend on the slices).
    Returns the host results (raw, stored)."""
    hix = hix or w["hix"]
    n = hix.store.n
    out = []
    for form, (kw, D) in enumerate(((dict(queries=w["q"][:nq]), w["Dq"][:nq]), (dict(qids=w["qids"][:ns]), w["Ds"][:ns]))):
        m = len(D)
        a, ra = (None if x is None else (x if np.ndim(x) == 1 else x[:m]) for x in (allow, allow if ref_allow is None else ref_allow))
        e = None if exclude is None else exclude[:m]
        if keep is not None and form in keep:
            ref = keep[form]
        else:
            ref = xr.exact_topk(D, ra, e, members, k)
            if keep is not None:
                keep[form] = ref
        got = hix.search_exact_filtered(allow=a, exclude=e, k=k, **kw)
        same(got, ref)
        pad = np.arange(k)[None, :] >= got[2][:, None]
        assert (got[0][pad] == EMPTY).all() and (bits(got[1])[pad] == bits(xr.FMAX)).all()
        if device:
            dv = device_exact(hix, k, allow=a, exclude=e, **kw)
            assert not dv[3].any()
            same(dv, ref)
        out.append(got)
    assert n == D.shape[1]
    return out


def mixed_exclude(per_q):
    """per query in turn: a candidate whose word lies in a pass past the third, a non-candidate, PHNSW_EMPTY, an id
    past n"""
    ex = np.full(len(per_q), EMPTY, dtype=np.uint64)
    for i in range(len(per_q)):
        inside, outside = np.nonzero(per_q[i])[0], np.nonzero(~per_q[i])[0]
        late = inside[inside >= 3 * sr.PASS_IDS]
        ex[i] = (int(late[i % len(late)]), int(outside[len(outside) // 2]), EMPTY, N + 7)[i % 4]
    return ex


@functools.lru_cache(maxsize=None)
def scan_cases(nq):
    """the bitmaps, exclude lists and k of section 1 for a batch of nq raw queries: name -> dict(allow, exclude, k).
    The restatement's rows are added per kind by the first test that needs them"""
    dense = mask(0.3, N, 11)
    dense[DUPS] = True
    sparse_q = mask(0.001, (nq, N), 12)  # about 70 candidates per query: most passes are empty
    assert (sparse_q.sum(axis=1) < 200).all() and (sparse_q[:, 3 * sr.PASS_IDS:].sum(axis=1) > 0).all()
    empty_passes = PASSES - len(np.unique(np.nonzero(sparse_q[0])[0] // sr.PASS_IDS))
    assert empty_passes >= 1, "no pass of the sparse bitmap is empty: `continue` never runs"
    late = np.array([int(np.nonzero(r)[0][np.nonzero(r)[0] >= 3 * sr.PASS_IDS][i % 5]) for i, r in enumerate(sparse_q)], dtype=np.uint64)
    last_pass = np.arange(N) >= (PASSES - 1) * sr.PASS_IDS
    ends = sr.words_mask(N, [0, NW - 1])
    assert ends.sum() == 32 + 17
    border = np.zeros((nq, N), dtype=bool)
    border[np.arange(nq), np.array([2047, 2048, N - 1])[np.arange(nq) % 3]] = True  # one candidate, at a pass border
    return {
        "dense shared, k 1024": dict(allow=dense, exclude=None, k=1024),
        "dense per query, k 10": dict(allow=mask(0.3, (nq, N), 13), exclude=None, k=10),
        "sparse shared, k 10": dict(allow=mask(0.001, N, 14), exclude=None, k=10),
        "sparse per query, a late candidate excluded, k 10": dict(allow=sparse_q, exclude=late, k=10),
        "sparse per query, every kind of exclude, k 1024": dict(allow=sparse_q, exclude=mixed_exclude(sparse_q), k=1024),
        "no bitmap, k 1": dict(allow=None, exclude=None, k=1),
        "the last pass only, k 1024": dict(allow=last_pass, exclude=None, k=1024),
        "words 0 and 2187 only, k 1024": dict(allow=ends, exclude=None, k=1024),
        "one candidate per query at a pass border, k 10": dict(allow=border, exclude=None, k=10),
    }


KEPT = {}  # (kind, dim, nq, case) -> the restatement's rows by form


@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("i8q", 24), ("pq", 24)])
def test_the_scan_over_many_passes_whatever_the_slices(monkeypatch, kind, dim, slices):
    w = world(kind, dim)
    cases = scan_cases(NQ)
    if slices is not None:  # the ranges this slice count cuts the 35 passes into: the issue's figures, from the rule
        sizes = [b - a for a, b in sr.slice_ranges(PASSES, int(slices))]
        assert sum(sizes) == PASSES and sizes == {"1": [35], "2": [17, 18], "3": [11, 12, 12], "4": [8, 9, 9, 9],
                                                  "6": [5, 6, 6, 6, 6, 6], "35": [1] * 35, "1000": [1] * 35}.get(slices, sizes)
        if slices == "34":
            assert sorted(sizes) == [1] * 33 + [2]
    dense = cases["dense shared, k 1024"]["allow"]
    assert len(np.unique(np.nonzero(dense)[0] // sr.PASS_IDS)) == PASSES  # candidates in every pass: stage[] is reused
    if slices == "6":  # six lists, every one full at k = 1024: the merge reads more than three and leaves them early
        per_pass = np.bincount(np.nonzero(dense)[0] // sr.PASS_IDS, minlength=PASSES)
        assert all(per_pass[a:b].sum() >= 1024 for a, b in sr.slice_ranges(PASSES, 6))
    kv = {} if slices is None else dict(PHNSW_EXACT_SLICES=slices)
    with env(monkeypatch, **kv):
        for name, c in cases.items():
            got = scan_check(w, allow=c["allow"], exclude=c["exclude"], k=c["k"], device=slices in (None, "6", "34"),
                             keep=KEPT.setdefault((kind, dim, NQ, name), {}))
            if name == "dense shared, k 1024":
                # every list full: with six slices or more the merge reads more than three full lists
                assert (got[0][2] == 1024).all() and (got[1][2] == 1024).all()
                if kind != "i8q":  # normalised rows: nothing is nearer to a row than its copies
                    for g in got:  # query 0 is the duplicated row, stored query 0 one of its copies
                        np.testing.assert_array_equal(g[0][0, :40], DUPS.astype(np.uint64))
            if name == "the last pass only, k 1024":
                assert (got[0][2] == N - (PASSES - 1) * sr.PASS_IDS).all() and (got[0][0][:, 0] >= (PASSES - 1) * sr.PASS_IDS).all()
            if name == "words 0 and 2187 only, k 1024":
                for g in got:  # all 49 come back: the first and the last slice both had a say
                    assert (g[2] == 49).all() and (g[0][:, 0:49] < 32).any() and (g[0][:, :49] >= (NW - 1) * 32).any()
            if name == "one candidate per query at a pass border, k 10":
                assert (got[0][2] == 1).all()
                np.testing.assert_array_equal(got[0][0][:, 0], np.array([2047, 2048, N - 1], dtype=np.uint64)[np.arange(NQ) % 3])
            if name == "sparse per query, a late candidate excluded, k 10":
                assert (c["exclude"] >= 3 * sr.PASS_IDS).all() and not (got[0][0] == c["exclude"][:NQ, None]).any()


@pytest.mark.parametrize("kind,dim", [("f32", 24), ("i8q", 24), ("pq", 24)])
def test_65_queries_and_the_default_slice_rule(monkeypatch, kind, dim):
    """With 65 queries at k = 1024 the default rule is not clamped to the 35 passes: a wave of the scan holds
    ph_exact_own_lds(1024) = 25 088 bytes of the 160 KiB a compute unit has, so at most 6 waves per unit are resident;
    on U units ceil(resident / 65) lies between ceil(U / 65) and ceil(6 U / 65), which for the part's 256 units is
    4 .. 24: several slices, fewer than passes, several passes each."""
    import torch
    w = world(kind, dim)
    units = torch.cuda.get_device_properties(0).multi_processor_count
    own = 2 * 1024 * 8 + 64 * 8 + sr.PASS_IDS * 4
    lo, hi = -(-units // NQX), -(-(160 * 1024 // own) * units // NQX)
    if kind != "pq":  # (a PQ table in LDS lowers the residency, not the bound)
        assert own == 25088 and 1 < lo and hi < PASSES, (units, lo, hi)
    cases = scan_cases(NQX)
    for slices in (None, "6"):
        with env(monkeypatch, **({} if slices is None else dict(PHNSW_EXACT_SLICES=slices))):
            for name in ("dense shared, k 1024", "sparse per query, every kind of exclude, k 1024",
                         "sparse per query, a late candidate excluded, k 10", "no bitmap, k 1"):
                c = cases[name]
                scan_check(w, allow=c["allow"], exclude=c["exclude"], k=c["k"], nq=NQX, device=slices is None,
                           keep=KEPT.setdefault((kind, dim, NQX, name), {}))


@pytest.mark.parametrize("kind,dim", [("f32", 24), ("i8q", 24), ("pq", 24)])
def test_filter_count_over_nine_trips(kind, dim):
    w = world(kind, dim)
    hix, half = w["hix"], half_index(kind, dim)
    per_q = mask(0.1, (NQX, N), 21)
    per_q[0], per_q[1], per_q[2] = False, True, sr.words_mask(N, [255, 256, 2047, 2048, NW - 1])  # either side of a trip
    words = fr.pack(per_q)
    assert words.shape == (NQX, NW) and NW > 8 * sr.COUNT_THREADS  # thread 0 counts nine words, thread 140 eight
    want = sr.popcount_candidates(words, N)
    np.testing.assert_array_equal(want, per_q.sum(axis=1))
    assert want[0] == 0 and want[1] == N and want[2] == 4 * 32 + 17
    np.testing.assert_array_equal(hix.filter_count(per_q), want)
    np.testing.assert_array_equal(half.filter_count(per_q), sr.popcount_candidates(words, N, EVEN))
    for shared in (mask(0.3, N, 22), mask(0.001, N, 23), np.ones(N, dtype=bool)):
        assert hix.filter_count(shared) == sr.popcount_candidates(fr.pack(shared), N)[0] == shared.sum()
        assert half.filter_count(shared) == (shared & EVEN).sum()
    assert hix.filter_count(None) == N and half.filter_count(None) == (N + 1) // 2
    wide = np.full((NQX, NW + 5), 0xFFFFFFFF, dtype=np.uint32)  # dirty bits at and past n, and between the bitmaps
    wide[:, :NW] = words
    wide[:, NW - 1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    np.testing.assert_array_equal(sr.popcount_candidates(wide, N), want)
    np.testing.assert_array_equal(hix.filter_count(wide), want)
    np.testing.assert_array_equal(half.filter_count(wide), sr.popcount_candidates(words, N, EVEN))
    dirty = fr.pack(mask(0.3, N, 22))
    dirty[-1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    assert hix.filter_count(dirty) == mask(0.3, N, 22).sum()


@pytest.mark.parametrize("n", NB)
def test_the_scan_at_exactly_1024_words_and_one_bit_more(monkeypatch, n):
    w = world_b(n)
    dense = mask(0.3, n, 31)
    for slices in (None, "4"):
        with env(monkeypatch, **({} if slices is None else dict(PHNSW_EXACT_SLICES=slices))):
            for allow in (dense, np.ones(n, dtype=bool)):
                for k in (10, 1024):
                    got = scan_check(w, allow=allow, k=k, device=slices == "4")
                    assert (got[0][2] == k).all()
    if n == NB[1]:  # the one id of word 1024, alone in pass 17
        one = np.zeros(n, dtype=bool)
        one[n - 1] = True
        got = scan_check(w, allow=one, k=10, device=True)
        assert (got[0][2] == 1).all() and (got[0][0][:, 0] == n - 1).all()
    assert w["hix"].filter_count(dense) == dense.sum() and w["hix"].filter_count(None) == n


# ---------------------------------------------------------------- 2: the shared-bitmap table
DENSE = [(24, 16), (24, 40), (24, 65), (256, 16), (256, 40), (256, 65)]


@pytest.mark.parametrize("dim,nq", DENSE)
def test_the_default_node_chunks(dim, nq):
    """no knob set: one chunk, the edge of the default chunk, two, three and nine chunks"""
    w = world("f32", dim)
    for c, chunks in ((8191, [8191]), (8192, [8192]), (8193, [8192, 1]), (20000, [8192, 8192, 3616]), (N, [8192] * 8 + [4465])):
        assert sr.node_chunks(c) == chunks
        allow = np.ones(N, dtype=bool) if c == N else sr.exactly_of(N, c, 100 + c, first=DUPS)
        for k in (10, 1024):
            got = shared_check(w, nq=nq, allow=allow, k=k, device=nq == 40 and k == 10)
            for form in (0, 1):
                assert (got[form][2] == k).all() and allow.sum() == c  # len == min(k, c) with c > 8192 past the edge
        if c > sr.DENSE_NODES:  # ids of the later chunks are among the rows returned
            later = np.nonzero(allow)[0][sr.DENSE_NODES]
            assert (got[0][0] >= later).any()


@pytest.mark.parametrize("dim,nq", [(24, 16), (256, 40), (24, 65)])
def test_the_node_chunk_clamp(monkeypatch, dim, nq):
    """PHNSW_DENSE_NODES=65536 is the largest chunk there is and 100000 is clamped to it: the same rows, and those of
    the default chunks"""
    w = world("f32", dim)
    hix = w["hix"]
    for c in (65536, 65537, N):
        allow = np.ones(N, dtype=bool) if c == N else sr.exactly_of(N, c, 200 + c, first=DUPS)
        assert sr.node_chunks(c, 65536) == sr.node_chunks(c, 100000) == ([65536] if c == 65536 else [65536, c - 65536])
        for k in (10, 1024):
            with env(monkeypatch, PHNSW_DENSE_NODES="65536"):
                base = shared_check(w, nq=nq, allow=allow, k=k, device=k == 10, forms=(0,) if k == 1024 else (0, 1))
            with env(monkeypatch, PHNSW_DENSE_NODES="100000"):
                same(hix.search_exact_shared(queries=w["q"][:nq], allow=allow, k=k), base[0])
                if 1 in base:
                    same(hix.search_exact_shared(qids=w["qids"][:nq], allow=allow, k=k), base[1])
            same(hix.search_exact_shared(queries=w["q"][:nq], allow=allow, k=k), base[0])  # no knob: the default chunks


def test_the_int8_table_over_three_node_chunks():
    w = world("i8q", 256)
    allow = sr.exactly_of(N, 20000, 7, first=DUPS)
    assert len(sr.node_chunks(20000)) == 3
    for k in (10, 1024):
        shared_check(w, nq=40, allow=allow, k=k, device=k == 10)


def listed(w, allow, nq=NQ):
    """every candidate of a bitmap with at most 1024 of them, as the table's list gave them to the select: the rows at
    k = 1024 hold the list whole"""
    c = int(allow.sum())
    assert 0 < c <= 1024
    got = shared_check(w, nq=nq, allow=allow, k=1024, device=True)
    for form in (0, 1):
        assert (got[form][2] == c).all()  # len == c
        for row in got[form][0]:
            np.testing.assert_array_equal(np.sort(row[:c]), np.nonzero(allow)[0].astype(np.uint64))
    return got


@pytest.mark.parametrize("which", ["A", NB[0], NB[1]])
def test_the_candidate_list_across_prefix_trips(which):
    """the list's offsets are an exclusive prefix over the bitmap words, 1024 words a trip with the running base
    carried: a wrong base puts the ids of words past 1023 elsewhere in the list, or nowhere"""
    w = world("f32", 24) if which == "A" else world_b(which)
    n = N if which == "A" else which
    nw = sr.words_of(n)
    rng = np.random.default_rng(41)

    def sparse_in(lo_word, count):
        m = np.zeros(n, dtype=bool)
        pool = np.arange(lo_word * 32, n)
        m[rng.permutation(pool)[:min(count, len(pool))]] = True
        return m

    edge = sr.words_mask(n, [x for x in (1023, 1024, 1025) if x < nw])  # all ones either side of the first carry
    assert edge.sum() == {N: 96, NB[0]: 32, NB[1]: 33}[n]
    got = listed(w, edge)
    if nw > 1024:
        assert (got[0][0][:, :int(edge.sum())] >= 32768).any()  # an id of the second trip came back
        late = sparse_in(1024, 700)  # candidates in words >= 1024 only: every offset is the carried base plus little
        assert late.sum() == min(700, n - 32768) and not late[:32768].any()
        listed(w, late)
        one = np.zeros(n, dtype=bool)
        one[32768] = True
        got = listed(w, one)
        assert (got[0][0][:, 0] == 32768).all() and (got[1][0][:, 0] == 32768).all()
        both = sparse_in(0, 900)  # both sides of the carry
        assert both[:32768].any() and (both[32768:].any() or n == NB[1])
        listed(w, both)
    if nw > 2048:  # World A: the third trip
        third = sparse_in(2048, 500)
        assert third.sum() == 500 and not third[:65536].any()
        listed(w, third)
        dense_late = np.arange(n) >= 32768  # 37 233 candidates, five node chunks, none in the first trip
        assert len(sr.node_chunks(int(dense_late.sum()))) == 5
        for k in (10, 1024):
            got = shared_check(w, nq=NQ, allow=dense_late, k=k, device=False)
            assert (got[0][0] >= 32768).all() and (got[0][2] == k).all()
        dense_third = np.arange(n) >= 65536
        got = shared_check(w, nq=NQ, allow=dense_third, k=1024)
        assert (got[0][0] >= 65536).all() and (got[0][2] == 1024).all()
    if nw == 1024:  # exactly one full trip, no carry: the total alone is written after the loop
        listed(w, sparse_in(1000, 700))
        shared_check(w, nq=NQ, allow=np.ones(n, dtype=bool), k=1024)


@pytest.mark.parametrize("dim,nq", [(24, 16), (256, 40)])
def test_the_table_over_an_index_of_every_second_vector(dim, nq):
    w = world("f32", dim)
    half = half_index("f32", dim)
    ones = np.ones(N, dtype=bool)
    assert (ones & EVEN).sum() == 35001 and len(sr.node_chunks(35001)) == 5
    for k in (10, 1024):
        got = shared_check(w, nq=nq, allow=ones, members=EVEN, hix=half, k=k, device=k == 10)
        for form in (0, 1):
            assert not (got[form][0] % 2).any() and (got[form][2] == k).all()
            if k == 1024:  # the even copies of row 0 tie for query 0's first places; id 70 000 is in the fifth chunk
                assert DUPS[-1] % 2 == 0 and (got[form][0][0] == DUPS[-1]).any() and DUPS[-1] > 2 * 4 * sr.DENSE_NODES


# ---------------------------------------------------------------- 3: the routed call past 256 queries
@functools.lru_cache(maxsize=None)
def first_graph():
    return ar.first_graph_count(SP[0], K, N)


def edge_cycle():
    e = first_graph()
    return [0, 1, K, ar.SCAN_BELOW_PER_QUERY, ar.SCAN_BELOW_PER_QUERY + 1, e - 1, e, 20000, N]


@functools.lru_cache(maxsize=None)
def cycled_bitmaps(seed, kind="f32", stored=False):
    """bool [600, N]: the counts of edge_cycle() in turn, rows drawn at random -- but past the first 256 queries a
    query with exactly e candidates allows the e rows FARTHEST from it (numpy, on the store's rows, as
    tests/test_gpu_filter_auto.py's `farthest`): the rule says graph, and a walk towards the query ends among rows it
    may not return, so the row comes back short and the scan is asked again"""
    counts = sr.cycle_counts(NQR, edge_cycle())
    allow = sr.bitmaps_of(N, counts, seed)
    w, e = gworld(kind), first_graph()
    rows = rows_a(kind == "i8q", 24).astype(np.float64)
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    for i in range(sr.ROUTE_QUERIES, NQR):
        if counts[i] == e:
            v = rows[int(w["qids"][i])] if stored else w["q"][i].astype(np.float64)
            allow[i] = False
            allow[i, np.argsort(-(unit @ (v / np.linalg.norm(v))), kind="stable")[N - e:]] = True
    assert allow.sum(axis=1).tolist() == counts
    return allow


def routed_check(w, allow, exclude=None, stored=False, device=False, sp=SP):
    """the host form (and the device form on a side stream) with scan_below = 0, so the library's thresholds decide,
    against ROWS, ROUTES and COMPLETE as tests/test_gpu_filter_auto.py names them.  Returns the host result."""
    hix, spp = w["hix"], ph.SearchParameters(*sp)
    kw = dict(qids=w["qids"]) if stored else dict(queries=w["q"])
    got = hix.search_filtered(sp=spp, allow=allow, exclude=exclude, k=K, scan_below=0, route=True, **kw)
    walk = hix.search_batch_filtered(sp=spp, allow=allow, strict=True, exclude=exclude, **kw)
    scan = hix.search_exact_filtered(allow=allow, exclude=exclude, k=K, **kw)
    want = ar.compose(walk, scan, N, sp[0], K, N, allow, exclude, None, 0)
    print("routes", np.bincount(got[3], minlength=3).tolist(), "expected", np.bincount(want[3], minlength=3).tolist())
    np.testing.assert_array_equal(got[3], want[3])
    same(got, want)                                   # ROWS
    per_query = allow is not None and np.ndim(allow) == 2
    counts = hix.filter_count(allow)
    np.testing.assert_array_equal(counts, allow.sum(axis=-1) if allow is not None else N)
    for i in range(NQR):                              # ROUTES: the rule on what filter_count reports
        r = ar.rule(counts[i] if per_query else counts, 0, sp[0], K, N, per_query)
        assert got[3][i] == r or (got[3][i] == ar.GRAPH_THEN_SCAN and r == ar.GRAPH), (i, got[3][i], r)
    ar.assert_complete(got, N, K, allow, exclude, None)  # COMPLETE
    if device:
        import torch
        assert exclude is None
        stream = torch.cuda.Stream()
        dv = device_auto(hix, spp, K, allow=allow, scan_below=0, stream=stream.cuda_stream, **kw)
        assert not dv[4].any()
        same(dv, got)
        np.testing.assert_array_equal(dv[3], got[3])
    return got


def both_routes_in_every_wave(route):
    """every wave of 64 queries of every 256-block holds scanned and walked queries"""
    for at in range(0, NQR, 64):
        r = route[at:at + 64]
        assert (r == ar.SCAN).any() and (r != ar.SCAN).any(), at


@pytest.mark.parametrize("stored", [False, True])
def test_the_routed_call_over_three_blocks_of_queries(stored):
    w = gworld("f32")
    e = first_graph()
    assert ar.SCAN_BELOW_PER_QUERY + 1 < e - 1 and e < 20000  # 10 001 and e - 1 scan by the second rule alone
    allow = cycled_bitmaps(51, "f32", stored)
    got = routed_check(w, allow, stored=stored, device=not stored)
    want = np.array([ar.SCAN] * 6 + [ar.GRAPH] * 3)[np.arange(NQR) % 9]
    np.testing.assert_array_equal(got[3] == ar.SCAN, want == ar.SCAN)
    both_routes_in_every_wave(got[3])
    assert (got[3][sr.ROUTE_QUERIES:] == ar.GRAPH_THEN_SCAN).any()  # a short walk behind a carried scan-list base
    assert (got[3][2 * sr.ROUTE_QUERIES:] == ar.GRAPH).any() and (got[3][2 * sr.ROUTE_QUERIES:] == ar.SCAN).any()
    # exclude: each query's nearest candidate (EMPTY where there is none)
    kw = dict(qids=w["qids"]) if stored else dict(queries=w["q"])
    ex = w["hix"].search_exact_filtered(allow=allow, k=1, **kw)[0][:, 0].copy()
    got = routed_check(w, allow, exclude=ex, stored=stored)
    assert not ((got[0] == ex[:, None]) & (ex[:, None] != EMPTY)).any()
    assert (got[3][sr.ROUTE_QUERIES:] == ar.GRAPH_THEN_SCAN).any()


@pytest.mark.parametrize("scan_first", [True, False])
def test_a_block_of_scans_next_to_blocks_of_walks(scan_first):
    """queries 0..255 all scan and the rest all walk, and the reverse: one list's carried base is 0 where the other's
    is 256, so a base that is off by a block puts a query in the wrong list place"""
    w = gworld("f32")
    e = first_graph()
    scans, walks = [0, 1, K, 5000, ar.SCAN_BELOW_PER_QUERY, e - 1], [e, 20000, N]
    head, tail = (scans, walks) if scan_first else (walks, scans)
    allow = sr.bitmaps_of(N, sr.arranged_counts(NQR, sr.ROUTE_QUERIES, head, tail), 61 + scan_first)
    got = routed_check(w, allow, stored=not scan_first, device=scan_first)
    first = got[3][:sr.ROUTE_QUERIES] == ar.SCAN
    rest = got[3][sr.ROUTE_QUERIES:] == ar.SCAN
    assert first.all() == scan_first and first.any() == scan_first and rest.all() != scan_first and rest.any() != scan_first


def test_the_shared_threshold_decides_for_600_queries():
    w = gworld("f32")
    e = first_graph()
    assert e <= ar.SCAN_BELOW_SHARED  # the second rule lets go below the threshold: 13 000 / 13 001 is the first rule's edge
    lo = sr.exactly_of(N, ar.SCAN_BELOW_SHARED, 71, first=DUPS)
    hi = sr.exactly_of(N, ar.SCAN_BELOW_SHARED + 1, 72, first=DUPS)
    for stored in (False, True):
        got = routed_check(w, lo, stored=stored, device=not stored)
        assert (got[3] == ar.SCAN).all()
        got = routed_check(w, hi, stored=stored, device=not stored)
        assert (got[3] != ar.SCAN).all() and (got[3] == ar.GRAPH).any()


def test_the_per_query_threshold_decides_for_600_queries():
    """at number_of_candidates 64 the second rule holds on to 10 937 candidates, so 10 000 and 10 001 both scan in
    the cycle above; at 128 it lets go at 5469 and the library's per-query threshold alone parts 10 000 from 10 001"""
    w = gworld("f32")
    sp = (128, 128, 2)
    lo, hi = ar.SCAN_BELOW_PER_QUERY, ar.SCAN_BELOW_PER_QUERY + 1
    assert ar.first_graph_count(sp[0], K, N) <= lo
    got = routed_check(w, sr.bitmaps_of(N, sr.cycle_counts(NQR, [lo, hi]), 91), sp=sp, device=True)
    np.testing.assert_array_equal(got[3] == ar.SCAN, np.arange(NQR) % 2 == 0)


@pytest.mark.parametrize("kind", ["i8q", "pq"])
def test_the_routed_call_on_the_other_kinds(kind):
    w = gworld(kind)
    got = routed_check(w, cycled_bitmaps(51, kind), device=True)
    both_routes_in_every_wave(got[3])
    assert (got[3][sr.ROUTE_QUERIES:] == ar.GRAPH).any() and (got[3][sr.ROUTE_QUERIES:] == ar.GRAPH_THEN_SCAN).any()


# ---------------------------------------------------------------- 4: the exact scan through the host chunk pipeline
def test_the_exact_scan_through_the_host_chunk_pipeline(monkeypatch):
    """a host list in ten chunks: per-query bitmaps travel with their chunk (the chunk's first bitmap is `first *
    stride` words into the caller's), the two staging streams alternate over the index's two scratch blocks, and the
    blocks grow from chunk to chunk (5, 6 and 7 queries) and between the k = 10 and the k = 1024 call -- every index
    here is new, so they start empty and the chunked calls come first"""
    import torch
    w = world("f32", 24)
    bounds = sr.host_chunk_bounds(NQX, 0, 5, 7)
    assert len(bounds) - 1 >= 3 and bounds[1] == 5 and max(np.diff(bounds)) <= 7 and bounds[-1] == NQX
    assert sr.host_chunk_bounds(NQX, *[int(x) for x in WHOLE.split(",")]) == [0, NQX]
    per_q = mask(0.01, (NQX, N), 81)  # about 700 candidates per query, every bitmap another
    assert fr.pack(per_q).shape == (NQX, NW) and (per_q.sum(axis=1) < 1024).all() and (per_q[1:] != per_q[0]).any(axis=1).all()
    ex = mixed_exclude(per_q)
    shared = mask(0.3, N, 82)
    shared[DUPS] = True
    words = torch.from_numpy(fr.pack(shared).view(np.int32)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    for allow, ref_allow, exclude in ((per_q, per_q, ex), (shared, shared, None), (None, shared, ex)):
        hix = ph.Hnsw.from_layers(w["store"], ring(np.arange(N)))
        if allow is None:
            hix.set_filter(words.data_ptr())  # the index's default filter serves the call that passes none
        try:
            for stored in (False, True):
                kw, D = (dict(qids=w["qids"]), w["Ds"]) if stored else (dict(queries=w["q"]), w["Dq"])
                ref = {k: xr.exact_topk(D, ref_allow, exclude, None, k) for k in (10, 1024)}
                for slices in (None, "4"):
                    kv = dict(PHNSW_HOST_CHUNKS=CHUNKED)
                    if slices is not None:
                        kv["PHNSW_EXACT_SLICES"] = slices
                    with env(monkeypatch, **kv):
                        for k in (10, 1024):
                            same(hix.search_exact_filtered(allow=allow, exclude=exclude, k=k, **kw), ref[k])
                with env(monkeypatch, PHNSW_HOST_CHUNKS=WHOLE):  # the same call with the list whole
                    for k in (10, 1024):
                        same(hix.search_exact_filtered(allow=allow, exclude=exclude, k=k, **kw), ref[k])
        finally:
            hix.set_filter(0)
