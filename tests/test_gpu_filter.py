"""Searches restricted to an allow-list of VectorIds (phnsw_search_batch_filtered[_device], phnsw_index_set_filter_device):
Layer::closest_vectors' `include` (lib.rs:250-277) as a bitmap.  Every comparison is on ids, distance bits and lengths,
no tolerance anywhere.  Yardsticks: the existing exclude search (a filter with one bit cleared per query is that search),
the unfiltered search (every bit set, or no filter), and tests/filter_reference.py -- the reference's algorithm with an
arbitrary `include`, pinned to the unchanged oracle by tests/test_filter_cpu.py -- over the oracle's distances of the
rows each store really holds (store.read(); lattice data on i8q, where the integer arithmetic equals the oracle's)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from parallel_hnsw_amd._lib import lib
from parallel_hnsw_amd.hnsw import _p

import filter_reference as fr
from test_gpu_i8 import adopt, bits, oracle_over
from test_gpu_i8q import env, lattice_rows

pytestmark = pytest.mark.gpu

N = 2000
COS = oracle.METRIC_COSINE_HALF
EMPTY = fr.EMPTY
E_INVALID = -1


@functools.lru_cache(maxsize=None)
def world(kind, dim):
    """(GPU index over a store of `kind`, the oracle over store.read() with the same graph or None, its layers for the
    restatement); the graph is phnsw_build's over the f32 rows.  Made once per (kind, dim), changed by no test"""
    rows = lattice_rows(N, dim, 7919 + dim) if kind == "i8q" else oracle.synth_rows(0, N, dim)[:, :dim].copy()
    full = ph.VectorStore(rows, metric=COS)
    g = ph.Hnsw.generate(full, np.arange(N, dtype=np.uint64), ph.BuildParameters(seed=1))
    assert g.layer_count() >= 3
    if kind == "f32":
        store, hix = full, g
    else:
        store = {"f16": ph.F16Store.from_full, "i8": ph.I8Store.from_full, "i8q": ph.I8QStore.from_full,
                 "pq": lambda f: ph.PqStore(f, dim // 4)}[kind](full)
        hix = adopt(store, g)
    oix = None if kind == "pq" else oracle_over(store, COS, g)
    return hix, oix, (None if oix is None else fr.layers_of(oix)), g


@functools.lru_cache(maxsize=None)
def raw_queries(kind, dim, nq):
    if kind == "i8q":
        return lattice_rows(nq, dim, 104729 + dim)
    return oracle.synth_rows(2 ** 32, nq, dim)[:, :dim].copy()


def dist(oix, **kw):
    """the oracle's distances in the kernels' summation order (ORC_SUM_BLOCKED64)"""
    return fr.distance_rows(oix, mode=oracle.SUM_BLOCKED64, **kw)


def mask(density, shape, seed):
    return np.random.default_rng(seed).random(shape) < density


def same(a, b, stats=True):
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(bits(a[1]), bits(b[1]))
    if stats and len(a) > 3 and len(b) > 3:
        np.testing.assert_array_equal(a[3], b[3])


def device_search(hix, sp, queries=None, qids=None, allow=None, exclude=None, strict=False, upto=0, stream=0):
    """phnsw_search_batch_filtered_device with torch buffers -> ids u64, d, len u64, stats u64, status"""
    import torch
    dev = torch.device("cuda", 0)
    keep = []

    def up(a, dt):
        t = torch.from_numpy(np.ascontiguousarray(a).view(dt) if dt is not None else np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t

    nq = len(queries) if queries is not None else len(qids)
    ef = sp.number_of_candidates
    qd = qi = ex = 0
    ld = 0
    if queries is not None:
        ld = hix.store.ld
        qp = np.zeros((nq, ld), dtype=np.float32)
        qp[:, :queries.shape[1]] = queries
        qd = up(qp, None).data_ptr()
    else:
        qi = up(np.asarray(qids, dtype=np.uint32), np.int32).data_ptr()
    if exclude is not None:
        ex = up(np.asarray(exclude, dtype=np.uint32), np.int32).data_ptr()
    words, stride = ph.hnsw.pack_allow(allow, hix.store.n, nq)
    wd = 0 if words is None else up(words, np.int32).data_ptr()
    ids = torch.empty((nq, ef), dtype=torch.int32, device=dev)
    d = torch.empty((nq, ef), dtype=torch.float32, device=dev)
    ln = torch.empty(nq, dtype=torch.int32, device=dev)
    st = torch.empty((nq, 2), dtype=torch.int32, device=dev)
    status = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    hix.search_batch_filtered_device(nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd, ldq=ld,
                                     qids=qi, exclude=ex, allow=wd, allow_stride=stride, strict=strict,
                                     out_stats=st.data_ptr(), upto=upto, stream=stream)
    torch.cuda.synchronize()
    i64 = ids.cpu().numpy().view(np.uint32).astype(np.uint64)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return (i64, d.cpu().numpy(), ln.cpu().numpy().view(np.uint32).astype(np.uint64),
            st.cpu().numpy().view(np.uint32).astype(np.uint64), status.cpu().numpy())


KINDS = [("f32", 6), ("f32", 100), ("f32", 768), ("f16", 100), ("i8", 100), ("i8q", 128), ("pq", 128)]


# ---------------------------------------------------------------- 1-3: the filter as the searches that already exist
@pytest.mark.parametrize("kind,dim", KINDS)
def test_one_cleared_bit_is_the_exclude_search(kind, dim):
    hix = world(kind, dim)[0]
    sp = ph.SearchParameters(64, 32, 2)
    nq = 40
    for kw in (dict(queries=raw_queries(kind, dim, nq)), dict(qids=np.arange(5, N, N // nq, dtype=np.uint64)[:nq])):
        plain = hix.search_batch(sp=sp, stats=True, **kw)
        ex = plain[0][np.arange(nq), np.arange(nq) % 7 + 1].copy()  # a result of the unfiltered search: it matters
        allow = np.ones((nq, N), dtype=bool)
        allow[np.arange(nq), ex.astype(np.int64)] = False
        excl = hix.search_batch(sp=sp, exclude=ex, stats=True, **kw)
        assert (excl[0] != plain[0]).any()
        same(hix.search_batch_filtered(sp=sp, allow=allow, stats=True, **kw), excl)
        dv = device_search(hix, sp, allow=allow, **kw)
        assert not dv[4].any()
        same(dv, excl)


@pytest.mark.parametrize("kind,dim", KINDS)
def test_every_bit_set_and_no_filter_are_the_unfiltered_search(kind, dim):
    hix = world(kind, dim)[0]
    sp = ph.SearchParameters(128, 128, 2)
    q = raw_queries(kind, dim, 40)
    plain = hix.search_batch(queries=q, sp=sp, stats=True)
    same(hix.search_batch_filtered(queries=q, sp=sp, allow=np.ones(N, dtype=bool), stats=True), plain)
    same(hix.search_batch_filtered(queries=q, sp=sp, allow=np.ones((40, N), dtype=bool), stats=True), plain)
    same(hix.search_batch_filtered(queries=q, sp=sp, allow=None, stats=True), plain)  # NULL and no default set
    same(device_search(hix, sp, queries=q, allow=np.ones(N, dtype=bool)), plain)
    same(device_search(hix, sp, queries=q), plain)


# ---------------------------------------------------------------- 4: general filters against the restatement
NQ = 16


@pytest.mark.parametrize("per_query", [False, True], ids=["shared", "per_query"])
@pytest.mark.parametrize("density", [0.5, 0.1, 0.01])
@pytest.mark.parametrize("kind,dim", [k for k in KINDS if k[0] != "pq"])
def test_general_filters_equal_the_restatement(kind, dim, density, per_query):
    hix, oix, layers, _ = world(kind, dim)
    spt = (64, 24, 2)
    sp = ph.SearchParameters(*spt)
    allow = mask(density, (NQ, N) if per_query else N, int(density * 1000) + dim)
    q = raw_queries(kind, dim, NQ)
    qids = np.arange(11, N, N // NQ, dtype=np.uint64)[:NQ]
    Dq, Ds = dist(oix, queries=q), dist(oix, qids=qids)
    ex = np.array([np.nonzero(allow if allow.ndim == 1 else allow[i])[0][i % 3] for i in range(NQ)], dtype=np.uint64)
    for kw, D in ((dict(queries=q), Dq), (dict(qids=qids), Ds)):
        for upto in (0, 1, 2):
            for e in (None, ex):
                ref = fr.search(oix, D, spt, allow=allow, exclude=e, upto=upto, layers=layers)
                same(hix.search_batch_filtered(sp=sp, allow=allow, exclude=e, upto=upto, stats=True, **kw), ref)
        same(device_search(hix, sp, allow=allow, exclude=ex, **kw), fr.search(oix, D, spt, allow=allow, exclude=ex, layers=layers))
    # a post-filter: the filtered result is never longer than the unfiltered one
    assert (hix.search_batch_filtered(queries=q, sp=sp, allow=allow)[2] <= hix.search_batch(queries=q, sp=sp)[2]).all()


# ---------------------------------------------------------------- 5: independence of the schedule
@pytest.mark.parametrize("kind,dim", [("f32", 100), ("f16", 100), ("i8q", 128)])
def test_filtered_results_do_not_depend_on_the_schedule(monkeypatch, kind, dim):
    hix, oix, layers, _ = world(kind, dim)
    spt = (64, 24, 2)
    sp = ph.SearchParameters(*spt)
    nq = 2100  # past the batch sizes of the small-batch kernels and of the dense-only launch of a split descent
    qids = (np.arange(nq, dtype=np.uint64) * 7) % N
    shared, per_q = mask(0.5, N, 1), mask(0.3, (nq, N), 2)
    ex = (qids + 1) % N
    base = {}
    for name, allow in (("shared", shared), ("per_query", per_q)):
        base[name] = hix.search_batch_filtered(qids=qids, sp=sp, allow=allow, exclude=ex, stats=True)
        D = dist(oix, qids=qids[:8])
        a8 = allow if allow.ndim == 1 else allow[:8]
        same(tuple(x[:8] for x in base[name]), fr.search(oix, D, spt, allow=a8, exclude=ex[:8], layers=layers))
        small = hix.search_batch_filtered(qids=qids[:300], sp=sp, allow=a8 if allow.ndim == 1 else allow[:300], exclude=ex[:300],
                                          stats=True)  # a small batch: the latency kernels on f32
        same(small, tuple(x[:300] for x in base[name]))
    split = dict(PHNSW_TWO_LAUNCH_MIN="1", PHNSW_SPLIT_BYTES="1")
    count = lib().phnsw_debug_two_launch_count
    count.restype = C.c_uint64
    settings = [dict(PHNSW_NO_TINY="1"), dict(PHNSW_VISITED="global"), dict(PHNSW_NO_LAT="1"),
                dict(PHNSW_TINY_TABLE_BYTES=str(300 * 4 * N)),  # the table holds ~300 queries: chunks of the list
                dict(PHNSW_HOST_CHUNKS="0,100,250"),            # the host path in many chunks
                # a split descent: the top layers in the dense-only launch, then one launch per layer below
                dict(split, PHNSW_TINY_MAX="200"), dict(split, PHNSW_NO_TINY="1"),
                # PHNSW_NO_LOCALITY takes the split descent (and its re-ordered launches) away again: a list this
                # short runs in natural order anyway, so the switch shows only where the split is forced
                dict(split, PHNSW_NO_LOCALITY="1")]
    for kv in settings:
        with env(monkeypatch, **kv):
            before = count()
            for name, allow in (("shared", shared), ("per_query", per_q)):
                same(hix.search_batch_filtered(qids=qids, sp=sp, allow=allow, exclude=ex, stats=True), base[name])
                if "PHNSW_NO_LAT" in kv:
                    same(hix.search_batch_filtered(qids=qids[:300], sp=sp, allow=allow if allow.ndim == 1 else allow[:300],
                                                   exclude=ex[:300], stats=True), tuple(x[:300] for x in base[name]))
            if "PHNSW_TWO_LAUNCH_MIN" in kv:  # the split descent ran, or PHNSW_NO_LOCALITY switched it off
                assert (count() == before) == ("PHNSW_NO_LOCALITY" in kv)
            if "PHNSW_TINY_TABLE_BYTES" in kv:
                assert lib().phnsw_debug_last_search_chunks(hix._h) > 1
            strict_here = hix.search_batch_filtered(qids=qids, sp=sp, allow=per_q, strict=True)
        same(strict_here, fr.strict(hix.search_batch_filtered(qids=qids, sp=sp, allow=per_q), per_q), stats=False)


# ---------------------------------------------------------------- 6: every queue capacity class
@pytest.mark.parametrize("ef", [64, 128, 256, 512])
def test_queue_capacity_classes(monkeypatch, ef):
    hix, oix, layers, _ = world("f32", 100)
    q = raw_queries("f32", 100, 12)
    allow = mask(0.5, N, ef)
    ref = fr.search(oix, dist(oix, queries=q), (ef, ef, 2), allow=allow, layers=layers)
    same(hix.search_batch_filtered(queries=q, sp=ph.SearchParameters(ef, ef, 2), allow=allow, stats=True), ref)
    with env(monkeypatch, PHNSW_NO_LAT="1", PHNSW_NO_TINY="1"):  # the throughput kernel of pick_kernel_rows, rows gathered per hop
        same(hix.search_batch_filtered(queries=q, sp=ph.SearchParameters(ef, ef, 2), allow=allow, stats=True), ref)


# ---------------------------------------------------------------- 7: strict mode
@pytest.mark.parametrize("kind,dim", [("f32", 100), ("i8", 100)])
def test_strict_mode_removes_the_disallowed_entry_vector(kind, dim):
    hix, oix, layers, g = world(kind, dim)
    entry = g.entry_vector()
    spt = (64, 64, 2)
    sp = ph.SearchParameters(*spt)
    allow = mask(0.01, N, 9)
    allow[entry] = False
    q = raw_queries(kind, dim, NQ)
    ref = fr.search(oix, dist(oix, queries=q), spt, allow=allow, layers=layers)
    has = (ref[0] == entry).any(axis=1)
    assert has.sum() >= 4  # the quirk is there: the disallowed entry vector is returned
    q, ref = q[has], tuple(x[has] for x in ref)
    loose = hix.search_batch_filtered(queries=q, sp=sp, allow=allow, stats=True)
    same(loose, ref)
    want = fr.strict(ref, allow)
    assert (want[2] == ref[2] - 1).all() and not (want[0] == entry).any()
    got = hix.search_batch_filtered(queries=q, sp=sp, allow=allow, strict=True, stats=True)
    same(got, want)
    assert (got[0][:, -1] == EMPTY).all() and (bits(got[1][:, -1]) == bits(fr.FMAX)).all()
    dv = device_search(hix, sp, queries=q, allow=allow, strict=True)
    assert not dv[4].any()
    same(dv, want)
    # nothing allowed: empty rows, no error
    none = hix.search_batch_filtered(queries=q, sp=sp, allow=np.zeros(N, dtype=bool), strict=True)
    assert not none[2].any() and (none[0] == EMPTY).all() and (bits(none[1]) == bits(fr.FMAX)).all()
    dv = device_search(hix, sp, queries=q, allow=np.zeros((len(q), N), dtype=bool), strict=True)
    assert not dv[4].any() and not dv[2].any() and (dv[0] == EMPTY).all()


# ---------------------------------------------------------------- 8: the default filter of an index
def test_set_filter_serves_filtered_calls_only():
    import torch
    hix = world("f32", 100)[0]
    sp = ph.SearchParameters(64, 64, 2)
    q = raw_queries("f32", 100, 40)
    allow = mask(0.3, N, 77)
    plain = hix.search_batch(queries=q, sp=sp, stats=True)
    want = hix.search_batch_filtered(queries=q, sp=sp, allow=allow, stats=True)
    assert (want[0] != plain[0]).any()
    words = torch.from_numpy(fr.pack(allow).view(np.int32)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    hix.set_filter(words.data_ptr())
    try:
        same(hix.search_batch_filtered(queries=q, sp=sp, stats=True), want)
        same(device_search(hix, sp, queries=q), want)
        same(hix.search_batch_filtered(queries=q, sp=sp, allow=np.ones(N, dtype=bool), stats=True), plain)  # an explicit filter wins
        same(hix.search_batch(queries=q, sp=sp, stats=True), plain)  # the existing entry points never see it
        ids, d, ln = hix.search_batch(queries=q, sp=sp, k=10)
        same((ids, d, ln), (plain[0][:, :10], plain[1][:, :10], np.minimum(plain[2], 10)))
    finally:
        hix.set_filter(0)
    same(hix.search_batch_filtered(queries=q, sp=sp, stats=True), plain)


# ---------------------------------------------------------------- 9: two filtered batches in flight
def test_two_filtered_batches_on_two_streams():
    import torch
    hix = world("f32", 100)[0]
    sp = ph.SearchParameters(64, 64, 2)
    dev = torch.device("cuda", 0)
    s1 = ph.stream_create_beside(0, 0)
    nq, ld = 1500, hix.store.ld
    lanes = []
    for k, st in enumerate((0, s1)):
        q = np.ascontiguousarray(oracle.synth_rows(2 ** 32 + 7919 * k, nq, 100)[:, :100])
        allow = mask(0.4, (nq, N), 31 + k)
        qp = np.zeros((nq, ld), dtype=np.float32)
        qp[:, :100] = q
        lanes.append(dict(q=q, allow=allow, stream=st, qd=torch.from_numpy(qp).to(dev),
                          w=torch.from_numpy(fr.pack(allow).view(np.int32)).to(dev),
                          ids=torch.empty((nq, 64), dtype=torch.int32, device=dev), d=torch.empty((nq, 64), dtype=torch.float32, device=dev),
                          ln=torch.empty(nq, dtype=torch.int32, device=dev), status=torch.empty(nq, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    for i in range(6):
        a = lanes[i & 1]
        hix.search_batch_filtered_device(nq, sp, a["ids"].data_ptr(), a["d"].data_ptr(), a["ln"].data_ptr(), a["status"].data_ptr(),
                                         queries=a["qd"].data_ptr(), ldq=ld, allow=a["w"].data_ptr(), allow_stride=(N + 31) // 32,
                                         stream=a["stream"])
    torch.cuda.synchronize()
    for a in lanes:
        alone = hix.search_batch_filtered(queries=a["q"], sp=sp, allow=a["allow"])
        assert int(a["status"].abs().sum()) == 0
        ids = a["ids"].cpu().numpy().view(np.uint32).astype(np.uint64)
        ids[ids == 0xFFFFFFFF] = EMPTY
        same((ids, a["d"].cpu().numpy(), a["ln"].cpu().numpy().astype(np.uint64)), alone)


# ---------------------------------------------------------------- 10: argument checks and the k cut
def test_argument_checks_and_the_k_cut():
    hix = world("f32", 100)[0]
    sp = ph.SearchParameters(64, 64, 2)
    q = raw_queries("f32", 100, 20)
    allow = mask(0.5, (20, N), 3)
    full = hix.search_batch_filtered(queries=q, sp=sp, allow=allow)
    ids, d, ln = hix.search_batch_filtered(queries=q, sp=sp, allow=allow, k=7)
    assert ids.shape == (20, 7)
    same((ids, d, ln), (full[0][:, :7], full[1][:, :7], np.minimum(full[2], 7)))
    strict7 = hix.search_batch_filtered(queries=q, sp=sp, allow=allow, k=7, strict=True)
    sfull = hix.search_batch_filtered(queries=q, sp=sp, allow=allow, strict=True)
    same(strict7, (sfull[0][:, :7], sfull[1][:, :7], np.minimum(sfull[2], 7)))
    words = fr.pack(allow)
    nw = words.shape[1]
    out = (np.empty((20, 64), dtype=np.uint64), np.empty((20, 64), dtype=np.float32), np.zeros(20, dtype=np.uint64))

    def call(stride, flags, k, w=words):
        return lib().phnsw_search_batch_filtered(hix._h, _p(q), None, 20, C.byref(sp), 0, None, _p(w), stride, flags, k, _p(out[0]),
                                                 _p(out[1]), _p(out[2]), None)

    assert call(nw, 0, 0) == 0
    same(out, full)
    assert call(nw - 1, 0, 0) == E_INVALID      # a stride below ceil(n / 32) that is not 0
    assert call(nw, 2, 0) == E_INVALID          # unknown flag bits
    assert call(nw, 0, 65) == E_INVALID         # k > number_of_candidates
    wide = np.zeros((20, nw + 3), dtype=np.uint32)
    wide[:, :nw] = words
    wide[:, nw:] = 0xFFFFFFFF                   # words past the bitmap (and, below, bits at or past n) are ignored
    assert call(nw + 3, 0, 0, wide) == 0
    same(out, full)
    tail = words.copy()
    tail[:, -1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    assert call(nw, 0, 0, tail) == 0
    same(out, full)
    with pytest.raises(ph.PhnswError) as e:
        hix.search_batch_filtered_device(20, sp, 8, 8, 8, 8, queries=0, qids=8, allow=8, allow_stride=nw - 1)
    assert e.value.code == E_INVALID
