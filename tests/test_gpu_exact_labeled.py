"""The exact top-k by row label (phnsw_labels_*, phnsw_search_exact_labeled[_device], filter_labeled.hip): posting lists
instead of bitmaps.  Every comparison is on ids, distance bits, lengths and status, no tolerance anywhere.

Two yardsticks, both for every case: tests/exact_filter_reference.py over the oracle's ORC_SUM_BLOCKED64 distances
(compare_vec on the PQ store) with the bitmaps labeled_reference.masks_of makes of the label column, which the code under
test did not make, and the existing scan, search_exact_filtered with those masks as per-query bitmaps, whose rows the new
call promises bit for bit.

The worlds are those of tests/test_gpu_exact_shared.py (N = 5000, 40 copies of row 0 spread over the id range, 65 raw and
65 stored queries, one-layer ring indexes).  The label column is constructed, not drawn: all 40 copies and 2100 other
rows carry BIG (a list longer than 2048: 34 batches, so the 40 ties cross batch and slice borders), labels of exactly 1,
64 and 65 rows, two labels with large values, 100 rows without a label, five labels over the rest, and one label that is
wanted and absent."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import exact_filter_reference as xr
import labeled_reference as lr
from test_gpu_exact_filter import COS, DUPS, EMPTY, N, ring, same, stores
from test_gpu_exact_shared import NQX, fetch, sworld
from test_gpu_i8 import bits
from test_gpu_i8q import env

pytestmark = pytest.mark.gpu

NONE = lr.LABEL_NONE
BIG, ONE, L64, L65, HALF, TOP, ABSENT = 7, 11, 12, 13, 0x7FFFFFFF, 0xFFFFFFFE, 999
REST = (5, 1000, 2000, 3000, 70000)
KINDS = [(k, d) for k in ("f32", "f16", "i8", "i8q") for d in (24, 256)] + [("f32", 768), ("i8q", 768), ("f32", 1536), ("pq", 24)]


@functools.lru_cache(maxsize=None)
def column():
    """the label of every vector, u32 [N]"""
    lab = np.full(N, NONE, dtype=np.uint32)
    others = np.random.default_rng(2024).permutation(np.setdiff1d(np.arange(N), DUPS))
    lab[DUPS] = BIG
    at = 0
    for value, count in ((BIG, 2100), (ONE, 1), (L64, 64), (L65, 65), (HALF, 150), (TOP, 150), (NONE, 100)):
        lab[others[at:at + count]] = value
        at += count
    rest = others[at:]
    for i, value in enumerate(REST):
        lab[rest[i::5]] = value
    assert (lab == BIG).sum() == 2140 and (lab == NONE).sum() == 100 and not (lab == ABSENT).any()
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def pq_world():
    """sworld's shape over the PQ store at 24: the yardstick is compare_vec, the distance batch"""
    store = stores("pq", 24)[1]
    from test_gpu_exact_filter import rows_of
    q = oracle.synth_rows(2 ** 33, NQX, 24)[:, :24].copy()
    q[0] = rows_of(False, 24)[0]
    qids = np.concatenate([[int(DUPS[3])], np.linspace(1, N - 1, NQX - 1).astype(np.int64)]).astype(np.uint64)
    every = np.arange(N, dtype=np.uint64)
    Dq = np.stack([store.compare_vec(ph.Unstored(np.ascontiguousarray(v)), every) for v in q])
    Ds = np.stack([store.compare_vec(ph.Stored(int(v)), every) for v in qids])
    return dict(store=store, hix=ph.Hnsw.from_layers(store, ring(np.arange(N))), q=q, qids=qids, Dq=Dq, Ds=Ds)


def world_of(kind, dim, metric=COS):
    if kind == "pq":
        return pq_world()
    return sworld(kind, dim) if metric == COS else sworld(kind, dim, metric)  # the cache keys on the call's form


@functools.lru_cache(maxsize=None)
def handle(kind, dim, metric=COS):
    return ph.Labels(world_of(kind, dim, metric)["hix"], column())


def cycle_want():
    """65 wanted labels: query 0 (the duplicated row) wants BIG, the others go round every label, the absent one and NONE"""
    values = [BIG, ONE, L64, L65, HALF, TOP, ABSENT, NONE] + list(REST)
    w = np.array([values[i % len(values)] for i in range(NQX)], dtype=np.int64)
    w[0] = BIG
    return w


def staged_labeled(hix, lb, k, want, queries=None, qids=None, exclude=None):
    """the inputs and outputs of one phnsw_search_exact_labeled_device call, uploaded; no synchronisation here.  Returns
    (launch, out): launch(stream) enqueues the call and nothing else, out is what fetch takes"""
    import torch
    dev = torch.device("cuda", 0)
    keep = []

    def up(a, dt):
        t = torch.from_numpy(np.ascontiguousarray(a).view(dt) if dt is not None else np.ascontiguousarray(a)).to(dev)
        keep.append(t)
        return t

    nq = len(queries) if queries is not None else len(qids)
    qd = qi = ex = ld = 0
    if queries is not None:
        ld = hix.store.ld
        qp = np.zeros((nq, ld), dtype=np.float32)
        qp[:, :queries.shape[1]] = queries
        qd = up(qp, None).data_ptr()
    else:
        qi = up(np.asarray(qids, dtype=np.uint32), np.int32).data_ptr()
    if exclude is not None:
        ex = up(np.asarray(exclude, dtype=np.uint32), np.int32).data_ptr()
    wd = up(ph.hnsw.pack_labels(want, nq, "want"), np.int32).data_ptr()
    ids = torch.full((nq, k), 7, dtype=torch.int32, device=dev)
    d = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev)
    ln = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    status = torch.full((nq,), -1, dtype=torch.int32, device=dev)

    def launch(stream=None):
        hix.search_exact_labeled_device(lb, nq, k, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd,
                                        ldq=ld, qids=qi, exclude=ex, want=wd, stream=0 if stream is None else stream.cuda_stream)

    return launch, (ids, d, ln, status, keep)


def device_labeled(hix, lb, k, want, queries=None, qids=None, exclude=None, stream=None, sync=True):
    """phnsw_search_exact_labeled_device with torch buffers -> ids u64, d, len u64, status (or the tensors, sync=False)"""
    import torch
    launch, out = staged_labeled(hix, lb, k, want, queries=queries, qids=qids, exclude=exclude)
    torch.cuda.synchronize()
    launch(stream)
    return fetch(out) if sync else out


def check(w, lb, want, nq=NQX, exclude=None, k=10, members=None, hix=None, device=True, forms=(0, 1), scan=True, labels=None):
    """raw (0) and stored (1) queries, host and device form, against both yardsticks -> the host results by form"""
    hix = hix or w["hix"]
    want = np.asarray(want)[:nq]
    allow = lr.masks_of(column() if labels is None else labels, want)
    out = {}
    for form in forms:
        kw, D = (dict(queries=w["q"][:nq]), w["Dq"][:nq]) if form == 0 else (dict(qids=w["qids"][:nq]), w["Ds"][:nq])
        e = None if exclude is None else exclude[:nq]
        ref = xr.exact_topk(D, allow, e, members, k)
        got = hix.search_exact_labeled(labels=lb, want=want, exclude=e, k=k, **kw)
        same(got, ref)
        if scan:
            same(got, hix.search_exact_filtered(allow=allow, exclude=e, k=k, **kw))
        assert (got[0][np.arange(k)[None, :] >= got[2][:, None]] == EMPTY).all()
        assert (bits(got[1])[np.arange(k)[None, :] >= got[2][:, None]] == bits(xr.FMAX)).all()
        if device:
            dv = device_labeled(hix, lb, k, want, exclude=e, **kw)
            assert not dv[3].any()
            same(dv, ref)
        out[form] = got
    return out


# ---------------------------------------------------------------- the handle
def test_the_handle_describes_the_lists():
    lb = handle("f32", 24)
    lab = column()
    values, counts = np.unique(lab[lab != NONE], return_counts=True)
    assert lb.info() == (N, len(values), N - 100, 2140)
    assert (lb.nlabels, lb.listed, lb.longest) == (len(values), N - 100, 2140)
    want = np.concatenate([values, [ABSENT, NONE, 0, 0xFFFFFFFD]])
    np.testing.assert_array_equal(lb.count(want), np.concatenate([counts, [0, 0, 0, 0]]))
    np.testing.assert_array_equal(lb.count(want), w_filter_count("f32", 24, want))
    assert lb.count(np.array([ONE, L64, L65])).tolist() == [1, 64, 65]


def w_filter_count(kind, dim, want, hix=None, labels=None):
    hix = hix or world_of(kind, dim)["hix"]
    return hix.filter_count(lr.masks_of(column() if labels is None else labels, want))


def test_a_handle_from_device_labels_gives_the_same_rows():
    import torch
    w = sworld("f32", 24)
    t = torch.from_numpy(column().copy().view(np.int32)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    lb = ph.Labels.from_device(w["hix"], t.data_ptr())
    assert lb.info() == handle("f32", 24).info()
    check(w, lb, cycle_want(), k=10)
    lb.close()
    lb.close()  # twice: a no-op


# ---------------------------------------------------------------- 1: kinds x dimensions, k, exclude
@pytest.mark.parametrize("kind,dim", KINDS)
def test_kinds_and_dimensions(kind, dim):
    w, lb, want = world_of(kind, dim), handle(kind, dim), cycle_want()
    got = check(w, lb, want, k=10)
    if kind not in ("i8q", "pq"):  # normalised rows: nothing is nearer to a row than its copies
        for form in (0, 1):  # query 0 is the duplicated row, stored query 0 one of its copies: the copies tie, ids decide
            np.testing.assert_array_equal(got[form][0][0], DUPS[:10].astype(np.uint64))
    check(w, lb, want, k=1, device=False)
    first = check(w, lb, want, k=64)
    lab = column()
    for form in (0, 1):
        best = first[form][0][:, 0]  # each query's best hit, where it has one: inside its list, and it matters
        inside = np.where(best == EMPTY, np.uint64(5), best)
        got = check(w, lb, want, exclude=inside, k=64, forms=(form,))[form]
        has = best != EMPTY
        assert not (got[0][has] == best[has, None]).any()
        np.testing.assert_array_equal(got[2][has], np.minimum(64, lr.masks_of(lab, want).sum(1)[has] - 1))
    # an exclude outside the list (a vector of another label, an unlabeled one, an id past n, PHNSW_EMPTY) changes nothing
    outside = np.full(NQX, EMPTY, dtype=np.uint64)
    outside[0::4] = int(np.nonzero(lab == L64)[0][0])
    outside[1::4] = int(np.nonzero(lab == NONE)[0][0])
    outside[2::4] = N + 7
    outside[np.asarray(want) == L64] = EMPTY
    got = check(w, lb, want, exclude=outside, k=64, device=False)
    for form in (0, 1):
        same(got[form], first[form])


def test_k_1024_returns_whole_lists_with_their_ties():
    w, lb = sworld("f32", 256), handle("f32", 256)
    got = check(w, lb, cycle_want(), k=1024)
    counts = lr.masks_of(column(), cycle_want()).sum(1)
    for form in (0, 1):
        np.testing.assert_array_equal(got[form][2], np.minimum(counts, 1024))
        np.testing.assert_array_equal(got[form][0][0, :40], DUPS.astype(np.uint64))
        assert len(set(bits(got[form][1][0, :40]).tolist())) == 1


@pytest.mark.parametrize("metric", [oracle.METRIC_L2, oracle.METRIC_ONE_MINUS_DOT])
def test_the_other_metrics(metric):
    check(world_of("f32", 24, metric), handle("f32", 24, metric), cycle_want(), k=64)


# ---------------------------------------------------------------- 2: tiles and slices
def grouped_want():
    """labels wanted by 1, 3, 4 and 7 queries, the rest BIG; spread over the batch, not adjacent"""
    w = np.full(NQX, BIG, dtype=np.int64)
    spots = np.random.default_rng(5).permutation(np.arange(1, NQX))
    w[spots[0:1]], w[spots[1:4]], w[spots[4:8]], w[spots[8:15]] = L65, HALF, TOP, REST[4]
    return w


@pytest.mark.parametrize("kind,dim", [("f32", 256), ("f16", 24), ("i8", 256), ("f32", 768), ("i8q", 256)])
def test_rows_do_not_depend_on_tiles_and_slices(monkeypatch, kind, dim):
    w, lb = world_of(kind, dim), handle(kind, dim)
    wants = (grouped_want(), np.full(NQX, BIG, dtype=np.int64))
    base = [check(w, lb, want, k=100) for want in wants]
    for tile in ("1", "3", None):
        for slices in ("1", "3", "7"):
            kw = dict(PHNSW_LABEL_SLICES=slices)
            if tile:
                kw["PHNSW_LABEL_TILE"] = tile
            with env(monkeypatch, **kw):
                for want, b in zip(wants, base):
                    now = check(w, lb, want, k=100, scan=False, device=slices == "3")
                    for form in (0, 1):
                        same(now[form], b[form])


# ---------------------------------------------------------------- 3: empty and odd rows
@pytest.mark.parametrize("kind,dim", [("f32", 256), ("i8q", 24), ("pq", 24)])
def test_empty_rows_and_k_larger_than_a_list(kind, dim):
    w, lb = world_of(kind, dim), handle(kind, dim)
    for value in (NONE, -1, ABSENT):
        got = check(w, lb, np.full(NQX, value, dtype=np.int64), nq=16, k=10)
        assert not got[0][2].any() and not got[1][2].any()
    want = np.array([ONE, L64, L65, ABSENT] * 4)
    got = check(w, lb, want, nq=16, k=100)
    for form in (0, 1):
        assert got[form][2].tolist() == [1, 64, 65, 0] * 4


@pytest.mark.parametrize("kind,dim", [("f32", 256), ("f32", 24), ("i8q", 256)])
def test_a_stored_query_id_past_n_is_reported_and_harms_nobody(monkeypatch, kind, dim):
    w, lb = world_of(kind, dim), handle(kind, dim)
    want = grouped_want()[:40]
    qids = w["qids"][:40].copy()
    bad = [3, 17, 39]
    qids[bad] = [N, N + 12345, 0xFFFFFFFE]
    ref = xr.exact_topk(w["Ds"][:40], lr.masks_of(column(), want), None, None, 10)
    good = np.setdiff1d(np.arange(40), bad)
    for kw in (dict(), dict(PHNSW_LABEL_TILE="1"), dict(PHNSW_LABEL_SLICES="3")):
        with env(monkeypatch, **kw):
            dv = device_labeled(w["hix"], lb, 10, want, qids=qids)
        same(tuple(x[good] for x in dv[:3]), tuple(x[good] for x in ref))
        assert (dv[3][bad] == 4).all() and not dv[3][good].any()
        assert (dv[0][bad] == EMPTY).all() and (bits(dv[1][bad]) == bits(xr.FMAX)).all() and not dv[2][bad].any()
    with pytest.raises(ph.PhnswError) as e:  # the host form refuses such an id, as the other exact calls do
        w["hix"].search_exact_labeled(qids=qids, labels=lb, want=want, k=10)
    assert e.value.code == -1 and "phnsw_search_exact_labeled:" in str(e.value) and "out of range" in str(e.value)


# ---------------------------------------------------------------- 4: an index over part of its store
@pytest.mark.parametrize("kind,dim", [("f32", 24), ("f32", 256), ("i8q", 256)])
def test_vectors_outside_the_index_are_never_listed(kind, dim):
    w = world_of(kind, dim)
    even = np.arange(N) % 2 == 0
    hix = ph.Hnsw.from_layers(w["store"], ring(np.arange(0, N, 2)))  # every second vector: vec2node is not the identity
    lb = ph.Labels(hix, column())
    lab = column()
    listed = even & (lab != NONE)
    values, counts = np.unique(lab[listed], return_counts=True)
    assert lb.info() == (N, len(values), listed.sum(), counts.max())
    want = cycle_want()
    np.testing.assert_array_equal(lb.count(want), hix.filter_count(lr.masks_of(lab, want)))
    np.testing.assert_array_equal(lb.count(want), (lr.masks_of(lab, want) & even).sum(1))
    got = check(w, lb, want, members=even, hix=hix, k=100)
    for form in (0, 1):
        assert not (got[form][0][got[form][0] != EMPTY] % 2).any()
    head = np.arange(N) < N - 100
    hix2 = ph.Hnsw.from_layers(w["store"], ring(np.arange(N - 100)))  # the first N - 100: identity, shorter than the store
    lb2 = ph.Labels(hix2, column())
    assert lb2.listed == (head & (lab != NONE)).sum()
    got = check(w, lb2, want, members=head, hix=hix2, k=1024, device=False)
    assert (got[0][0][got[0][0] != EMPTY] < N - 100).all()


# ---------------------------------------------------------------- 5: refusals
def test_refusals():
    w, lb = sworld("f32", 24), handle("f32", 24)
    hix, q, want = w["hix"], w["q"][:4], np.array([BIG, ONE, ABSENT, NONE])
    for k in (0, 1025):
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_labeled(queries=q, labels=lb, want=want, k=k)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_labeled: k must be 1..1024 (got %d)" % k
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_labeled_device(lb, 4, k, 8, 8, 8, 8, qids=8, want=8)
        assert str(e.value) == "phnsw error -1: phnsw_search_exact_labeled_device: k must be 1..1024 (got %d)" % k
    # a handle made for another index over the same store
    other = ph.Hnsw.from_layers(w["store"], ring(np.arange(N)))
    for call in (lambda: other.search_exact_labeled(queries=q, labels=lb, want=want, k=3),
                 lambda: other.search_exact_labeled_device(lb, 4, 3, 8, 8, 8, 8, qids=8, want=8)):
        with pytest.raises(ph.PhnswError) as e:
            call()
        assert e.value.code == -1 and "the labels are stale" in str(e.value) and "phnsw_search_exact_labeled" in str(e.value)
    # the handle is looked at before the other arguments, k before the handle
    with pytest.raises(ph.PhnswError) as e:
        other.search_exact_labeled_device(lb, 4, 0, 8, 8, 8, 8, qids=8, want=8)
    assert "k must be" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:
        other.search_exact_labeled_device(lb, 4, 3, 8, 8, 8, 8)
    assert "stale" in str(e.value)
    for bad in (dict(queries=16, ldq=24, qids=8, want=8), dict(want=8), dict(qids=8)):  # both, neither, no want
        with pytest.raises(ph.PhnswError) as e:
            hix.search_exact_labeled_device(lb, 4, 3, 8, 8, 8, 8, **bad)
        assert e.value.code == -1 and "phnsw_search_exact_labeled_device: invalid argument" in str(e.value)
    ids, d, ln = hix.search_exact_labeled(queries=np.zeros((0, 24), dtype=np.float32), labels=lb, want=np.zeros(0, dtype=np.int64), k=3)
    assert ids.shape == (0, 3)  # nq == 0: a no-op
    # n not the store's
    import ctypes as C
    out = C.c_void_p()
    col = column()
    assert ph.lib().phnsw_labels_create(hix._h, col.ctypes.data_as(C.c_void_p), N - 1, C.byref(out)) == -1
    msg = ph.lib().phnsw_last_error().decode()
    assert msg.startswith("phnsw_labels_create: %d labels for a store of %d vectors" % (N - 1, N)) and not out.value
    # a shared-codebook PQ store: unsupported, as for the scan; the handle itself can be made
    rows = oracle.synth_rows(0, 400, 32)[:, :32].copy()
    f2 = ph.VectorStore(rows, metric=ph.METRIC_L2)
    shared = ph.SharedPqStore(f2, 16, 100, seed=3, centroid_bp=ph.BuildParameters(seed=2),
                              quantized_search=ph.SearchParameters(32, 32, 2))
    pix = ph.Hnsw.from_layers(shared, ring(np.arange(400)))
    plb = ph.Labels(pix, np.arange(400) % 3)
    with pytest.raises(ph.PhnswError) as e:
        pix.search_exact_labeled(queries=rows[:2], labels=plb, want=np.array([0, 1]), k=3)
    assert e.value.code == -7 and "phnsw_search_exact_labeled:" in str(e.value)


def test_a_handle_is_stale_after_the_store_has_grown():
    rows = oracle.synth_rows(0, 300, 24)[:, :24].copy()
    store = ph.VectorStore(rows[:200], metric=COS)
    hix = ph.Hnsw.from_layers(store, ring(np.arange(200)))
    lab = np.arange(200) % 4
    lb = ph.Labels(hix, lab)
    got = hix.search_exact_labeled(queries=rows[:3], labels=lb, want=np.array([0, 1, 2]), k=5)
    same(got, hix.search_exact_filtered(queries=rows[:3], allow=lr.masks_of(lab, np.array([0, 1, 2])), k=5))
    store.append(rows[200:])
    with pytest.raises(ph.PhnswError) as e:
        hix.search_exact_labeled(queries=rows[:3], labels=lb, want=np.array([0, 1, 2]), k=5)
    assert e.value.code == -1 and "the labels are stale" in str(e.value)
    lab2 = np.concatenate([lab, np.full(100, 1)])
    lb2 = ph.Labels(hix, lab2)  # a new handle: the appended vectors are not in the index, so they are not listed
    assert lb2.listed == 200
    got = hix.search_exact_labeled(queries=rows[:3], labels=lb2, want=np.array([0, 1, 2]), k=5)
    same(got, hix.search_exact_filtered(queries=rows[:3], allow=lr.masks_of(lab2, np.array([0, 1, 2])), k=5))


# ---------------------------------------------------------------- 6: calls in flight
def test_calls_in_flight_on_several_streams_with_no_synchronisation_between_them(monkeypatch):
    """Everything is uploaded first and the device is synchronised ONCE; then 24 calls are enqueued back to back on six
    streams (more than the four scratch sets a handle makes before calls share one) and on the default stream, with
    nothing between them that waits; only then are the rows fetched.  The calls differ in want, form, k, batch size and
    slice count, small ones before large ones on the same stream, so a set is handed on while its last call may still
    run, its blocks grow behind unfinished work, and a call that read another's scratch would return another's rows."""
    import torch
    w = sworld("f32", 256)
    lb = ph.Labels(w["hix"], column())  # a handle of its own: no scratch set exists yet
    shapes = [(grouped_want(), 0, 16, 10, None), (cycle_want(), 1, 65, 100, "7"), (np.full(NQX, BIG), 0, 65, 64, "3"),
              (cycle_want(), 0, 40, 1, None), (grouped_want(), 1, 65, 1024, "3"), (np.full(NQX, BIG), 1, 33, 10, "1")]

    def kwargs(form, nq):
        return dict(queries=w["q"][:nq]) if form == 0 else dict(qids=w["qids"][:nq])

    expect = [xr.exact_topk((w["Dq"], w["Ds"])[form][:nq], lr.masks_of(column(), want[:nq]), None, None, k)
              for want, form, nq, k, _ in shapes]
    streams = [torch.cuda.Stream() for _ in range(6)] + [None]
    plan = []  # (shape, stream) of the 24 calls: every stream sees small and large calls, neighbours differ
    for r in range(4):
        for j in range(6):
            plan.append(((j + r) % 6, streams[(j * (r + 1) + r) % 7]))
    staged = [staged_labeled(w["hix"], lb, shapes[i][3], shapes[i][0][:shapes[i][2]], **kwargs(shapes[i][1], shapes[i][2]))
              for i, _ in plan]
    torch.cuda.synchronize()  # the one synchronisation: inputs and outputs are there
    for (i, stream), (launch, _) in zip(plan, staged):
        slices = shapes[i][4]
        with env(monkeypatch, **({} if slices is None else {"PHNSW_LABEL_SLICES": slices})):
            launch(stream)  # enqueues and returns; nothing waits for the device
    for (i, _), (_, out) in zip(plan, staged):
        got = fetch(out)
        assert not got[3].any()
        same(got, expect[i])
    lb.close()


# ---------------------------------------------------------------- 7: value edges
VALUE_WORLDS = [("lattice", 2, 256, "f32"), ("l2_overflow", 2, 768, "f32"), ("tiny", 0, 100, "f16")]


@pytest.mark.parametrize("key", VALUE_WORLDS, ids=lambda k: "%s-m%d-d%d-%s" % k)
def test_value_edges_against_the_scan(monkeypatch, key):
    """ties (lattice under L2), infinite distances (l2_overflow) and one tie over everything (tiny): the rows of
    search_exact_filtered for the equivalent bitmaps, and of the restatement over yardstick 1"""
    import filter_value_worlds as fw
    from test_gpu_filter_value_edges import queries_of, ring_index
    w, hix = fw.world(*key), ring_index(key)
    lab = (np.arange(fw.N) % 3).astype(np.int64) * 1000  # three labels of 700 rows: eleven batches each
    lab[np.arange(0, fw.N, 50)] = -1
    lb = ph.Labels(hix, lab)
    for form in (0, 1):
        kw = queries_of(w, form)
        nq = len(next(iter(kw.values())))
        want = np.arange(nq) % 3 * 1000
        allow = lr.masks_of(lab, want)
        for k in (10, 1024):
            ref = hix.search_exact_filtered(allow=allow, k=k, **kw)
            same(ref, xr.exact_topk((w["Dq"], w["Ds"])[form][:nq], allow, None, None, k))
            for env_kw in (dict(), dict(PHNSW_LABEL_TILE="1"), dict(PHNSW_LABEL_SLICES="3")):
                with env(monkeypatch, **env_kw):
                    same(hix.search_exact_labeled(labels=lb, want=want, k=k, **kw), ref)
