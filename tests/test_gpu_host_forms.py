"""The unpipelined host form of the filtered and exact calls (csrc/host_call.h), every one of them beside its device form:
phnsw_search_exact_shared, _exact_grouped, _exact_labeled, _exact_labelset, _batch_labeled, _filtered_auto and
_labeled_auto.  The host form pads the query rows, lays the per-query words into one block, runs the call on a scratch
set's stream, takes the leading k of every row and widens ids and lengths; the device form gets queries this file padded
itself, u32 words it narrowed itself, and returns u32 rows.  Ids (PHNSW_EMPTY padded), distance bits, lengths, routes
and stats must be equal; the device forms are pinned to the references by the files of the calls themselves.

The world is the smallest at which the staging can go wrong: 300 f32 rows under a ring index, rows of 6 floats (24 bytes,
padded to 8) and of 8 (not padded), 5 queries -- odd and more than one, so a wrong [x][nq] offset lands in a neighbour's
words -- and k = 3."""
import functools
import threading

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import labeled_reference as lr
from test_gpu_exact_filter import COS, EMPTY, ring, same

pytestmark = pytest.mark.gpu

N, NQ, K, EF = 300, 5, 3, 16
DIMS = (6, 8)
NONE = lr.LABEL_NONE
LABELS = (5, 1000, 70000)
WANT = np.array([5, 1000, 70000, NONE, 5], dtype=np.int64)
WANT_SETS = [[5, 1000], [70000], [], [1000, 1000, 5], [NONE, 70000]]
ALLOW_OF = np.array([0, 1, -1, 1, 0], dtype=np.int64)  # -1: no bitmap
NO_EXCLUDE32 = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def world(dim):
    """made once per row length, changed by no test"""
    rows = oracle.synth_rows(0, N, dim)[:, :dim].copy()
    store = ph.VectorStore(rows, metric=COS)
    assert store.ld == 8 and store.dim == dim
    hix = ph.Hnsw.from_layers(store, ring(np.arange(N)))
    rng = np.random.default_rng(77 + dim)
    lab = np.array([LABELS[i % 3] for i in range(N)], dtype=np.int64)
    lab[np.arange(4, N, 10)] = -1  # some rows without a label
    allow = rng.random(N) < 0.4
    table = rng.random((2, N)) < 0.4
    q = oracle.synth_rows(2 ** 33, NQ, dim)[:, :dim].copy()
    qids = np.array([0, 7, 150, 298, 299], dtype=np.uint64)
    return dict(store=store, hix=hix, lab=lab, lb=ph.Labels(hix, lab), allow=allow, table=table, q=q, qids=qids)


def device_form(w, form, exclude32, row, call, **words):
    """One device call with torch buffers.  form 0: raw queries, padded to ld HERE; form 1: stored ids as u32.  words: u32
    arrays the call takes besides.  call(p) gets the device pointers by name (queries, ldq, qids, exclude, ids, d, len,
    status, route, stats and the words).  Returns ids u64 [NQ, row], d, len u64, status, route, stats u64 [NQ, 2]"""
    import torch
    dev = torch.device("cuda", 0)
    keep = {}

    def up(name, a):
        keep[name] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return keep[name].data_ptr()

    p = dict(queries=0, ldq=0, qids=0, exclude=0)
    if form == 0:
        ld = w["store"].ld
        qp = np.zeros((NQ, ld), dtype=np.float32)
        qp[:, :w["q"].shape[1]] = w["q"]
        p["queries"], p["ldq"] = up("queries", qp), ld
    else:
        p["qids"] = up("qids", w["qids"].astype(np.uint32).view(np.int32))
    if exclude32 is not None:
        p["exclude"] = up("exclude", np.asarray(exclude32, dtype=np.uint32).view(np.int32))
    for name, a in words.items():
        p[name] = up(name, np.asarray(a, dtype=np.uint32).view(np.int32)) if len(a) else 0
    ids = torch.full((NQ, row), 7, dtype=torch.int32, device=dev)
    d = torch.full((NQ, row), -1.0, dtype=torch.float32, device=dev)
    ln, status, route = (torch.full((NQ,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    stats = torch.full((NQ, 2), -1, dtype=torch.int32, device=dev)
    p.update(ids=ids.data_ptr(), d=d.data_ptr(), len=ln.data_ptr(), status=status.data_ptr(), route=route.data_ptr(),
             stats=stats.data_ptr())
    torch.cuda.synchronize()
    call(p)
    torch.cuda.synchronize()

    def u64(t):
        return t.cpu().numpy().view(np.uint32).astype(np.uint64)

    i64 = u64(ids)
    i64[i64 == 0xFFFFFFFF] = EMPTY
    return i64, d.cpu().numpy(), u64(ln), status.cpu().numpy(), route.cpu().numpy().view(np.uint32), u64(stats)


def queries_of(w, form):
    return dict(queries=w["q"]) if form == 0 else dict(qids=w["qids"])


# ---------------------------------------------------------------- the seven calls: (host, device) by name
# host(w, form, exclude u64 or None) -> what the host form returns; device(w, form, exclude u32 or None) -> device_form's
SP = ph.SearchParameters(EF, EF, 2)


def shared_host(w, form, e):
    return w["hix"].search_exact_shared(allow=w["allow"], exclude=e, k=K, **queries_of(w, form))


def shared_device(w, form, e):
    words, stride = ph.hnsw.pack_allow(w["allow"], N, NQ)
    assert stride == 0
    return device_form(w, form, e, K, lambda p: w["hix"].search_exact_shared_device(
        NQ, K, p["ids"], p["d"], p["len"], p["status"], queries=p["queries"], ldq=p["ldq"], qids=p["qids"],
        exclude=p["exclude"], allow=p["allow"]), allow=words)


def grouped_host(w, form, e):
    return w["hix"].search_exact_grouped(allows=w["table"], allow_of=ALLOW_OF, exclude=e, k=K, **queries_of(w, form))


def grouped_device(w, form, e):
    words, stride = ph.hnsw.pack_allow_table(w["table"], N)
    return device_form(w, form, e, K, lambda p: w["hix"].search_exact_grouped_device(
        NQ, K, p["ids"], p["d"], p["len"], p["status"], queries=p["queries"], ldq=p["ldq"], qids=p["qids"],
        exclude=p["exclude"], allows=p["allows"], allow_stride=stride, nallows=2, allow_of=p["allow_of"]),
        allows=words.reshape(-1), allow_of=ph.hnsw.pack_allow_of(ALLOW_OF, NQ))


def labeled_host(w, form, e):
    return w["hix"].search_exact_labeled(labels=w["lb"], want=WANT, exclude=e, k=K, **queries_of(w, form))


def labeled_device(w, form, e):
    return device_form(w, form, e, K, lambda p: w["hix"].search_exact_labeled_device(
        w["lb"], NQ, K, p["ids"], p["d"], p["len"], p["status"], queries=p["queries"], ldq=p["ldq"], qids=p["qids"],
        exclude=p["exclude"], want=p["want"]), want=ph.hnsw.pack_labels(WANT, NQ, "want"))


def labelset_host(w, form, e):
    return w["hix"].search_exact_labelset(labels=w["lb"], want=WANT_SETS, exclude=e, k=K, **queries_of(w, form))


def labelset_device(w, form, e):
    first, values = ph.hnsw.pack_label_sets(WANT_SETS, NQ)
    return device_form(w, form, e, K, lambda p: w["hix"].search_exact_labelset_device(
        w["lb"], NQ, len(values), K, p["ids"], p["d"], p["len"], p["status"], queries=p["queries"], ldq=p["ldq"],
        qids=p["qids"], exclude=p["exclude"], want_first=p["want_first"], want_values=p["want_values"]),
        want_first=first, want_values=values)


def walk_host(w, form, e, k=K):
    return w["hix"].search_batch_labeled(sp=SP, labels=w["lb"], want=WANT, exclude=e, stats=True, k=k, **queries_of(w, form))


def walk_device(w, form, e, k=K):
    """the device form returns the whole queue: the host form's take is the leading k of it"""
    i64, d, ln, st, _, stats = device_form(w, form, e, EF, lambda p: w["hix"].search_batch_labeled_device(
        w["lb"], NQ, SP, p["ids"], p["d"], p["len"], p["status"], queries=p["queries"], ldq=p["ldq"], qids=p["qids"],
        exclude=p["exclude"], want=p["want"], out_stats=p["stats"]), want=ph.hnsw.pack_labels(WANT, NQ, "want"))
    k = EF if k is None else k
    return i64[:, :k], d[:, :k], np.minimum(ln, k), st, None, stats


def auto_host(w, form, e, scan_below=0):
    return w["hix"].search_filtered(sp=SP, allow=w["allow"], exclude=e, k=K, scan_below=scan_below, route=True,
                                    **queries_of(w, form))


def auto_device(w, form, e, scan_below=0):
    words, stride = ph.hnsw.pack_allow(w["allow"], N, NQ)
    return device_form(w, form, e, K, lambda p: w["hix"].search_filtered_device(
        NQ, SP, K, p["ids"], p["d"], p["len"], p["status"], queries=p["queries"], ldq=p["ldq"], qids=p["qids"],
        exclude=p["exclude"], allow=p["allow"], allow_stride=stride, scan_below=scan_below, out_route=p["route"]),
        allow=words)


def labeled_auto_host(w, form, e, scan_below=0):
    return w["hix"].search_labeled(sp=SP, labels=w["lb"], want=WANT, exclude=e, k=K, scan_below=scan_below, route=True,
                                   **queries_of(w, form))


def labeled_auto_device(w, form, e, scan_below=0):
    return device_form(w, form, e, K, lambda p: w["hix"].search_labeled_device(
        w["lb"], NQ, SP, K, p["ids"], p["d"], p["len"], p["status"], queries=p["queries"], ldq=p["ldq"], qids=p["qids"],
        exclude=p["exclude"], want=p["want"], scan_below=scan_below, out_route=p["route"]),
        want=ph.hnsw.pack_labels(WANT, NQ, "want"))


def graph_first(fn):
    """the routed calls with a threshold of one candidate: the rule sends these shapes to the walk first"""
    return functools.partial(fn, scan_below=1)


# name -> (host, device, the fourth value a host form returns: None, "route" or "stats")
CALLS = {
    "exact_shared": (shared_host, shared_device, None),
    "exact_grouped": (grouped_host, grouped_device, None),
    "exact_labeled": (labeled_host, labeled_device, None),
    "exact_labelset": (labelset_host, labelset_device, None),
    "batch_labeled": (walk_host, walk_device, "stats"),
    "batch_labeled_whole_queue": (functools.partial(walk_host, k=None), functools.partial(walk_device, k=None), "stats"),
    "filtered_auto": (auto_host, auto_device, "route"),
    "filtered_auto_graph_first": (graph_first(auto_host), graph_first(auto_device), "route"),
    "labeled_auto": (labeled_auto_host, labeled_auto_device, "route"),
    "labeled_auto_graph_first": (graph_first(labeled_auto_host), graph_first(labeled_auto_device), "route"),
}


def equal(got, dv, extra):
    assert not dv[3].any()  # every device status is 0
    same(got, dv)
    if extra == "route":
        np.testing.assert_array_equal(got[3], dv[4])
    if extra == "stats":
        np.testing.assert_array_equal(got[3], dv[5])
    pad = np.arange(got[0].shape[1])[None, :] >= got[2][:, None]
    assert (got[0][pad] == EMPTY).all()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("name", list(CALLS))
def test_a_host_form_returns_its_device_forms_rows(name, dim):
    w = world(dim)
    host, device, extra = CALLS[name]
    for form in (0, 1):
        plain = host(w, form, None)
        equal(plain, device(w, form, None), extra)
        assert plain[2].any()  # the comparison is about rows, not about nothing
        # exclude: one ordinary entry, query 0's best hit (so it matters), the others at n or past it -- "no exclude"
        # by the host rule; the device form is given 0xFFFFFFFF there
        # (the walk's second hit: its first is the entry vector, which both forms return whatever exclude says; what
        # exclude means to the walk is tests/test_gpu_labeled_walk.py's subject)
        at = 1 if extra == "stats" else 0
        best = int(plain[0][0, at]) if plain[0][0, at] != EMPTY else 1
        e64 = np.array([best, N, N + 7, 2 ** 40, EMPTY], dtype=np.uint64)
        e32 = np.array([best] + [NO_EXCLUDE32] * 4, dtype=np.uint32)
        got = host(w, form, e64)
        equal(got, device(w, form, e32), extra)
        if plain[0][0, at] != EMPTY:
            assert not (got[0][0] == best).any()
        same(tuple(x[1:] for x in got[:3]), tuple(x[1:] for x in plain[:3]))


def test_the_routed_calls_took_both_routes():
    """what the two thresholds above are for: the default scans these shapes, a threshold of one candidate walks first"""
    w = world(6)
    assert (auto_host(w, 0, None)[3] == ph.hnsw.ROUTE_SCAN).all()
    assert (graph_first(auto_host)(w, 0, None)[3] != ph.hnsw.ROUTE_SCAN).all()
    routes = graph_first(labeled_auto_host)(w, 0, None)[3]
    assert (routes != ph.hnsw.ROUTE_SCAN).any()


# ---------------------------------------------------------------- callers at once
def test_four_threads_call_two_host_forms_at_once():
    """the pool acquire and the guard under contention, on the padded rows: each thread has its own queries, wanted
    labels and exclude, and must get the rows it gets alone"""
    w = world(6)
    hix, lb = w["hix"], w["lb"]
    jobs = []
    for t in range(4):
        q = oracle.synth_rows(2 ** 34 + 100 * t, NQ + t, 6)[:, :6].copy()
        want = np.array([LABELS[(i + t) % 3] for i in range(NQ + t)], dtype=np.int64)
        e = np.arange(t, t + NQ + t, dtype=np.uint64)
        jobs.append((q, want, e))

    def labeled(t):
        q, want, e = jobs[t]
        return hix.search_exact_labeled(queries=q, labels=lb, want=want, exclude=e, k=K)

    def shared(t):
        q, _, e = jobs[t]
        return hix.search_exact_shared(queries=q, allow=w["allow"], exclude=e, k=K + t)

    alone = [(labeled(t), shared(t)) for t in range(4)]
    got, errs = [None] * 4, []

    def work(t):
        try:
            for _ in range(5):
                got[t] = (labeled(t), shared(t))
        except Exception as exc:  # noqa: BLE001
            errs.append(exc)

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errs, errs
    for t in range(4):
        same(got[t][0], alone[t][0])
        same(got[t][1], alone[t][1])


# ---------------------------------------------------------------- the walk's re-run
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("cap", ["1", "6"])
def test_the_walk_reruns_overflowed_queries_from_its_list_in_small(monkeypatch, dim, cap):
    """PHNSW_OVF_CAP forces a tiny spill list: at 6 entries some of the five walks overflow, at 1 all do and some again
    at the 8 of the first re-run.  The device form, which re-runs nothing, says so (status 5); the host form re-runs them
    from the redo list it keeps behind small's common words and returns the rows of the unforced run.  A workspace keeps
    the largest spill list it ever had, so every call that must overflow gets a new index and a handle made for it"""
    base = world(dim)

    def fresh():
        w = dict(base)
        w["hix"] = ph.Hnsw.from_layers(w["store"], ring(np.arange(N)))
        w["lb"] = ph.Labels(w["hix"], w["lab"])
        return w

    e64 = np.array([N, 7, EMPTY, 150, N + 1], dtype=np.uint64)
    e32 = np.array([NO_EXCLUDE32, 7, NO_EXCLUDE32, 150, NO_EXCLUDE32], dtype=np.uint32)
    for form in (0, 1):
        plain = walk_host(base, form, e64, k=None)
        monkeypatch.setenv("PHNSW_OVF_CAP", cap)
        status = walk_device(fresh(), form, e32, k=None)[3]
        assert (status == 5).any() and set(status.tolist()) <= {0, 5}  # the overflow really happens here
        got = walk_host(fresh(), form, e64, k=None)
        cut = walk_host(fresh(), form, e64)
        monkeypatch.delenv("PHNSW_OVF_CAP")
        same(got, plain)
        np.testing.assert_array_equal(got[3], plain[3])
        same(cut, (plain[0][:, :K], plain[1][:, :K], np.minimum(plain[2], K)))
        np.testing.assert_array_equal(cut[3], plain[3])
