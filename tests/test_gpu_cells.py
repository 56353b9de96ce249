"""Cells that follow the data (bruteforce.hip) and the table order of a launch (api.hip, tiny.hip).

The cells: every anchor is replaced once by the normalised mean of the sample rows nearest to it, and nodes are
assigned over all dimensions.  Checked against a float64 numpy statement of the same procedure on a 64-cluster store.
The order: a plain launch of at least 2 048 queries with a dense table walks in the order of the cells its queries
land in.  Order only, so every result is what the natural order gives, and what the raw cells give."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from parallel_hnsw_amd._lib import check, lib

pytestmark = pytest.mark.gpu

N, K, SEED = 65536, 64, 42  # the smallest store that carries cells
SHAPES = {64: 1.0, 256: 2.0}  # dim -> noise: the vector-unit table and the matrix-core table
NQ = 2048 + 37
EF = 128  # the 5 461-node layer is the table layer on both table kernels (48 * ef and 80 * ef nodes)


class env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def table_order_count():
    f = lib().phnsw_debug_table_order_count
    f.restype = C.c_uint64
    return f()


def store_cells(store):
    """(anchors [A][dim] f32, rank [A]) of a store, made on first use"""
    f = lib().phnsw_debug_store_cells
    na = C.c_uint32()
    check(f(store._h, None, None, C.byref(na)))
    anchors = np.empty((na.value, store.ld), dtype=np.float32)
    rank = np.empty(na.value, dtype=np.uint32)
    check(f(store._h, anchors.ctypes.data_as(C.c_void_p), rank.ctypes.data_as(C.c_void_p), C.byref(na)))
    return anchors[:, :store.dim], rank


def layer_pos(h, lft, n_nodes):
    pos = np.empty(n_nodes, dtype=np.uint32)
    check(lib().phnsw_debug_layer_cells(h._h, C.c_uint32(lft), pos.ctypes.data_as(C.c_void_p)))
    return pos


def cluster_of_rows(first, n):
    """the cluster every synthetic row was drawn from (the generator's own hash, misc.hip)"""
    u = np.uint64
    with np.errstate(over="ignore"):
        x = (u(SEED) + u(first) + np.arange(n, dtype=u)) * u(0xA24BAED4963EE407) + u(0x9FB21C651E98DF25)
        x ^= x >> u(30)
        x *= u(0xBF58476D1CE4E5B9)
        x ^= x >> u(27)
        x *= u(0x94D049BB133111EB)
        x ^= x >> u(31)
        hi, lo = x >> u(32), x & u(0xFFFFFFFF)
        return ((hi * u(K) + ((lo * u(K)) >> u(32))) >> u(32)).astype(np.int64)


def own_majority_share(cell, cluster, n_cells):
    cnt = np.zeros((n_cells, K), dtype=np.int64)
    np.add.at(cnt, (cell, cluster), 1)
    return float((cnt.argmax(1)[cell] == cluster).mean())


def assign(r64, a64, chosen=None):
    """float64 scores of rows against anchors, a piece at a time: (best anchor, best score - score of `chosen`)"""
    best = np.empty(len(r64), dtype=np.int64)
    lost = np.zeros(len(r64))
    for at in range(0, len(r64), 8192):
        sc = r64[at:at + 8192] @ a64.T
        best[at:at + 8192] = sc.argmax(1)
        if chosen is not None:
            lost[at:at + 8192] = sc.max(1) - sc[np.arange(len(sc)), chosen[at:at + 8192]]
    return best, lost


def reference_cells(r64, n_anchors):
    """the procedure in float64: strided rows as anchors, one mean pass over the (whole, here) sample, all dimensions"""
    anchors = r64[np.arange(n_anchors) * (len(r64) // n_anchors)].copy()
    cell, _ = assign(r64, anchors)
    for a in np.unique(cell):
        s = r64[cell == a].sum(0)
        anchors[a] = s / np.sqrt((s * s).sum())
    return assign(r64, anchors)[0]


@pytest.fixture(scope="module", params=sorted(SHAPES))
def built(request):
    dim = request.param
    store = ph.VectorStore.clustered(N, dim, seed=SEED, n_clusters=K, noise=SHAPES[dim])
    h = ph.Hnsw.generate(store, np.arange(N, dtype=np.uint64), ph.BuildParameters(max_link_rounds=1))
    return dim, store, h


def test_cells_follow_the_clusters(built):
    dim, store, h = built
    rows = store.read().astype(np.float64)
    anchors, rank = store_cells(store)
    A = len(anchors)
    assert A == 4096 and sorted(rank.tolist()) == list(range(A))
    cell_of_rank = np.argsort(rank)
    a64 = anchors.astype(np.float64)
    cluster = cluster_of_rows(0, N)
    L = h.layer_count()
    for lft in (L - 1, L - 2):  # the bottom layer (node = row) and the table layer of the searches below
        nodes = np.asarray(h.layers[lft].nodes, dtype=np.int64)
        pos = layer_pos(h, lft, len(nodes))
        assert int(pos.max()) < A
        cell = cell_of_rank[pos]
        _, lost = assign(rows[nodes], a64, cell)
        print("dim %d layer %d: largest score given up %.3g (bound %.3g)" % (dim, lft, lost.max(), 2 * dim * 2.0 ** -24))
        assert lost.max() <= 2 * dim * 2.0 ** -24
        if lft == L - 1:
            ref = own_majority_share(reference_cells(rows, A), cluster, A)
            got = own_majority_share(cell, cluster, A)
            print("dim %d: nodes whose cell's majority cluster is their own: %.4f, float64 reference %.4f" % (dim, got, ref))
            assert ref > 0.9
            assert got >= ref - 0.02


def test_anchors_are_the_same_bits_twice(built):
    dim, store, _ = built
    again = ph.VectorStore.clustered(N, dim, seed=SEED, n_clusters=K, noise=SHAPES[dim])
    a, ra = store_cells(store)
    b, rb = store_cells(again)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    np.testing.assert_array_equal(ra, rb)
    np.testing.assert_allclose(np.sqrt((a.astype(np.float64) ** 2).sum(1)), 1.0, atol=1e-5)
    with env(PHNSW_CELLS="raw"):
        raw = ph.VectorStore.clustered(N, dim, seed=SEED, n_clusters=K, noise=SHAPES[dim])
        c, _ = store_cells(raw)
    np.testing.assert_array_equal(c.view(np.uint32), store.read()[np.arange(len(c)) * (N // len(c))].view(np.uint32))
    assert (a.view(np.uint32) != c.view(np.uint32)).any()


def search_device(h, q, sp):
    import torch
    dev = torch.device("cuda", 0)
    nq, ef = len(q), sp.number_of_candidates
    qd = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    ids = torch.full((nq, ef), -1, dtype=torch.int32, device=dev)
    d = torch.zeros((nq, ef), dtype=torch.float32, device=dev)
    ln = torch.zeros(nq, dtype=torch.int32, device=dev)
    stats = torch.zeros((nq, 2), dtype=torch.int32, device=dev)
    status = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    h.search_batch_device(nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), queries=qd.data_ptr(),
                          ldq=q.shape[1], out_stats=stats.data_ptr())
    torch.cuda.synchronize()
    ln_ = ln.cpu().numpy()
    live = ln_[:, None] > np.arange(ef)[None, :]  # entries past a row's length are not part of the result
    return (np.where(live, ids.cpu().numpy(), -1), np.where(live, d.cpu().numpy().view(np.uint32), 0), ln_,
            stats.cpu().numpy(), status.cpu().numpy())


def test_results_do_not_depend_on_the_order_or_the_cells(built):
    dim, store, h = built
    assert dim % 4 == 0 and store.ld == dim
    q = ph.VectorStore.clustered(NQ, dim, seed=SEED, first=2 ** 33, n_clusters=K, noise=SHAPES[dim]).read()
    sp = ph.SearchParameters(EF, EF, 2)
    layers, table_nodes, matrix_cores = h.dense_top_layers(EF)
    assert layers == h.layer_count() - 1 and table_nodes >= 256 and matrix_cores == (dim == 256)
    before = table_order_count()
    ordered = search_device(h, q, sp)
    assert table_order_count() == before + 1, "the launch did not take the table order"
    with env(PHNSW_TABLE_ORDER="0"):
        natural = search_device(h, q, sp)
    assert table_order_count() == before + 1
    short = search_device(h, q[:2047], sp)  # under the threshold: natural order
    assert table_order_count() == before + 1
    with env(PHNSW_CELLS="raw"):
        store_raw = ph.VectorStore.clustered(N, dim, seed=SEED, n_clusters=K, noise=SHAPES[dim])
        h_raw = ph.Hnsw.from_layers(store_raw, [(l.nodes, l.neighbors) for l in h.layers])
        raw = search_device(h_raw, q, sp)
    assert table_order_count() == before + 2
    assert int(np.abs(ordered[4]).sum()) == 0 and int(ordered[2].min()) == EF
    for what, a, b, c, s in zip(("ids", "distance bits", "lengths", "counters", "status"), ordered, natural, raw, short):
        np.testing.assert_array_equal(a, b, err_msg=what + ": table order against natural order")
        np.testing.assert_array_equal(a, c, err_msg=what + ": refined cells against raw cells")
        np.testing.assert_array_equal(a[:2047], s, err_msg=what + ": a list under the threshold")
    # and the oracle, on a slice: the order is no part of any result
    ix = oracle.Index(store.read(), dim=dim, metric=oracle.METRIC_COSINE_HALF, sum_mode=oracle.SUM_BLOCKED64)
    for l in h.layers:
        ix.push_layer(l.nodes, l.neighbors, l.neighborhood_size)
    m = 200
    ci, cd, cl, cs = ix.search(queries=q[:m], sp=(EF, EF, 2), stats=True)
    np.testing.assert_array_equal(ordered[2][:m].astype(np.uint64), cl.astype(np.uint64))
    np.testing.assert_array_equal(ordered[0][:m].astype(np.uint64), ci.astype(np.uint64))
    np.testing.assert_array_equal(ordered[1][:m], cd.view(np.uint32))
    np.testing.assert_array_equal(ordered[3][:m].astype(np.uint64), cs.astype(np.uint64))


@pytest.mark.parametrize("kind", ["F16Store", "I8Store"])
def test_converted_stores_get_the_same_treatment(built, kind):
    """an f16 / i8 store refines its anchors on its widened rows and takes the table order like the f32 store; the
    order changes none of its results either"""
    dim, store, h = built
    conv = getattr(ph, kind)(store)
    g = ph.Hnsw.from_layers(conv, [(l.nodes, l.neighbors) for l in h.layers])
    q = ph.VectorStore.clustered(NQ, dim, seed=SEED, first=2 ** 34, n_clusters=K, noise=SHAPES[dim]).read()
    sp = ph.SearchParameters(EF, EF, 2)
    before = table_order_count()
    ordered = search_device(g, q, sp)
    assert table_order_count() == before + 1
    with env(PHNSW_TABLE_ORDER="0"):
        natural = search_device(g, q, sp)
    assert table_order_count() == before + 1
    for what, a, b in zip(("ids", "distance bits", "lengths", "counters", "status"), ordered, natural):
        np.testing.assert_array_equal(a, b, err_msg=what)
    anchors, rank = store_cells(conv)
    assert sorted(rank.tolist()) == list(range(len(anchors)))
    np.testing.assert_allclose(np.sqrt((anchors.astype(np.float64) ** 2).sum(1)), 1.0, atol=1e-5)
    L = g.layer_count()
    assert int(layer_pos(g, L - 1, N).max()) < len(anchors)
    cell = np.argsort(rank)[layer_pos(g, L - 1, N)]
    got = own_majority_share(cell, cluster_of_rows(0, N), len(anchors))
    print("%s dim %d: nodes whose cell's majority cluster is their own: %.4f" % (kind, dim, got))
    assert got > 0.9 - 0.02  # the floor the f32 reference must clear, less the same 0.02: rounding a row moves no cluster
