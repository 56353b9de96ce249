"""f32 rows of 1537 .. 4096 floats (DistF32Wide, the chunk classes 8 / 12 / 16) on the distance batch, the plain walk and
the build, against the CPU oracle in the kernels' summation order (ORC_SUM_BLOCKED64): bit for bit.

The distances are also held to a float64 reference.  A lane's chain is 4 NV fmas, the butterfly 6 adds and the metric one
more operation: e = (4 NV + 7) * 2^-24 * sum |terms|, terms = q_i x_i or (q_i - x_i)^2, carried through the metric with
its slope: 1/2 (cosine), 1 (dot), 1 / (2 sqrt r) (L2; a row against itself has r = e = 0)."""
import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from test_gpu_build import layers_equal
from test_gpu_search import assert_same, build_oracle_index, to_gpu

pytestmark = pytest.mark.gpu

COS, DOT, L2 = oracle.METRIC_COSINE_HALF, oracle.METRIC_ONE_MINUS_DOT, oracle.METRIC_L2


def f64_distance(q, x, metric):
    """the distance in float64 and the a-priori bound on an f32 result in the chunk class of len(q)"""
    q, x = q.astype(np.float64), x.astype(np.float64)
    nv = 8 if len(q) <= 2048 else (12 if len(q) <= 3072 else 16)
    terms = (q - x) ** 2 if metric == L2 else q * x
    r, e = terms.sum(), (4 * nv + 7) * 2.0 ** -24 * np.abs(terms).sum()
    if metric == L2:
        return np.sqrt(r), (e / (2 * np.sqrt(r)) if r > 0 else 0.0)
    return ((1 - r) / 2, e / 2) if metric == COS else (1 - r, e)


@pytest.mark.parametrize("metric", [COS, DOT, L2])
@pytest.mark.parametrize("dim", [1537, 1540, 2048, 2052, 3072, 4092, 4096])
def test_distance_bits(dim, metric):
    n = 130  # two full batches of 64 and a partial one
    rows = oracle.synth_rows(0, n, dim, normalize=(metric != L2))
    store = ph.VectorStore(rows[:, :dim], metric=metric)
    ix = oracle.Index(rows, dim=dim, metric=metric)
    ids = np.arange(n, dtype=np.uint64)
    raw = oracle.synth_rows(2 ** 32, 1, dim, normalize=(metric != L2))[0, :dim]
    for q, v in ((raw, ph.Unstored(raw)), (rows[7, :dim], ph.Stored(7))):
        got = store.compare_vec(v, ids)
        want = np.array([ix.distance(q, rows[i, :dim], oracle.SUM_BLOCKED64) for i in range(n)], dtype=np.float32)
        ref = [f64_distance(q, rows[i, :dim], metric) for i in range(n)]
        d64, bound = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
        print("dim %d metric %d: oracle error / bound at most %.3f" % (dim, metric, np.max(np.abs(want - d64)[bound > 0] / bound[bound > 0])))
        assert (np.abs(want - d64) <= bound).all()  # the oracle itself
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (np.abs(got - d64) <= bound).all()


def search_device(gix, sp, nq, queries=None, qids=None):
    torch = pytest.importorskip("torch")
    ef = sp.number_of_candidates
    ids = torch.empty((nq, ef), dtype=torch.int32, device="cuda")
    d = torch.empty((nq, ef), dtype=torch.float32, device="cuda")
    ln = torch.empty(nq, dtype=torch.int32, device="cuda")
    status = torch.empty(nq, dtype=torch.int32, device="cuda")
    if queries is not None:
        qd = torch.from_numpy(np.ascontiguousarray(queries)).cuda()
        kw = dict(queries=qd.data_ptr(), ldq=queries.shape[1])
    else:
        qd = torch.from_numpy(qids.astype(np.int32)).cuda()
        kw = dict(qids=qd.data_ptr())
    torch.cuda.synchronize()
    gix.search_batch_device(nq, sp, ids.data_ptr(), d.data_ptr(), ln.data_ptr(), status.data_ptr(), **kw)
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    ln = ln.cpu().numpy().astype(np.uint64)
    live = ln[:, None] > np.arange(ef, dtype=np.uint64)[None, :]  # entries past a row's length are not part of the result
    return np.where(live, ids.cpu().numpy().astype(np.uint64), ph.EMPTY), np.where(live, d.cpu().numpy(), np.float32(0)), ln


@pytest.mark.parametrize("n,dim,ef,metric", [(1500, 2048, 64, COS), (1500, 3072, 300, COS), (1000, 4096, 128, L2),
                                             (1200, 1540, 256, COS), (1000, 3072, 1024, COS)])
def test_walk_parity(n, dim, ef, metric):
    """one shape per queue size (128, 256, 512, 1024 slots) and per class; raw and stored queries, host and device form"""
    rows, oix = build_oracle_index(n, dim, metric=metric, normalize=(metric != L2))
    store, gix = to_gpu(rows, dim, oix, metric)
    q = oracle.synth_rows(2 ** 32, 70, dim, normalize=(metric != L2))
    qids = np.arange(0, n, 13, dtype=np.uint64)
    sp = ph.SearchParameters(ef, ef, 2)
    for kw in (dict(queries=q[:, :dim]), dict(qids=qids)):
        cpu = oix.search(sp=(ef, ef, 2), stats=True, **kw)
        gpu = gix.search_batch(sp=sp, stats=True, **kw)
        assert_same(gpu, cpu)
        np.testing.assert_array_equal(gpu[3], cpu[3])  # distance evaluations and hops per query
        live = cpu[2][:, None] > np.arange(ef, dtype=np.uint64)[None, :]
        dev = search_device(gix, sp, len(cpu[2]), queries=q if "queries" in kw else None, qids=qids)
        assert_same(dev, (np.where(live, cpu[0], ph.EMPTY), np.where(live, cpu[1], np.float32(0)), cpu[2]))


@pytest.mark.parametrize("n,dim,metric", [(1200, 2048, COS), (800, 3076, L2), (700, 3072, DOT), (600, 4096, COS)])  # classes 8, 16 (769 chunks), 12, 16
def test_build_parity(n, dim, metric):
    rows = oracle.synth_rows(0, n, dim, normalize=(metric != L2))
    bp = oracle.default_build_params(seed=3)
    oix = oracle.Index.generate(rows, np.arange(n), bp, dim=dim, metric=metric, sum_mode=oracle.SUM_BLOCKED64)
    gix = ph.Hnsw.generate(ph.VectorStore(rows[:, :dim], metric=metric), np.arange(n), ph.BuildParameters(seed=3))
    layers_equal(gix, oix)
    assert gix.stochastic_recall() == oix.stochastic_recall_at(oix.layer_count - 1, bp.optimization)


def test_past_the_last_class():
    n, dim = 64, 4100
    store = ph.VectorStore(oracle.synth_rows(0, n, dim)[:, :dim].copy())
    with pytest.raises(ph.PhnswError) as e:
        store.compare_vec(ph.Stored(0), np.arange(n, dtype=np.uint64))
    assert e.value.code == -7 and "4096" in str(e.value)  # PHNSW_E_UNSUPPORTED
    nodes = np.arange(n, dtype=np.uint64)
    gix = ph.Hnsw.from_layers(store, [(nodes, ((nodes[:, None] + 1 + np.arange(4, dtype=np.uint64)) % n))])
    with pytest.raises(ph.PhnswError) as e:
        gix.search_batch(qids=nodes[:4], sp=ph.SearchParameters(16, 16, 2))
    assert e.value.code == -7 and "4096" in str(e.value)
