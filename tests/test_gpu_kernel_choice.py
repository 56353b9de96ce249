"""The grid the search's kernel choice spans: row kind {f32, f16, i8, i8q} x chunks per lane NV {1, 3, 6} (32, 768, 1536
dimensions) x queue size class (ef 64, 200, 300, 600: queues of 128, 256 -- 512 under PHNSW_VISITED=global --, 512
and 1024 slots), on the throughput kernels (PHNSW_NO_LAT=1), plus the ef 200 row once as a small batch would run it
(latency kernel for f32, throughput for the converted kinds) and once with the visited sets in the HBM bitmap, plus one
search with Stored queries and exclude per kind and dimension at ef 300 (prepare_stored on the big-queue kernels).

Every search must equal -- ids, distance BITS, lengths, per-query distance and hop counters -- the oracle in the
kernel's summation order (SUM_BLOCKED64) over the rows phnsw_store_read returns for that store.  No tolerance.

f32, f16, i8: one graph per dimension, built by the oracle over the f32 rows (n = 2000) and adopted by all three stores;
129 raw queries (two full waves plus one), probe depth 2.

i8q equals the oracle on lattice data only (codes times a power of two, tests/test_i8q_cpu.py), so it has rows, graph and
queries of its own: i8q_reference.lattice rows, the oracle's graph over them as the store dequantises them, 129 lattice
queries.  Its grid launches every DistI8Q kernel pick_kernel_rows has (queue class / NV): ef 64 <2, 1|3|6>, ef 200
<8, 1>, <4, DistI8Q<3, 8>> and <4, 6>, ef 300 and ef 200 under PHNSW_VISITED=global <8, 1|3|6>, ef 600 <16, 1|3|6>.
At n = 2000 every layer is a dense one for every ef of the grid (tiny.hip: up to 80 ef nodes), so a search as it comes
sends only the entry vector through the kernel's distance policy; each i8q search therefore runs a second time under
PHNSW_NO_TINY=1, where every distance comes from DistI8Q::batch, against the same oracle result.

Wall time of the file on an MI355X: 3.0 s for the 54 searches of 129 queries over f32, f16 and i8 rows (the oracle's
three builds and its searches on the host are most of it; the slowest case, the first, takes 0.22 s).  The 30 cases
added with the i8q row (three more oracle builds, 2 to 5 s each on the host, and 21 cases of two searches) have not run
on an MI355X yet: no wall time for the 84 cases.  Until there is one, run the file under `timeout -k 10 120`."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import i8q_reference
from i8_reference import dequantize, quantize

pytestmark = pytest.mark.gpu

N, NQ, PD = 2000, 129, 2
KINDS = ["f32", "f16", "i8"]
DIMS = [32, 768, 1536]
EFS = [64, 200, 300, 600]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def graph(dim):
    """the f32 rows and the oracle's graph over them: [(nodes, neighbors[n, W])...] top first"""
    rows = oracle.synth_rows(0, N, dim)
    oix = oracle.Index.generate(rows, np.arange(N), oracle.default_build_params(seed=1), dim=dim,
                                sum_mode=oracle.SUM_BLOCKED64)
    return rows[:, :dim].copy(), [oix.layer(l) for l in range(oix.layer_count)]


def oracle_over(held, layers):
    """the oracle over the rows a store really holds, with the shared graph"""
    ix = oracle.Index(held, sum_mode=oracle.SUM_BLOCKED64)
    for nodes, nb in layers:
        ix.push_layer(nodes, nb, nb.shape[1])
    return ix


@pytest.fixture(scope="module")
def pairs():
    """(kind, dim) -> (GPU index over that store, oracle over store_read of it); built on first use, never changed"""
    made = {}

    def get(kind, dim):
        if (kind, dim) not in made:
            rows, layers = graph(dim)
            full = made.setdefault(("full", dim), ph.VectorStore(rows))
            store = {"f32": lambda s: s, "f16": ph.F16Store.from_full, "i8": ph.I8Store.from_full}[kind](full)
            made[(kind, dim)] = (ph.Hnsw.from_layers(store, layers, ph.BuildParameters(seed=1)),
                                 oracle_over(store.read(), layers))
        return made[(kind, dim)]

    return get


@functools.lru_cache(maxsize=None)
def queries(dim):
    return oracle.synth_rows(2 ** 32, NQ, dim)[:, :dim]


def same(gpu, cpu):
    gi, gd, gl, gs = gpu
    ci, cd, cl, cs = cpu
    np.testing.assert_array_equal(gl, cl)
    np.testing.assert_array_equal(gi, ci)
    np.testing.assert_array_equal(bits(gd), bits(cd))
    np.testing.assert_array_equal(gs, cs)  # distance evaluations and hops per query


def check(pairs, kind, dim, ef):
    hix, oix = pairs(kind, dim)
    q = queries(dim)
    same(hix.search_batch(queries=q, sp=ph.SearchParameters(ef, ef, PD), stats=True),
         oix.search(queries=q, sp=(ef, ef, PD), stats=True))


@pytest.mark.parametrize("ef", EFS)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_throughput_kernels(pairs, monkeypatch, kind, dim, ef):
    monkeypatch.setenv("PHNSW_NO_LAT", "1")
    check(pairs, kind, dim, ef)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_small_batch_kernels(pairs, monkeypatch, kind, dim):
    monkeypatch.delenv("PHNSW_NO_LAT", raising=False)
    check(pairs, kind, dim, 200)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_visited_in_the_bitmap(pairs, monkeypatch, kind, dim):
    monkeypatch.setenv("PHNSW_NO_LAT", "1")
    monkeypatch.setenv("PHNSW_VISITED", "global")
    check(pairs, kind, dim, 200)


STORED = np.arange(0, N, 15, dtype=np.uint64)  # 134 stored queries, the entry vector or not as the graph has it


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_stored_queries_with_exclude_on_the_big_queue_kernels(pairs, monkeypatch, kind, dim):
    monkeypatch.setenv("PHNSW_NO_LAT", "1")
    hix, oix = pairs(kind, dim)
    same(hix.search_batch(qids=STORED, sp=ph.SearchParameters(300, 300, PD), exclude=STORED, stats=True),
         oix.search(qids=STORED, sp=(300, 300, PD), exclude=STORED, stats=True))


# ---------------------------------------------------------------- the i8q row of the grid
def lattice_rows(n, dim, seed):
    rows, c, k = i8q_reference.lattice(n, dim, np.random.default_rng(seed))
    # what makes the oracle's f32 sums exact on these rows, asserted on the inputs themselves
    assert int(np.abs(c.astype(np.int64)).sum(axis=1).max()) * 127 < 2 ** 24
    return rows


@functools.lru_cache(maxsize=None)
def i8q_queries(dim):
    return lattice_rows(NQ, dim, 104729 + dim)


@pytest.fixture(scope="module")
def i8q_pairs():
    """dim -> (GPU index over the i8q store, oracle over store_read of it), both with the oracle's graph over the
    dequantised lattice rows; built on first use, never changed"""
    made = {}

    def get(dim):
        if dim not in made:
            rows = lattice_rows(N, dim, 7919 * N + dim)
            held = dequantize(*quantize(rows))
            np.testing.assert_array_equal(bits(held), bits(rows))  # lattice rows are their own dequantised rows
            g = oracle.Index.generate(held, np.arange(N), oracle.default_build_params(seed=1), dim=dim,
                                      sum_mode=oracle.SUM_BLOCKED64)
            layers = [g.layer(l) for l in range(g.layer_count)]
            store = ph.I8QStore.from_full(ph.VectorStore(rows))
            np.testing.assert_array_equal(bits(store.read()), bits(held))
            made[dim] = (ph.Hnsw.from_layers(store, layers, ph.BuildParameters(seed=1)), oracle_over(store.read(), layers))
        return made[dim]

    return get


def check_i8q(i8q_pairs, monkeypatch, dim, ef, **kw):
    """as it comes (every layer of 2000 nodes is a dense one: distances from the int8 table) and per hop (every distance
    from the kernel's DistI8Q), both against the oracle"""
    hix, oix = i8q_pairs(dim)
    if not kw:
        kw = dict(queries=i8q_queries(dim))
    cpu = oix.search(sp=(ef, ef, PD), stats=True, **kw)
    assert hix.dense_top_layers(ef)[0] == hix.layer_count()
    same(hix.search_batch(sp=ph.SearchParameters(ef, ef, PD), stats=True, **kw), cpu)
    assert hix.dispatches()[1]["n_table"] > 0
    monkeypatch.setenv("PHNSW_NO_TINY", "1")
    same(hix.search_batch(sp=ph.SearchParameters(ef, ef, PD), stats=True, **kw), cpu)
    d = hix.dispatches()[1]
    assert d["n_table"] == 0 and d["n_dist"] == int(cpu[3][:, 0].sum())


@pytest.mark.parametrize("ef", EFS)
@pytest.mark.parametrize("dim", DIMS)
def test_i8q_throughput_kernels(i8q_pairs, monkeypatch, dim, ef):
    monkeypatch.setenv("PHNSW_NO_LAT", "1")
    check_i8q(i8q_pairs, monkeypatch, dim, ef)


@pytest.mark.parametrize("dim", DIMS)
def test_i8q_small_batch_kernels(i8q_pairs, monkeypatch, dim):
    monkeypatch.delenv("PHNSW_NO_LAT", raising=False)
    check_i8q(i8q_pairs, monkeypatch, dim, 200)


@pytest.mark.parametrize("dim", DIMS)
def test_i8q_visited_in_the_bitmap(i8q_pairs, monkeypatch, dim):
    monkeypatch.setenv("PHNSW_NO_LAT", "1")
    monkeypatch.setenv("PHNSW_VISITED", "global")
    check_i8q(i8q_pairs, monkeypatch, dim, 200)


@pytest.mark.parametrize("dim", DIMS)
def test_i8q_stored_queries_with_exclude_on_the_big_queue_kernels(i8q_pairs, monkeypatch, dim):
    monkeypatch.setenv("PHNSW_NO_LAT", "1")
    check_i8q(i8q_pairs, monkeypatch, dim, 300, qids=STORED, exclude=STORED)
