"""The grid the search's kernel choice spans: row kind {f32, f16, i8} x chunks per lane NV {1, 3, 6} (32, 768, 1536
dimensions) x queue size class (ef 64, 200, 300, 600: queues of 128, 256 -- 512 under PHNSW_VISITED=global --, 512
and 1024 slots), on the throughput kernels (PHNSW_NO_LAT=1), plus the ef 200 row once as a small batch would run it
(latency kernel for f32, throughput for the converted kinds) and once with the visited sets in the HBM bitmap.

Every search must equal -- ids, distance BITS, lengths, per-query distance and hop counters -- the oracle in the
kernel's summation order (SUM_BLOCKED64) over the rows phnsw_store_read returns for that store.  No tolerance.

One graph per dimension, built by the oracle over the f32 rows (n = 2000) and adopted by all three stores; 129 raw
queries (two full waves plus one), probe depth 2.

Wall time of the file on an MI355X: 3.0 s for its 54 searches of 129 queries (the oracle's three builds and its
searches on the host are most of it; the slowest case, the first, takes 0.22 s)."""
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

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


def check(pairs, kind, dim, ef):
    hix, oix = pairs(kind, dim)
    q = queries(dim)
    gi, gd, gl, gs = hix.search_batch(queries=q, sp=ph.SearchParameters(ef, ef, PD), stats=True)
    ci, cd, cl, cs = oix.search(queries=q, sp=(ef, ef, PD), stats=True)
    np.testing.assert_array_equal(gl, cl)
    np.testing.assert_array_equal(gi, ci)
    np.testing.assert_array_equal(bits(gd), bits(cd))
    np.testing.assert_array_equal(gs, cs)  # distance evaluations and hops per query


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
