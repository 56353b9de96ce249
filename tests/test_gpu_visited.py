"""The visited set of the gathered layers (csrc/search.hip): an open-addressed table in the wave's LDS, which moves
into the per-wave bitmap in HBM when a walk would pass its load limit.  Which of the two a walk uses must not change
a bit of the results: ids, distance bits, lengths, hop and evaluation counters equal the oracle's on the default
path, on the bitmap alone (PHNSW_VISITED=global) and with tables so small that walks move to the bitmap part-way
through a layer (PHNSW_VISITED_LDS_SLOTS)."""
import os
import re

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

pytestmark = pytest.mark.gpu

MODES = [
    {},                                      # the LDS table, sized by the launch
    {"PHNSW_VISITED": "global"},             # the bitmap throughout
    {"PHNSW_VISITED_LDS_SLOTS": "64"},       # every walk leaves the table within its first hops
    {"PHNSW_VISITED_LDS_SLOTS": "700"},      # bottom-layer walks leave it after a few hundred ids
]


class visited_mode:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in ("PHNSW_VISITED", "PHNSW_VISITED_LDS_SLOTS", "PHNSW_NO_LAT",
                                                     "PHNSW_VERBOSE")}
        for k in self.saved:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same_as_oracle(got, exp):
    gi, gd, gl, gs = got
    ci, cd, cl, cs = exp
    np.testing.assert_array_equal(gl, cl)
    np.testing.assert_array_equal(gs, cs)  # evaluations, hops
    np.testing.assert_array_equal(gi, ci)
    np.testing.assert_array_equal(gd.view(np.uint32), cd.view(np.uint32))


@pytest.fixture(scope="module")
def index768():
    n, dim = 6000, 768
    rows = oracle.synth_rows(0, n, dim)
    oix = oracle.Index.generate(rows, np.arange(n), oracle.default_build_params(seed=1), dim=dim,
                                sum_mode=oracle.SUM_BLOCKED64)
    store = ph.VectorStore(rows[:, :dim])
    g = ph.Hnsw.from_layers(store, [oix.layer(l) for l in range(oix.layer_count)])
    return oix, g, dim


def table_slots(err):
    """slots of the LDS visited table each search launch got (PHNSW_VERBOSE=1 on stderr)"""
    return [int(x) for x in re.findall(r"visited table (\d+) slots", err)]


# 256: the queues of 256 slots that leave room for the table; 100: queues of 128; 400: queues of 512, which leave
# no room for it at 768 dimensions
@pytest.mark.parametrize("sp", [(256, 256, 8), (100, 100, 2), (400, 400, 2)])
# the throughput kernels; the same on a batch <= 1024 (PHNSW_NO_LAT); the latency kernels, which keep the bitmap
@pytest.mark.parametrize("nq,lat", [(1500, False), (300, False), (300, True)])
def test_search_every_visited_path_equals_oracle(index768, sp, nq, lat, capfd):
    oix, g, dim = index768
    q = oracle.synth_rows(2 ** 32, nq, dim)[:, :dim]
    exp = oix.search(queries=q, sp=sp, stats=True)
    shape = not lat and sp[0] <= 256  # a kernel that compiles the table (search.hip: vis_lds_shape)
    for env in MODES:
        env = dict(env, PHNSW_VERBOSE="1", **({} if lat else {"PHNSW_NO_LAT": "1"}))
        capfd.readouterr()
        with visited_mode(env):
            got = g.search_batch(queries=q, sp=ph.SearchParameters(*sp), stats=True)
        slots = table_slots(capfd.readouterr().err)
        # which visited set the walks had: the path these results come from
        if not shape or "PHNSW_VISITED" in env:
            want = 0
        elif "PHNSW_VISITED_LDS_SLOTS" in env:
            want = int(env["PHNSW_VISITED_LDS_SLOTS"])
        else:
            want = None  # what the LDS leaves: 1024 slots at least
        assert slots, env
        assert all((n >= 1024) if want is None else (n == want) for n in slots), (env, slots)
        same_as_oracle(got, exp)


def test_knn_and_threshold_nn_every_visited_path_equal_oracle():
    n, dim = 4000, 32
    rows = oracle.synth_rows(0, n, dim)
    oix = oracle.Index.generate(rows, np.arange(n), oracle.default_build_params(seed=2), dim=dim,
                                sum_mode=oracle.SUM_BLOCKED64)
    store = ph.VectorStore(rows[:, :dim])
    g = ph.Hnsw.from_layers(store, [oix.layer(l) for l in range(oix.layer_count)])
    thr = np.float32(0.33)
    for k in (5, 200):
        ki, kd, kl = oix.knn(k, 2)
        for env in MODES:
            with visited_mode(env):
                res = g.knn(k, 2)
            for i, (v, got) in enumerate(res):
                assert [x[0] for x in got] == [int(x) for x in ki[i, :int(kl[i])]], (env, k, i)
                assert [np.float32(x[1]).view(np.uint32) for x in got] == [x.view(np.uint32) for x in kd[i, :int(kl[i])]]
    ti, td, tl = oix.threshold_nn(thr, 2, 4, max_out=256)
    assert int(tl.max()) > 8  # the queue grew
    for env in MODES:
        with visited_mode(env):
            res = g.threshold_nn(float(thr), 2, 4, max_out=256)
        for i, (v, got) in enumerate(res):
            assert [x[0] for x in got] == [int(x) for x in ti[i, :int(tl[i])]], (env, i)
            assert [np.float32(x[1]).view(np.uint32) for x in got] == [x.view(np.uint32) for x in td[i, :int(tl[i])]]


@pytest.mark.parametrize("n,dim", [(3000, 32), (1500, 768)])
def test_build_every_visited_path_equals_oracle(n, dim):
    """the link rounds of a build run the search kernel: the graph is the oracle's whichever visited set they use"""
    rows = oracle.synth_rows(0, n, dim)
    oix = oracle.Index.generate(rows, np.arange(n), oracle.default_build_params(seed=4), dim=dim,
                                sum_mode=oracle.SUM_BLOCKED64)
    store = ph.VectorStore(rows[:, :dim])
    for env in MODES:
        with visited_mode(env):
            gix = ph.Hnsw.generate(store, np.arange(n), ph.BuildParameters(seed=4))
        assert gix.layer_count() == oix.layer_count
        for l in range(oix.layer_count):
            nodes, nb = oix.layer(l)
            gl = gix._layer(l)
            np.testing.assert_array_equal(gl.nodes, nodes)
            np.testing.assert_array_equal(gl.neighbors, nb, err_msg="%s layer %d" % (env, l))
