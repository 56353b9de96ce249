"""The dense table made beside the other workspace's search kernel (csrc/tiny.hip, search.hip: vis_table_slots).

The matrix-core table kernel has two staging depths: G = 2 for a launch that has the chip to itself, G = 1 (half the
LDS, at most 128 registers) for a launch whose table pass runs beside the search kernel of the index's other
workspace.  PHNSW_TABLE_BESIDE=0|1|auto picks; the prepared graph and the packed node operand are kept per workspace
between launches.  None of it may move a bit of any result.

Every GPU step runs in a child process under its own `timeout`: this file, started as a script with the case's name.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

STEP_SECONDS = 300
# n, dim, metric name, sp: the three row widths the matrix-core table takes
SHAPES = {256: (8000, 256, "METRIC_ONE_MINUS_DOT", (64, 64, 2)),
          768: (6000, 768, "METRIC_COSINE_HALF", (104, 104, 8)),
          1536: (3000, 1536, "METRIC_COSINE_HALF", (128, 128, 2))}


def run_case(*args, env=None):
    e = dict(os.environ)
    e.pop("PHNSW_TABLE_BESIDE", None)
    e.pop("PHNSW_NO_TINY_KEEP", None)
    e.setdefault("PHNSW_HOST_CHUNKS", "4000000000,1024,4096")  # one launch per list, as for test_gpu_tiny (conftest.py)
    e.update(env or {})
    cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__)] + [str(a) for a in args]
    p = subprocess.run(cmd, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(p.stdout)
    print(p.stderr[-4000:])
    assert p.returncode == 0, "case %s ended with status %d" % (" ".join(map(str, args)), p.returncode)
    return p


@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_both_staging_depths_make_the_same_table(dim):
    run_case("tables", dim)


def test_searches_equal_the_oracle_in_every_form():
    run_case("search")


def test_kept_graph_and_operand_are_rebuilt_when_the_index_changes():
    run_case("epoch")


def test_second_of_two_launches_in_flight_takes_the_beside_form():
    p = run_case("lanes", env={"PHNSW_VERBOSE": "1"})
    forms = {}
    phase = None
    for line in p.stderr.splitlines():
        m = re.match(r"\[case\] phase (\w+)", line)
        if m:
            phase = m.group(1)
        m = re.search(r"dense table: .* matrix cores, G = (\d)", line)
        if m and phase:
            forms.setdefault(phase, []).append(int(m.group(1)))
    assert forms.get("pair") == [2, 1], forms   # the first finds the index idle, the second finds the first in flight
    assert forms.get("lone") == [2], forms


# ------------------------------------------------------------------------------------------------ the child process

def _setup(dim, seed=3):
    sys.path.insert(0, ROOT)
    import oracle
    import parallel_hnsw_amd as ph
    n, dim, metric, sp = SHAPES[dim]
    metric = getattr(ph, metric)
    rows = oracle.synth_rows(0, n, dim)[:, :dim]
    store = ph.VectorStore(rows, metric=metric)
    h = ph.Hnsw.generate(store, np.arange(n, dtype=np.uint64), ph.BuildParameters(seed=seed, max_link_rounds=1))
    assert h._layer(0).node_count() <= 1024
    assert h.dense_top_layers(sp[0])[2], "this shape's table is not made on the matrix cores"
    return oracle, ph, rows, store, h, metric, sp


def _oracle_of(oracle, rows, dim, metric, h):
    ix = oracle.Index(rows, dim=dim, metric=metric, sum_mode=oracle.SUM_BLOCKED64)
    for l in h.layers:
        ix.push_layer(l.nodes, l.neighbors, l.neighborhood_size)
    return ix


def _raw_table(ph, h):
    L = ph.lib()
    f = L.phnsw_debug_last_tiny_table
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64] + [C.POINTER(C.c_uint32)] * 3 + [C.POINTER(C.c_int)]
    npos, tn, stride, g = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int()
    assert f(h._h, None, 0, C.byref(npos), C.byref(tn), C.byref(stride), C.byref(g)) == 0
    out = np.empty((npos.value, stride.value), dtype=np.float32)
    assert f(h._h, out.ctypes.data, out.size, C.byref(npos), C.byref(tn), C.byref(stride), C.byref(g)) == 0
    return out[:, :tn.value].copy(), g.value


def _equal(got, want, what):
    gi, gd, gl, gs = got
    ci, cd, cl, cs = want
    assert np.array_equal(gi, ci), what + ": ids"
    assert np.array_equal(gd.view(np.uint32), cd.view(np.uint32)), what + ": distance bits"
    assert np.array_equal(gl, cl), what + ": lengths"
    assert np.array_equal(gs, cs), what + ": counters"


def case_tables(dim):
    oracle, ph, rows, store, h, metric, sp = _setup(dim)
    d = rows.shape[1]
    q = oracle.synth_rows(2 ** 32, 333, d)[:, :d]  # 5 whole position tiles + 13 rows; the table layer's size is no multiple of 64 either
    spx = ph.SearchParameters(*sp)
    tables = {}
    for mode, g_want in (("0", 2), ("1", 1)):
        os.environ["PHNSW_TABLE_BESIDE"] = mode
        res = h.search_batch(queries=q, sp=spx, stats=True)
        tables[mode], g = _raw_table(ph, h)
        assert g == g_want, "PHNSW_TABLE_BESIDE=%s ran G = %d" % (mode, g)
        tables[mode + "res"] = res
    assert tables["0"].shape[0] == 333 and tables["0"].shape[1] % 64 != 0, tables["0"].shape
    assert np.array_equal(tables["0"].view(np.uint32), tables["1"].view(np.uint32)), "G = 1 and G = 2 tables differ"
    _equal(tables["1res"], tables["0res"], "results of the two forms")
    print("tables equal: %d x %d, dim %d" % (tables["0"].shape + (d,)))


def case_search():
    oracle, ph, rows, store, h, metric, sp = _setup(768)
    d = rows.shape[1]
    # 1500 queries: past the latency kernels, so the throughput kernel with the hole in its LDS runs; 333: the latency kernels
    q = oracle.synth_rows(2 ** 32, 1500, d)[:, :d]
    want = _oracle_of(oracle, rows, d, metric, h).search(queries=q, sp=sp, stats=True)
    spx = ph.SearchParameters(*sp)
    for env in ({"PHNSW_TABLE_BESIDE": "1"}, {"PHNSW_TABLE_BESIDE": "0"}, {"PHNSW_TABLE_BESIDE": "auto"},
                {"PHNSW_TABLE_BESIDE": "1", "PHNSW_NO_TINY_KEEP": "1"}):
        for k in ("PHNSW_TABLE_BESIDE", "PHNSW_NO_TINY_KEEP"):
            os.environ.pop(k, None)
        os.environ.update(env)
        # the index's two workspaces alternate: calls 0 and 1 prepare, calls 2 and 3 find graph and operand kept
        for call in range(4):
            _equal(h.search_batch(queries=q, sp=spx, stats=True), want, "%s call %d" % (env, call))
            m = 333
            _equal(h.search_batch(queries=q[:m], sp=spx, stats=True), [x[:m] for x in want], "%s call %d, %d queries" % (env, call, m))
    print("searches equal the oracle")


def case_epoch():
    oracle, ph, rows, store, h, metric, sp = _setup(768)
    d = rows.shape[1]
    q = oracle.synth_rows(2 ** 32, 1500, d)[:, :d]
    spx = ph.SearchParameters(*sp)

    def check(what):
        want = _oracle_of(oracle, rows, d, metric, h).search(queries=q, sp=sp, stats=True)
        for call in range(3):  # both workspaces, and one of them a second time
            _equal(h.search_batch(queries=q, sp=spx, stats=True), want, "%s, call %d" % (what, call))
        return want

    first = check("fresh index")
    # a node list changes: vectors of layer 1 that layer 0 lacks join layer 0
    top, below = h._layer(0).nodes, h._layer(1).nodes
    extra = np.setdiff1d(below, top)[:5]
    h.extend_layer(0, extra)
    assert h._layer(0).node_count() == len(top) + len(extra)
    second = check("after extend_layer")
    # neighbour rows change in place: one more link round on the dense layers
    added = sum(h.link_layer_to_better_neighbors(l, ph.SearchParameters(300, 300, 2)) for l in (0, 1))
    third = check("after link rounds (%d new edges)" % added)
    moved = [not np.array_equal(a[0], b[0]) or not np.array_equal(a[3], b[3]) for a, b in ((first, second), (second, third))]
    print("results moved with the index: extend_layer %s, link rounds %s (%d edges)" % (moved[0], moved[1], added))


def case_lanes():
    oracle, ph, rows, store, h, metric, sp = _setup(768)
    import torch
    d = rows.shape[1]
    nq, ef = 20000, sp[0]
    dev = torch.device("cuda", 0)
    spx = ph.SearchParameters(*sp)
    q = torch.from_numpy(np.ascontiguousarray(oracle.synth_rows(2 ** 32, nq, d)[:, :d])).to(dev)
    s0 = torch.cuda.current_stream().cuda_stream
    s1 = ph.stream_create_beside(0, s0)

    def buffers():
        return (torch.empty((nq, ef), dtype=torch.int32, device=dev), torch.empty((nq, ef), dtype=torch.float32, device=dev),
                torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev))
    a, b = buffers(), buffers()

    def launch(o, stream):
        h.search_batch_device(nq, spx, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(),
                              queries=q.data_ptr(), ldq=d, stream=stream)

    def say(phase):
        sys.stderr.flush()
        os.write(2, ("[case] phase %s\n" % phase).encode())

    say("warm")  # allocations and first-use costs of both workspaces
    launch(a, s0)
    torch.cuda.synchronize()
    launch(b, s1)
    torch.cuda.synchronize()
    say("pair")  # two launches back to back on the two workspaces, a stream each
    launch(a, s0)
    launch(b, s1)
    torch.cuda.synchronize()
    say("lone")
    launch(a, s0)
    torch.cuda.synchronize()
    say("done")
    assert int(a[3].abs().sum()) == 0 and int(b[3].abs().sum()) == 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2])
    # a's last launch ran alone (G = 2), b's beside a's (G = 1): the same queries, the same bits
    assert int(a[2].min()) > 0


if __name__ == "__main__":
    case = sys.argv[1]
    if case == "tables":
        case_tables(int(sys.argv[2]))
    else:
        {"search": case_search, "epoch": case_epoch, "lanes": case_lanes}[case]()
