"""Run time on an MI355X: not measured (the file has not run on one yet); until it has, run it under `timeout -k 10 120`.

Every entry of the i8q store's int8 distance table (ph_tiny_table_i8_kernel, tiny.hip) and, beside it, the same
distances through DistI8Q in the search kernels and through phnsw_distance_batch, against the numpy restatement of
tests/i8q_reference.py.  No oracle, no built graph and no tolerance: one layer in which node i sees i - 1 and i + 1,
searched with ef = n, evaluates and returns every node whatever the data (i8q_reference.circulant says why;
tests/test_i8q_cpu.py checks it against the oracle), so for each query the result must be all n ids sorted by
(distance, id) with the reference's distance bits, n evaluations and n hops.

Each case runs twice, and both runs must equal the reference, not merely each other:
  * as it comes: the one layer is a dense one, so every distance but the entry vector's is a look-up in the table of the
    int8 matrix-core kernel (n_table == (n - 1) nq of n_dist == n nq: the entry vector's distance, before any layer,
    is a per-hop evaluation in every one-launch descent, search.hip).  A walk never looks up the entry vector's column, so
    the raw table of the launch (phnsw_debug_last_tiny_table) is compared as well, all nq x n entries of it;
  * under PHNSW_NO_TINY=1: every distance from DistI8Q::batch in the search kernel, n_table == 0.

Shapes: n on both sides of the 32-row MFMA halves and the 64-node block tiles, nq likewise, dimensions of one code
word (K padded from 4 / 8 bytes to 128), a ragged, an exactly full and a just-begun last K step, and 12 steps; every n
and every nq with every dimension class, every dimension with both metrics.  Data: general rows (oracle.synth_rows),
`saturated` rows whose integer dot products pass 2^24 -- where an f32 partial sum, a truncating or a half-away int -> f32
conversion shows -- and queries on the quantiser's edges (i8q_reference.quantiser_edges)."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph

import i8q_reference as ref
from i8_reference import quantize

pytestmark = pytest.mark.gpu

COS, DOT = oracle.METRIC_COSINE_HALF, oracle.METRIC_ONE_MINUS_DOT
NS = [3, 31, 32, 33, 63, 64, 65, 127, 129, 200]
NQS = [1, 5, 31, 33, 64, 65, 129]
DIM_CLASSES = {"one_word": [4, 6], "ragged": [100], "last_step": [124, 128, 132], "two_steps": [256, 260], "six_steps": [768],
               "twelve_steps": [1532, 1536]}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def class_cases(name):
    """ten (n, nq, dim, metric): every n once, every nq at least once (which n meets which nq differs from class to
    class), the class's dimensions in turn, and the metric changing once they have all had their turn"""
    dims = DIM_CLASSES[name]
    shift = sorted(DIM_CLASSES).index(name)
    return [(n, NQS[(j + shift) % len(NQS)], dims[j % len(dims)], (COS, DOT)[(j // len(dims)) % 2]) for j, n in enumerate(NS)]


def test_the_case_lists_cover_what_they_claim():
    for name, dims in DIM_CLASSES.items():
        cases = class_cases(name)
        assert sorted(c[0] for c in cases) == NS and {c[1] for c in cases} == set(NQS)
        assert {(c[2], c[3]) for c in cases} == {(d, m) for d in dims for m in (COS, DOT)}


@functools.lru_cache(maxsize=None)
def general_rows(n, dim, row_scale=1.0):
    return np.ascontiguousarray(oracle.synth_rows(0, n, dim)[:, :dim] * np.float32(row_scale))


def raw_table(hix):
    """[positions, nodes] of the dense table the last launch on hix made; fails when it made none"""
    f = ph.lib().phnsw_debug_last_tiny_table
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64] + [C.POINTER(C.c_uint32)] * 3 + [C.POINTER(C.c_int)]
    npos, tn, stride, g = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int()
    assert f(hix._h, None, 0, C.byref(npos), C.byref(tn), C.byref(stride), C.byref(g)) == 0
    out = np.empty((npos.value, stride.value), dtype=np.float32)
    assert f(hix._h, out.ctypes.data, out.size, C.byref(npos), C.byref(tn), C.byref(stride), C.byref(g)) == 0
    return out[:, :tn.value]


class Case:
    """an i8q store over `rows`, one circulant layer over it, and the numpy quantiser's codes and scales of the rows"""

    def __init__(self, rows, metric, reach=1):
        self.n, self.metric, self.reach = rows.shape[0], metric, reach
        self.codes, self.scales = quantize(rows)
        self.store = ph.I8QStore.from_full(ph.VectorStore(rows, metric=metric))
        np.testing.assert_array_equal(self.store.codes(), self.codes)
        np.testing.assert_array_equal(bits(self.store.scales()), bits(self.scales))
        self.hix = ph.Hnsw.from_layers(self.store, ref.circulant(self.n, reach))
        # a ring is exhausted at any probe depth; a wider graph has hops that find nothing new, which count against it
        self.sp = ph.SearchParameters(self.n, self.n, 2 if reach == 1 else self.n + 1)

    def check(self, monkeypatch, msg, queries=None, qids=None, exclude=None):
        n = self.n
        D = ref.matrix(queries, self.codes, self.scales, self.metric, qids)
        assert np.isfinite(D).all(), msg
        want_ids, want_d = ref.ranked(D, exclude)
        nq = len(D)
        kw = dict(queries=queries) if qids is None else dict(qids=qids, exclude=exclude)
        for path in ("table", "per hop"):
            with monkeypatch.context() as mp:
                if path == "per hop":
                    mp.setenv("PHNSW_NO_TINY", "1")
                gi, gd, gl, gs = self.hix.search_batch(sp=self.sp, stats=True, **kw)
                disp = self.hix.dispatches()
            at = "%s, %s" % (msg, path)
            assert len(disp) == 2 and disp[1]["n_dist"] == n * nq, (at, disp)
            if path == "table":
                assert disp[1]["n_table"] == (n - 1) * nq, (at, disp)  # all but the entry vector's
                np.testing.assert_array_equal(bits(raw_table(self.hix)), bits(D), err_msg=at + ": the raw table")
            else:
                assert disp[1]["n_table"] == 0, (at, disp)
            np.testing.assert_array_equal(gs[:, 0], np.full(nq, n), err_msg=at + ": evaluations")
            if self.reach == 1:
                np.testing.assert_array_equal(gs[:, 1], np.full(nq, n), err_msg=at + ": hops")
            for i in range(nq):
                w = len(want_ids[i])
                assert gl[i] == w, "%s: query %d returns %d of %d" % (at, i, gl[i], w)
                np.testing.assert_array_equal(gi[i, :w].astype(np.int64), want_ids[i], err_msg="%s: ids of query %d" % (at, i))
                np.testing.assert_array_equal(bits(gd[i, :w]), bits(want_d[i]), err_msg="%s: distance bits of query %d" % (at, i))
                assert (gi[i, w:] == ph.EMPTY).all() and (bits(gd[i, w:]) == bits(oracle.FMAX)).all(), at
        # the same distances through phnsw_distance_batch, for the first, the middle and the last query
        ids = np.arange(n, dtype=np.uint64)
        for i in sorted({0, nq // 2, nq - 1}):
            v = ph.Unstored(queries[i]) if qids is None else ph.Stored(int(qids[i]))
            np.testing.assert_array_equal(bits(self.store.compare_vec(v, ids)), bits(D[i]),
                                          err_msg="%s: distance batch of query %d" % (msg, i))

    def check_all_forms(self, monkeypatch, msg, q):
        """raw queries, Stored queries with and without exclude; nq = len(q)"""
        nq = len(q)
        self.check(monkeypatch, msg + " raw", queries=q)
        qids = ((np.arange(nq) * 7 + 1) % self.n).astype(np.uint64)  # repeats when nq > n; the entry vector 0 among them
        self.check(monkeypatch, msg + " stored", qids=qids)
        self.check(monkeypatch, msg + " stored + exclude", qids=qids, exclude=qids)


def general_queries(rows, nq, dim):
    """synth queries with every third one a stored row passed raw (quantised again, like any raw query)"""
    q = np.ascontiguousarray(oracle.synth_rows(2 ** 32, nq, dim)[:, :dim])
    q[::3] = rows[(np.arange(0, nq, 3) * 5) % rows.shape[0]]
    return q


# ---------------------------------------------------------------- general data: every n, nq and dimension
@pytest.mark.parametrize("name", sorted(DIM_CLASSES))
def test_general_rows(name, monkeypatch):
    for n, nq, dim, metric in class_cases(name):
        rows = general_rows(n, dim)
        case = Case(rows, metric)
        case.check_all_forms(monkeypatch, "general n %d nq %d dim %d metric %d" % (n, nq, dim, metric),
                             general_queries(rows, nq, dim))


# ---------------------------------------------------------------- dot products past 2^24
@pytest.mark.parametrize("metric", [COS, DOT])
@pytest.mark.parametrize("dim", [1536, 1532])
def test_saturated_rows(dim, metric, monkeypatch):
    rng = np.random.default_rng(dim)
    rows, c, k = ref.saturated(200, dim, rng)
    q, cq, kq = ref.saturated(65, dim, rng)
    codes, scales = quantize(q)
    np.testing.assert_array_equal(codes, cq)  # the numpy quantiser gives the planned codes; the rows' are checked in Case
    ref.assert_saturated(ref.idots(cq, c))
    case = Case(rows, metric)
    np.testing.assert_array_equal(case.codes, c)
    case.check_all_forms(monkeypatch, "saturated dim %d metric %d" % (dim, metric), q)
    # stored rows against each other pass 2^24 as well, in both signs
    ref.assert_saturated(ref.idots(c[:65], c))


# ---------------------------------------------------------------- wider graphs: masks of up to 64 candidates per hop
@pytest.mark.parametrize("reach", [12, 32])
@pytest.mark.parametrize("family,dim", [("general", 100), ("general", 768), ("general", 260), ("saturated", 1536)])
def test_wide_circulant(family, dim, reach, monkeypatch):
    """i +- 1 .. reach at n = 200: the first hop evaluates 2 * reach new nodes (24; 64, a full mask), the later ones
    whatever the walk leaves, in rounds of four with tails that are no multiple of four -- 1, 3 and 6 chunks per lane,
    with the 8-row kernel at 768 dimensions"""
    n, nq = 200, 33
    if family == "saturated":
        rng = np.random.default_rng(dim + reach)
        rows, c, k = ref.saturated(n, dim, rng)
        q = ref.saturated(nq, dim, rng)[0]
        ref.assert_saturated(ref.idots(quantize(q)[0], c))
    else:
        rows = general_rows(n, dim)
        q = general_queries(rows, nq, dim)
    Case(rows, COS if reach == 12 else DOT, reach).check_all_forms(monkeypatch, "%s dim %d reach %d" % (family, dim, reach), q)


# ---------------------------------------------------------------- queries on the quantiser's edges
@pytest.mark.parametrize("metric", [COS, DOT])
@pytest.mark.parametrize("dim", [4, 6, 100, 132, 260, 768, 1536])
def test_quantiser_edge_queries(dim, metric, monkeypatch):
    n = 65
    edges = ref.quantiser_edges(dim)
    tiny = np.finfo(np.float32).tiny
    for row_scale in sorted({e[4] for e in edges}):
        group = [e for e in edges if e[4] == row_scale]
        case = Case(general_rows(n, dim, row_scale), metric)
        q = np.stack([e[1] for e in group])
        for name, query, want_codes, want_scale, _ in group:
            prod = (want_scale * case.scales).astype(np.float32)
            assert (prod == 0).all() if name == "zeros" else (prod >= tiny).all(), name  # no product of scales underflows
        case.check(monkeypatch, "edges %s dim %d metric %d" % ("+".join(e[0] for e in group), dim, metric), queries=q)
