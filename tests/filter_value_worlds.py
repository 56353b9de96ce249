"""The worlds of the filtered and exact top-k calls on value edges (test_filter_value_edges_cpu.py,
test_gpu_filter_value_edges.py): the families of tests/value_families.py at N = 2100 rows under all three metrics, the
rows an f32, f16 or i8 store holds of them, the bitmaps of every case, and both yardsticks:

  1. D = value_families.oracle_matrix(rows_held, q, metric, SUM_BLOCKED64), over which exact_filter_reference,
     filter_reference and filter_auto_reference restate the calls;
  2. the float64 second opinion: ref32 / topk64 on the lattice, ref64 within bound() elsewhere (second_opinion below).

Nothing here imports the library or touches a GPU.  rows_held of an f16 or i8 store is restated on the CPU (a rounding to
binary16; tests/i8_reference.py); the GPU file asserts that store.read() has exactly these bits before it uses D.

N = 2100: 66 bitmap words, so the scan takes two passes of 64 words, the second ragged; N % 32 == 20; the candidate
list crosses one 2 048-id border.  40 raw queries (the shared call needs 32 for the matrix-core table) and 8 stored."""
import functools

import numpy as np

import oracle
import exact_filter_reference as xr
import filter_auto_reference as ar
import filter_reference as fr
import value_families as vf
from i8_reference import dequantize, quantize

N, NW, NQ, NS = 2100, 66, 40, 8
assert (N + 31) // 32 == NW and N % 32 == 20 and 64 < NW < 128 and N > 2048
EMPTY = xr.EMPTY
INF_BITS = 0x7F800000
DIMS = (3, 100, 256, 260, 768)
FAMILY_METRIC = [(f, m) for f in ("lattice", "scaled", "cancelling", "tiny", "wide") for m in (0, 1, 2)] + [("l2_overflow", 2)]
# f16 where binary16 can hold the family's values (tiny rounds to rows of zeros: one tie over everything), i8 on two
KINDS_OF = {"lattice": ("f32", "f16"), "scaled": ("f32", "f16", "i8"), "cancelling": ("f32",), "tiny": ("f32", "f16"),
            "wide": ("f32", "i8"), "l2_overflow": ("f32",)}
WORLDS = [(f, m, d, k) for (f, m) in FAMILY_METRIC for d in DIMS for k in KINDS_OF[f]] + [("scaled", 1, 1536, "f32")]
WALK_WORLDS = [w for w in WORLDS if w[2] in (100, 768) and w[3] in ("f32", "f16")]
ROUTED_WORLDS = [(f, m, d, "f32") for (f, m) in (("scaled", 1), ("lattice", 2)) for d in (100, 256)]
INF_WORLDS = [("l2_overflow", 2, d, "f32") for d in (100, 768)]
# stored queries: 5 sits on the lattice's duplicate stride (5, 16, 27, ...), 2 is an all-zero lattice row, 16 is a copy
# of row 13; the others lie at the ends of the id range and on either side of the 2 048-id border
QIDS = np.array([5, 2, 16, 2047, 2048, 1023, 31, N - 1], dtype=np.uint64)
# lattice rows i and i - 3 that are equal (value_families.lattice), at the start, across the pass border, near the end
COPIES = ((13, 16), (2048, 2051), (2081, 2084))
SP_WIDE, SP_NARROW = (64, 64, 2), (6, 6, 9)
ROUTED_EF, ROUTED_K = 64, 10
INF_EF, INF_K = 1024, 10


def world_id(w):
    return "%s-m%d-d%d-%s" % w


def mask(density, shape, seed):
    return np.random.default_rng(seed).random(shape) < density


# ---------------------------------------------------------------- rows
@functools.lru_cache(maxsize=None)
def family_rows(family, dim):
    """(rows [N, ld], raw queries [NQ, dim], replaced row ids, replaced query ids) -- the last two empty but on l2_overflow"""
    if family == "l2_overflow":
        return vf.l2_overflow(N, dim, nq=NQ)
    rows, q = vf.make(family, N, dim, nq=NQ)
    return rows, q, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def held_rows(family, dim, kind):
    """[N, ld] f32: the rows a store of `kind` holds, i.e. what store.read() returns, zero-padded to ld"""
    rows = family_rows(family, dim)[0]
    if kind == "f32":
        return rows
    if kind == "f16":
        h = rows[:, :dim].astype(np.float16)
        assert np.isfinite(h).all()  # the family fits binary16
        return vf._pad(h.astype(np.float32))
    assert kind == "i8"
    return vf._pad(dequantize(*quantize(rows[:, :dim])))


@functools.lru_cache(maxsize=None)
def world(family, metric, dim, kind):
    """rows as held, the raw and stored queries, yardstick 1's distance of each to every row; made once, changed by no test"""
    rows, q, big_rows, big_q = family_rows(family, dim)
    held = held_rows(family, dim, kind)
    qs = np.ascontiguousarray(held[QIDS.astype(np.int64), :dim])
    return dict(family=family, metric=metric, dim=dim, kind=kind, held=held, q=q, qids=QIDS, qs=qs,
                Dq=vf.oracle_matrix(held, q, metric, oracle.SUM_BLOCKED64),
                Ds=vf.oracle_matrix(held, qs, metric, oracle.SUM_BLOCKED64), big_rows=big_rows, big_q=big_q)


@functools.lru_cache(maxsize=2)
def opinion(family, metric, dim, kind):
    """yardstick 2 per form (0 raw, 1 stored): ref64, bound and ref32 over the held rows"""
    w = world(family, metric, dim, kind)
    return [(vf.ref64(w["held"], x, metric), vf.bound(w["held"], x, metric), vf.ref32(w["held"], x, metric)) for x in (w["q"], w["qs"])]


def key_of(w):
    return w["family"], w["metric"], w["dim"], w["kind"]


# ---------------------------------------------------------------- graphs
@functools.lru_cache(maxsize=None)
def graph(family, metric, dim):
    """[(nodes, neighbors)] top first, built by the oracle over the family's f32 rows; for l2_overflow over vf.scaled (the
    reference cannot build over rows at +inf from everything) and adopted over the overflowing rows"""
    base = vf.scaled(N, dim, nq=NQ)[0] if family == "l2_overflow" else family_rows(family, dim)[0]
    g = vf.graph_over(base, dim, metric)
    layers = [g.layer(l) for l in range(g.layer_count)]
    entry = int(layers[0][0][0])
    assert entry not in family_rows(family, dim)[2]  # the entry vector is not a replaced row
    return layers


def walk_layers(w):
    return [(nodes, nb, {int(v): i for i, v in enumerate(nodes)}) for nodes, nb in graph(w["family"], w["metric"], w["dim"])]


def entry_vector(w):
    return int(graph(w["family"], w["metric"], w["dim"])[0][0][0])


def walkable(w, form):
    """bool per query: at a finite distance from the entry vector (a query at +inf from it is outside the walk's contract)"""
    return np.isfinite((w["Dq"], w["Ds"])[form][:, entry_vector(w)])


def restated_walk(w, form, sp, allow, exclude=None, rows=None):
    """filter_reference.search over yardstick 1 for the queries `rows` (default: all) -> ids, d, len, stats"""
    D = (w["Dq"], w["Ds"])[form]
    rows = np.arange(len(D)) if rows is None else rows
    a = allow if allow is None or np.ndim(allow) == 1 else allow[rows]
    return fr.search(None, D[rows], sp, allow=a, exclude=None if exclude is None else exclude[rows], layers=walk_layers(w))


# ---------------------------------------------------------------- bitmaps and cases
def shared_bitmap():
    return mask(0.3, N, 301)


def per_query_bitmaps():
    return mask(0.05, (NQ, N), 302)


def small_bitmap():
    """about 100 candidates, the lattice's equal pairs among them: with k = 1024 every candidate is returned"""
    m = mask(0.045, N, 303)
    m[np.array(COPIES).reshape(-1)] = True
    assert 64 < m.sum() < 192
    return m


def own_ids(form):
    """exclude: a stored query's own id; the raw queries exclude nothing"""
    return QIDS.copy() if form == 1 else None


def scan_cases(w, per_query=True):
    """(name, allow, exclude by form, k) of case A; case B runs them without the per-query bitmaps"""
    out = []
    for k in (1, 10, 64):
        out.append(("shared 0.3 k %d" % k, shared_bitmap(), (None, None), k))
        if per_query:
            out.append(("per query 0.05 k %d" % k, per_query_bitmaps(), (None, None), k))
        out.append(("no filter k %d" % k, None, (None, own_ids(1)), k))
    out.append(("about 100 candidates k 1024", small_bitmap(), (None, None), 1024))
    if w["family"] == "tiny" and w["metric"] != 2:
        out.append(("no filter k 1024", None, (None, own_ids(1)), 1024))  # one tie over sixteen 64-id batches
    return out


def of_form(w, form, allow, nq=None):
    """(D, allow) of one form, cut to the form's query count (or to nq)"""
    D = (w["Dq"], w["Ds"])[form]
    n = len(D) if nq is None else min(nq, len(D))
    return D[:n], (allow if allow is None or np.ndim(allow) == 1 else allow[:n])


def routed_bitmaps():
    """even queries at density 0.5 (1050 candidates: the graph), odd ones at 0.05 (105: below ceil(10 * 2100 / 64) = 329)"""
    m = mask(0.5, (NQ, N), 304)
    m[1::2] = mask(0.05, (NQ, N), 305)[1::2]
    return m


def inf_bitmap(w):
    """the replaced rows and five ordinary ones"""
    fin = np.setdiff1d(np.arange(N), w["big_rows"])
    m = np.zeros(N, dtype=bool)
    m[w["big_rows"]] = True
    m[fin[::400][:5]] = True
    return m


def restated_routed(w, form, allow, ef, k, rows=None, exclude=None):
    """phnsw_search_filtered_auto restated over yardstick 1: the strict restated walk and exact_topk, composed"""
    D = (w["Dq"], w["Ds"])[form]
    rows = np.arange(len(D)) if rows is None else rows
    a = allow if np.ndim(allow) == 1 else allow[rows]
    e = None if exclude is None else exclude[rows]
    walk = fr.strict(restated_walk(w, form, (ef, ef, 2), allow, exclude, rows), a)
    scan = xr.exact_topk(D[rows], a, e, None, k)
    return ar.compose(walk, scan, N, ef, k, N, a, e, None, 1)


# ---------------------------------------------------------------- yardstick 2
def second_opinion_distances(w, form, ids, d, ln, rows=None):
    """every returned distance against float64: on the lattice the bits of ref32, elsewhere within bound() of ref64
    where finite and +inf exactly where the f32 sum of squares overflows"""
    R64, B, R32 = opinion(*key_of(w))[form]
    rows = np.arange(len(ln)) if rows is None else rows
    for i, r in enumerate(rows):
        m = int(ln[i])
        v, x = ids[i, :m].astype(np.int64), d[i, :m]
        if w["family"] == "lattice":
            np.testing.assert_array_equal(vf.bits(x), vf.bits(R32[r, v] + np.float32(0.0)))
            continue
        fin = np.isfinite(x)
        np.testing.assert_array_equal(~fin, np.isinf(R32[r, v]))
        assert (vf.bits(x[~fin]) == INF_BITS).all()
        err = np.abs(x[fin].astype(np.float64) - R64[r, v[fin]])
        assert (err <= B[r, v[fin]]).all(), (key_of(w), form, r, float(err.max()))


def second_opinion(w, form, res, allow, exclude, k):
    """an exact row against float64.  Lattice: the ids are topk64's restricted to the candidates (ref32, then id).
    Elsewhere: the distances as above, and no candidate left out lies below the k-th returned one by more than both
    bounds; behind a k-th entry at +inf only candidates at +inf are left out."""
    R64, B, R32 = opinion(*key_of(w))[form]
    ids, d, ln = res[:3]
    second_opinion_distances(w, form, ids, d, ln)
    for i in range(len(ln)):
        cand = np.nonzero(xr.candidates(N, allow, exclude, None, i))[0]
        m = int(ln[i])
        assert m == min(k, len(cand))
        v = ids[i, :m].astype(np.int64)
        if w["family"] == "lattice":
            np.testing.assert_array_equal(v, cand[np.lexsort((cand, R32[i, cand] + np.float32(0.0)))][:k])
            continue
        rest = np.setdiff1d(cand, v)
        assert len(rest) + m == len(cand)  # candidates only, each once
        if not len(rest):
            continue
        last = v[-1]
        if np.isinf(R32[i, last]):
            assert np.isinf(R32[i, rest]).all()
        else:
            rest = rest[np.isfinite(R32[i, rest])]
            assert (R64[i, rest] >= R64[i, last] - B[i, last] - B[i, rest]).all(), (key_of(w), form, i)


# ---------------------------------------------------------------- what the GPU file asserts to occur
def has_negative(res):
    valid = np.arange(res[0].shape[1])[None, :] < res[2][:, None]
    return bool((res[1][valid] < 0).any())


def expects_negative(w):
    return w["family"] in ("scaled", "wide") and w["metric"] != 2


def assert_whole_tie(w, res, allow, exclude, k):
    """tiny under a dot metric: every distance is exactly 0.5 / 1.0, so a row is the k lowest candidate ids"""
    want = np.float32(0.5 if w["metric"] == 0 else 1.0)
    for i in range(len(res[2])):
        cand = np.nonzero(xr.candidates(N, allow, exclude, None, i))[0][:k]
        m = int(res[2][i])
        np.testing.assert_array_equal(res[0][i, :m], cand.astype(np.uint64))
        assert (vf.bits(res[1][i, :m]) == vf.bits(want)).all()


def assert_copies_adjacent(res, pairs=COPIES):
    """equal lattice rows share every distance: both of a pair in one row = next to each other, lower id first; only a
    candidate at the same distance with an id between theirs may stand between them (at dim 3 there are such)"""
    seen = 0
    for i in range(len(res[2])):
        row = res[0][i, :int(res[2][i])].tolist()
        for a, b in pairs:
            if a in row and b in row:
                at, bt = row.index(a), row.index(b)
                assert at < bt and len(set(vf.bits(res[1][i, at:bt + 1]).tolist())) == 1, (i, a, b)
                assert row[at:bt + 1] == sorted(row[at:bt + 1]), (i, a, b)
                seen += 1
    return seen


def assert_inf_tail(w, res, allow, k, replaced_queries):
    """l2_overflow: the finite candidates ascending, then the candidates at +inf in id order with bits 0x7F800000, then
    padding; the row of a replaced query (at +inf from every ordinary row, and from a replaced row unless all `dim`
    signs agree: none does at the dims used) is k entries at +inf in id order"""
    cand = np.nonzero(allow)[0]
    tails = 0
    for i in range(len(res[2])):
        m = int(res[2][i])
        assert m == min(k, len(cand))
        d, v = res[1][i, :m], res[0][i, :m].astype(np.int64)
        fin = np.isfinite(d)
        nf = int(fin.sum())
        assert fin[:nf].all() and (vf.bits(d[nf:]) == INF_BITS).all()  # finite first, then +inf: never mixed
        assert (np.diff(v[nf:]) > 0).all()
        assert (res[0][i, m:] == EMPTY).all() and (vf.bits(res[1][i, m:]) == vf.bits(xr.FMAX)).all()
        tails += m > nf
        if i in replaced_queries:
            assert nf == 0 and m == k, (i, nf, m)
    return tails
