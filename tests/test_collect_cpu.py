"""CPU checks of the collecting search's test reference (tests/collect_reference.py), pinned to the unchanged oracle:

  * every row allowed, k <= number_of_candidates, both flag values: the row is oracle.search(...)[:k] -- ids, distance
    bits, lengths -- and the stats are oracle.search's (a change of `kept` then implies a change of the layer's queue, so
    EXTEND is a no-op);
  * without EXTEND and with a random filter the stats are oracle.search's: the traversal is the plain search's;
  * the row holds the first k entries of the STRICT post-filter row (filter_reference.strict) or better ones: entry for
    entry its (distance, id) is not above the strict row's, and it is at least as long -- against the post-filter of the
    walk it shares (see below);
  * EXTEND never evaluates less than the plain walk, and its row is entry for entry as good or better;
  * a constructed path at probe_depth 2: EXTEND returns rows the plain walk stops short of, and stops itself once the
    idle-hop budget is spent;
  * fewer than k allowed rows on a connected bottom layer, with a probe depth the walk cannot use up: every allowed row
    reachable from the entry is returned, with either flag value.

The last case as the issue words it -- "with EXTEND ... every allowed row reachable from the entry is returned" -- holds
for any probe depth only if a walk with EXTEND runs until its frontier is exhausted.  Under the contract's own rule (a
hop did something when it changed the layer's queue or `kept`; probe_depth counts the hops that improve neither) a walk
stops after probe_depth idle hops in all (the budget is never refilled), however many allowed rows lie further out.  The case therefore runs with
probe_depth = the bottom layer's node count: every hop expands another node, so the budget outlasts the frontier.

The superset case needs the same care.  The issue words it against filter_reference.strict(filter_reference.search(allow)),
the filtered walk.  That walk filters the queue of EVERY layer, so below the top layer it descends from other candidates
than the plain search, which the contract makes the collecting search's descent (upper layers unfiltered, stats equal to
the plain search's).  The two bottom-layer walks then evaluate different rows and neither row contains the other: at
dim 6, sp (64, 16, 2), density 0.5, k 10 the strict row of the filtered walk holds (0.05920783, 1173) and
(0.06327033, 1251) in fifth and sixth place, rows the plain descent never evaluates, where `kept` has (0.06671077, 869)
and (0.06677541, 724).  So the case is checked where it is a theorem: against the strict post-filter of the PLAIN
search's row for every descent, and against the filtered walk itself where the two descents coincide (upto_layers = 1:
the only layer walked is the last)."""
import numpy as np
import pytest

import oracle

import collect_reference as cr
import filter_reference as fr
from value_families import bits, graph_over

N, NQ = 1500, 24


_made = {}


def built(dim):
    if dim not in _made:
        rows = oracle.synth_rows(0, N, dim)
        ix = graph_over(rows, dim, oracle.METRIC_COSINE_HALF)
        assert ix.layer_count >= 3
        _made[dim] = (ix, fr.layers_of(ix), oracle.synth_rows(2 ** 32, NQ, dim)[:, :dim].copy())
    return _made[dim]


def keys(ids, d, ln):
    """[(distance, id)] of the valid entries of one row"""
    return [(float(d[i]), int(ids[i])) for i in range(int(ln))]


@pytest.mark.parametrize("extend", [False, True])
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("dim,sp", [(6, (64, 16, 2)), (100, (96, 96, 3))])
def test_every_row_allowed_is_the_head_of_the_plain_search(dim, sp, k, extend):
    ix, layers, q = built(dim)
    qids = np.arange(3, N, N // NQ, dtype=np.uint64)[:NQ]
    for kw, D in ((dict(queries=q), fr.distance_rows(ix, queries=q)), (dict(qids=qids), fr.distance_rows(ix, qids=qids))):
        pi, pd_, pl, ps = ix.search(sp=sp, stats=True, **kw)
        for allow in (np.ones(N, dtype=bool), None):
            gi, gd, gl, gs = cr.search(ix, D, sp, k, allow=allow, extend=extend, layers=layers)
            np.testing.assert_array_equal(gl, np.minimum(pl, k))
            np.testing.assert_array_equal(gi, pi[:, :k])
            np.testing.assert_array_equal(bits(gd), bits(pd_[:, :k]))
            np.testing.assert_array_equal(gs, ps)


@pytest.mark.parametrize("dim,sp", [(6, (64, 16, 2)), (100, (96, 96, 3))])
def test_filtered_rows_against_the_plain_walk_and_the_strict_post_filter(dim, sp):
    ix, layers, q = built(dim)
    D = fr.distance_rows(ix, queries=q)
    rng = np.random.default_rng(11 + dim)
    plain = ix.search(queries=q, sp=sp, stats=True)
    ex = plain[0][:, 2].copy()
    for density, k in ((0.5, 10), (0.05, 10), (0.05, 64), (0.3, 1)):
        allow = rng.random((NQ, N)) < density
        allow[np.arange(NQ), ex.astype(np.int64)] = True  # the excluded row is itself allowed
        for exclude, base in ((None, plain), (ex, ix.search(queries=q, sp=sp, exclude=ex, stats=True))):
            got = cr.search(ix, D, sp, k, allow=allow, exclude=exclude, layers=layers)
            np.testing.assert_array_equal(got[3], base[3])  # without EXTEND the traversal is the plain search's
            ext = cr.search(ix, D, sp, k, allow=allow, exclude=exclude, extend=True, layers=layers)
            assert (ext[3] >= got[3]).all()
            strict = fr.strict(base, allow)  # the post-filter of the walk `kept` was collected on
            for i in range(NQ):
                g, e, s = keys(*[x[i] for x in got[:3]]), keys(*[x[i] for x in ext[:3]]), keys(*[x[i] for x in strict[:3]])
                s = [x for x in s if exclude is None or x[1] != int(ex[i])]  # (an excluded entry vector stays in that row)
                assert g == sorted(g) and len(set(v for _, v in g)) == len(g)
                assert all(allow[i, v] and (exclude is None or v != int(ex[i])) for _, v in g + e)
                assert len(g) >= min(k, len(s)) and all(a <= b for a, b in zip(g, s[:k]))
                assert len(e) >= len(g) and all(a <= b for a, b in zip(e, g))
                # whatever the strict row holds and `kept` does not is behind kept's tail
                if len(g) == k:
                    assert all(x in g or x > g[-1] for x in s)
                else:
                    assert all(x in g for x in s)


@pytest.mark.parametrize("dim,sp", [(6, (64, 16, 2)), (100, (96, 96, 3))])
def test_one_layer_rows_hold_the_head_of_the_filtered_walks_strict_row(dim, sp):
    """upto_layers = 1: the filtered walk and the collecting walk are the same walk of the top layer"""
    ix, layers, q = built(dim)
    D = fr.distance_rows(ix, queries=q)
    rng = np.random.default_rng(29 + dim)
    for density, k in ((0.5, 10), (0.1, 10), (0.5, 1)):
        allow = rng.random((NQ, N)) < density
        strict = fr.strict(fr.search(ix, D, sp, allow=allow, upto=1, layers=layers), allow)
        got = cr.search(ix, D, sp, k, allow=allow, upto=1, layers=layers)
        np.testing.assert_array_equal(got[3], strict[3])
        for i in range(NQ):
            g, s = keys(*[x[i] for x in got[:3]]), keys(*[x[i] for x in strict[:3]])
            assert len(g) >= min(k, len(s)) and all(a <= b for a, b in zip(g, s[:k]))
            assert all(x in g or (len(g) == k and x > g[-1]) for x in s)


def test_extend_walks_on_where_the_plain_walk_stops():
    """a constructed one-layer path 0 - 1 - 2 - ..., node i at distance i + 1, entry 0, ef 4, probe_depth 2: the walk goes
    outward one node per hop, the layer's queue is full after nodes 0..3, and every later hop is idle for it.  The plain
    walk therefore evaluates nodes 4 and 5 and stops.  With rows 4..30 allowed and EXTEND every hop up to node 30
    changes `kept`, so the budget lasts until nodes 31 and 32: the row holds 4..30, which the plain walk stops short of"""
    n, ef, pd, k = 60, 4, 2, 64
    nb = np.full((n, 2), fr.EMPTY, dtype=np.uint64)
    nb[0, 0] = 1
    for i in range(1, n):
        nb[i] = (i - 1, i + 1) if i + 1 < n else (i - 1, fr.EMPTY)
    layers = [(np.arange(n, dtype=np.uint64), nb, {i: i for i in range(n)})]
    drow = np.arange(1, n + 1, dtype=np.float32)
    allowed = lambda v: 4 <= v <= 30  # noqa: E731
    ids, d, ln, st = cr.search_one(layers, drow, (ef, ef, pd), k, allowed, fr.EMPTY, False)
    assert ids[:ln].tolist() == [4, 5] and st == [6, 5]  # evaluations: the entry + nodes 1..5; hops: nodes 0..4 expanded
    ids, d, ln, st = cr.search_one(layers, drow, (ef, ef, pd), k, allowed, fr.EMPTY, True)
    assert ids[:ln].tolist() == list(range(4, 31)) and d[:ln].tolist() == [float(v + 1) for v in range(4, 31)]
    assert st == [33, 32]  # ... + nodes 6..32: the two idle hops are those that evaluate 31 and 32
    # a `kept` of 3 slots is full after node 6: from then on nothing changes it, and nodes 7 and 8 use up the budget
    ids, d, ln, st = cr.search_one(layers, drow, (ef, ef, pd), 3, allowed, fr.EMPTY, True)
    assert ids[:ln].tolist() == [4, 5, 6] and st == [9, 8]


@pytest.mark.parametrize("extend", [False, True])
def test_fewer_than_k_allowed_rows_all_come_back(extend):
    dim, k = 6, 10
    ix, layers, q = built(dim)
    D = fr.distance_rows(ix, queries=q)
    nodes, nb, vec2node = layers[-1]
    # the bottom layer as the walk sees it: everything reachable from the entry vector's node
    seen, todo = {vec2node[int(layers[0][0][0])]}, [vec2node[int(layers[0][0][0])]]
    while todo:
        for n in nb[todo.pop()]:
            if n != fr.EMPTY and int(n) not in seen:
                seen.add(int(n))
                todo.append(int(n))
    assert len(seen) == len(nodes) == N  # a connected graph
    rng = np.random.default_rng(3)
    allow = np.zeros((NQ, N), dtype=bool)
    for i in range(NQ):
        allow[i, rng.choice(N, size=i % k, replace=False)] = True  # 0 .. k - 1 allowed rows
    ids, d, ln, st = cr.search(ix, D, (64, 16, N), k, allow=allow, extend=extend, layers=layers)
    for i in range(NQ):
        want = sorted((float(D[i, v]), int(v)) for v in np.nonzero(allow[i])[0])
        assert keys(ids[i], d[i], ln[i]) == want
        assert (ids[i, len(want):] == fr.EMPTY).all() and (bits(d[i, len(want):]) == bits(fr.FMAX)).all()
