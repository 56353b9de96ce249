"""numpy restatement of the i8q store's distance (include/phnsw.h): the query quantised like a row
(i8_reference.quantize), idot = the exact integer dot product of the codes, dot = (sq * sr) * float(idot) with two f32
multiplies in that order, then the metric.  `lattice` makes rows on which the f32 arithmetic of the unchanged oracle
gives the same bits, which is how the searches are checked."""
import numpy as np

from i8_reference import quantize

METRIC_COSINE_HALF, METRIC_ONE_MINUS_DOT = 0, 1


def distance_codes(cq, sq, codes, scales, metric):
    """a query given as codes [dim] and scale against rows given as codes [n, dim] and scales [n] -> [n] f32"""
    idot = codes.astype(np.int64) @ cq.astype(np.int64)
    assert np.abs(idot).max(initial=0) < 2 ** 31
    dot = (np.float32(sq) * scales.astype(np.float32)).astype(np.float32) * idot.astype(np.float32)  # int -> f32: RNE
    one = np.float32(1.0)
    return ((one - dot) / np.float32(2.0) if metric == METRIC_COSINE_HALF else one - dot).astype(np.float32)


def distance(q, codes, scales, metric):
    """a raw query [dim] f32: quantised with the rows' quantiser"""
    cq, sq = quantize(np.asarray(q, dtype=np.float32)[None, :])
    return distance_codes(cq[0], sq[0], codes, scales, metric)


def matrix(queries, codes, scales, metric, qids=None):
    """every distance: raw queries [nq, dim], or stored rows qids (their codes and scales as they are) -> [nq, n] f32"""
    if qids is not None:
        return np.stack([distance_codes(codes[int(i)], scales[int(i)], codes, scales, metric) for i in qids])
    return np.stack([distance(q, codes, scales, metric) for q in queries])


def ranked(D, exclude=None, entry=0):
    """what a search that evaluates every row must return for the distances D [nq, n]: per query all ids sorted by
    (distance, id), -0.0 folded into +0.0 for the order.  exclude [nq] drops one id per query, as Stored queries with
    exclude = qids do -- except where that id is the entry vector, which is in the running candidates before any layer
    filters its output and stays.  -> per query: ids int64 [n or n - 1], distances f32"""
    ids, ds = [], []
    for i, d in enumerate(D):
        order = np.lexsort((np.arange(len(d)), d + np.float32(0.0)))
        if exclude is not None and int(exclude[i]) != entry:
            order = order[order != int(exclude[i])]
        ids.append(order.astype(np.int64))
        ds.append(d[order])
    return ids, ds


def circulant(n, reach=1):
    """one layer in which node i sees i - reach .. i + reach.  reach 1, a ring: the visited nodes are an arc whose two
    ends are the only nodes not yet expanded, so every hop finds exactly one new node until the arc closes, and with
    ef = n a search evaluates and returns every node at any probe depth.  reach > 1: a hop may find nothing new, which
    counts against the probe depth; with a probe depth above n the walk still reaches every node.
    -> [(nodes, neighbors [n, 2 * reach])] as Hnsw.from_layers and Index.push_layer take it"""
    assert n > 2 * reach
    i = np.arange(n, dtype=np.int64)
    steps = [s for r in range(1, reach + 1) for s in (-r, r)]
    return [(i.astype(np.uint64), np.stack([(i + s) % n for s in steps], axis=1).astype(np.uint64))]


def assert_saturated(idot):
    """the conditions the `saturated` family is for, on the exact dot products of the codes"""
    big = np.abs(idot) > 2 ** 24
    assert 4 * int(big.sum()) >= idot.size, "a quarter of the pairs past 2^24"
    assert int((big & (idot % 2 != 0)).sum()) >= 100, "odd dot products past 2^24: exact ties between two floats"
    assert (idot[big] > 0).any() and (idot[big] < 0).any(), "both signs"
    assert int(np.abs(idot).max()) < 2 ** 31


def idots(cq, codes):
    """exact integer dot products of code rows [nq, dim] and [n, dim] -> [nq, n] int64"""
    return cq.astype(np.int64) @ codes.astype(np.int64).T


def saturated(n, dim, rng):
    """rows whose integer dot products pass 2^24: + or - one shared sign pattern at full scale (codes +-127), three
    to six components per row lowered to 126, 125 or 0 and one to three signs flipped, times a per-row power of two 2^k with
    k in [1, 6].  Every product of two scales is then at least 4 and the unit in the last place of (sq * sr) * f32(idot)
    at least 8, so 1 - dot rounds back to -dot: each bit of the converted idot shows in the distance.  quantize() returns
    exactly (c, 2^k).  At 1536 dimensions |idot| is 127^2 * 1536 = 24 774 144 less at most 18 * 2 * 127^2.
    -> rows f32, c int8, k"""
    assert dim >= 64
    # the pattern depends on the dimension alone: rows and queries drawn by separate calls share it
    pattern = np.where(np.random.default_rng(dim).integers(0, 2, size=dim) == 1, 127, -127).astype(np.int32)
    c = pattern[None, :] * np.where(rng.integers(0, 2, size=n) == 1, 1, -1)[:, None]
    c[: min(n, 2)] *= np.array([[1], [-1]])[: min(n, 2)]  # both signs, whatever the draw
    for i in range(n):
        at = rng.choice(dim - 1, size=9, replace=False) + 1  # component 0 keeps +-127: the scale stays 2^k
        low = int(rng.integers(3, 7))  # 3 to 6 components lowered, so that the sums come in both parities
        c[i, at[:low]] = np.sign(c[i, at[:low]]) * rng.choice([126, 125, 0], size=low)
        c[i, at[6:6 + int(rng.integers(1, 4))]] *= -1
    k = rng.integers(1, 7, size=n)
    rows = (c.astype(np.float64) * np.exp2(k.astype(np.float64))[:, None]).astype(np.float32)
    return rows, c.astype(np.int8), k


# what rintf does to k + 1/2, written out: the nearest even integer
TIES = [(0.5, 0), (1.5, 2), (-2.5, -2), (2.5, 2), (3.5, 4), (-0.5, 0), (-1.5, -2), (-3.5, -4), (125.5, 126), (126.5, 126),
        (-125.5, -126), (-126.5, -126), (63.5, 64), (64.5, 64), (-63.5, -64), (-64.5, -64)]
SUBNORMAL_ROW_SCALE, HUGE_ROW_SCALE = 2.0 ** 120, 2.0 ** -56  # what the rows are multiplied by for these two queries


def quantiser_edges(dim):
    """queries on the edges of the quantiser, each with the codes and the scale it must quantise to, written by hand (no
    quantiser runs here) -> [(name, query f32 [dim], codes int8 [dim], scale f32, power of two the store's rows are
    multiplied by so that sq * sr is a normal number and the codes show in the distance bits)]"""
    assert dim >= 4
    i = np.arange(dim)
    out = []

    def add(name, q, codes, scale, row_scale=1.0):
        q = np.asarray(q, dtype=np.float64)
        assert (q.astype(np.float32).astype(np.float64) == q).all(), name  # the query is what was written
        out.append((name, q.astype(np.float32), np.asarray(codes, dtype=np.int8), np.float32(scale), row_scale))

    # half-to-even ties, even and odd k, both signs; the maximum 127 * 2^-3 makes the scale 2^-3 exactly
    x = np.array([TIES[j % len(TIES)][0] for j in i])
    c = np.array([TIES[j % len(TIES)][1] for j in i])
    x[dim - 1], c[dim - 1] = 127.0, 127
    add("ties", x / 8.0, c, 0.125)
    # a pattern of codes in [-125, 125] with the +-127 wherever a case wants it
    pat = (i * 7) % 251 - 125
    c = pat.copy()
    c[1] = -127
    add("max_negative", c * 0.5, c, 0.5)
    c = pat.copy()
    c[0] = 127
    add("max_first", c * 1.0, c, 1.0)
    c = pat.copy()
    c[dim - 1] = 127
    add("max_last", c * 2.0, c, 2.0)
    # x / (x / 127) is 127 to within an ulp for any x
    third = np.float32(0.3)
    add("all_equal", np.full(dim, float(third)), np.full(dim, 127), third / np.float32(127.0))
    c = np.zeros(dim, dtype=np.int64)
    c[dim // 2] = -127
    add("one_component", np.where(c != 0, -2.5, 0.0), c, np.float32(2.5) / np.float32(127.0))
    # every component an f32 subnormal: maxabs 127 * 2^-133 < 2^-126, scale 2^-133 (a subnormal itself), x / scale exact
    c = pat.copy()
    c[2] = 127
    add("subnormal", c * 2.0 ** -133, c, 2.0 ** -133, SUBNORMAL_ROW_SCALE)
    # one component of 127 * 2^53 = 1.14e18, two ties and a -2 beside it, everything else far below half a step
    x = np.where(i % 2 == 0, 1.0, -1.0)
    c = np.zeros(dim, dtype=np.int64)
    x[1], c[1] = 127.0 * 2.0 ** 53, 127
    x[0], c[0] = 1.5 * 2.0 ** 53, 2
    x[2], c[2] = -0.5 * 2.0 ** 53, 0
    x[3], c[3] = -2.0 * 2.0 ** 53, -2
    add("huge", x, c, 2.0 ** 53, HUGE_ROW_SCALE)
    add("zeros", np.zeros(dim), np.zeros(dim), 0.0)
    return out


def lattice(n, dim, rng, k_range=12):
    """rows c * 2^k: integer codes c in [-127, 127] with one component per row forced to +-127, a per-row power of two
    with k in [-k_range, k_range].  quantize() returns exactly (c, 2^k) for them.  -> rows f32, c int8, k"""
    c = np.clip(np.rint(40.0 * rng.standard_normal((n, dim))), -127, 127).astype(np.int32)
    c[np.arange(n), rng.integers(0, dim, size=n)] = np.where(rng.integers(0, 2, size=n) == 1, 127, -127)
    k = rng.integers(-k_range, k_range + 1, size=n)
    rows = (c.astype(np.float64) * np.exp2(k.astype(np.float64))[:, None]).astype(np.float32)
    return rows, c.astype(np.int8), k
