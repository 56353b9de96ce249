"""Seeded value families for the distance-parity tests (test_value_families_cpu.py, test_gpu_value_edges.py), an
exact float64 reference of the three metrics and the a-priori f32 error bound.

Every generator returns (rows[n, ld] f32, queries[nq, dim] f32); ld is dim padded to a multiple of 4 with zeros, the
layout of oracle.synth_rows.  All values are finite.  Outside l2_overflow no sum of |a_i*b_i| or of (a_i-b_i)^2 can
exceed f32::MAX for any pair taken from rows and queries (checked through Cauchy-Schwarz: 4 * the largest squared
norm), so no metric meets inf or inf - inf.

Nothing in this file is measured on the code under test: the bound is the textbook one, derived at bound().
The last section holds what the two test files share on the oracle's side (the only part that imports it).
"""
import numpy as np

FMAX = float(np.float32(3.4028234663852886e38))
U = 2.0 ** -24          # unit roundoff of binary32
ETA = 2.0 ** -149       # smallest binary32 subnormal: an operation that lands among the subnormals errs by <= ETA / 2
COSINE_HALF, ONE_MINUS_DOT, L2 = 0, 1, 2


def _pad(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, dim = x.shape
    ld = (dim + 3) // 4 * 4
    out = np.zeros((n, ld), dtype=np.float32)
    out[:, :dim] = x
    return out


def _finish(rows, queries, overflow_ok=False):
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    assert np.isfinite(rows).all() and np.isfinite(queries).all()
    if not overflow_ok:
        big = max(float((rows.astype(np.float64) ** 2).sum(1).max()), float((queries.astype(np.float64) ** 2).sum(1).max()))
        # sum|a_i b_i| <= |a||b| and sum (a_i-b_i)^2 <= (|a|+|b|)^2 <= 4 max(|a|,|b|)^2
        assert 4.0 * big < FMAX, "a partial sum could exceed f32::MAX"
    return _pad(rows), queries


def lattice(n, dim, lo=-8, hi=8, nq=40, seed=0):
    """integer components in [lo, hi]: every product, difference and partial sum is an integer below 2^24, so any
    summation order, fused or not, is exact and the correctly rounded f64 result is THE answer of every kernel and
    every oracle mode.  Some rows are exact duplicates of earlier rows, some are all zero; some queries are rows."""
    assert dim * (hi - lo) ** 2 < 2 ** 24 and dim * max(abs(lo), abs(hi)) ** 2 < 2 ** 24
    rng = np.random.default_rng([seed, n, dim, hi - lo])
    rows = rng.integers(lo, hi + 1, size=(n, dim)).astype(np.float32)
    for i in range(5, n, 11):
        rows[i] = rows[i - 3]     # duplicates: equal distance to everything, the id decides
    rows[2::13] = 0.0             # all-zero rows: dot 0 with every query
    queries = rng.integers(lo, hi + 1, size=(nq, dim)).astype(np.float32)
    src = rows[:3 * (min(nq, n) // 4):3]
    queries[:len(src)] = src           # stored vectors as raw queries: L2 distance 0, duplicates tie at 0
    return _finish(rows, queries)


def scaled(n, dim, nq=40, seed=0):
    """Gaussian rows, each multiplied by 2^k, k uniform in [-12, 12] (exact: a power of two); queries the same.  Dot
    distances span large negative to large positive values."""
    rng = np.random.default_rng([seed, n, dim, 1])

    def make(m):
        x = rng.standard_normal((m, dim)).astype(np.float32)
        k = rng.integers(-12, 13, size=(m, 1))
        return x * np.exp2(k).astype(np.float32)

    return _finish(make(n), make(nq))


def cancelling(n, dim, nq=40, seed=0):
    """a query repeats one direction w in both halves; the second half of a row is the negated first half of the row
    times (1 + 2^-12 * noise): the dot cancels to about 1e-4 of sum|a_i*b_i|, so its bits depend on the summation order
    as much as they can"""
    rng = np.random.default_rng([seed, n, dim, 2])
    h = dim // 2
    s = np.float32(1.0 / np.sqrt(max(dim, 1)))
    rows = (rng.standard_normal((n, dim)) * 2.0 ** -12).astype(np.float32) * s  # components past 2h (odd dim, dim 1)
    a = rng.standard_normal((n, h)).astype(np.float32) * s
    rows[:, :h] = a
    rows[:, h:2 * h] = -a * (np.float32(1.0) + np.float32(2.0 ** -12) * rng.standard_normal((n, h)).astype(np.float32))
    queries = (rng.standard_normal((nq, dim)) * 2.0 ** -12).astype(np.float32) * s
    w = rng.standard_normal((nq, h)).astype(np.float32) * s
    queries[:, :h] = w
    queries[:, h:2 * h] = w
    return _finish(rows, queries)


def tiny(n, dim, nq=40, seed=0):
    """Gaussian rows times 1e-21: squares and products are subnormal, dot sums underflow.  Under the dot metrics every
    distance is 0.5 / 1.0 exactly (one tie over all rows); under L2 the distances are about 4e-20 * sqrt(dim / 768),
    built from subnormal squares -- zero wherever denormals are flushed"""
    rng = np.random.default_rng([seed, n, dim, 3])
    t = np.float32(1e-21)
    return _finish(rng.standard_normal((n, dim)).astype(np.float32) * t, rng.standard_normal((nq, dim)).astype(np.float32) * t)


def wide(n, dim, nq=40, seed=0):
    """within one row the magnitudes run from 2^-60 to 2^55 (random sign, mantissa in [1, 2), exponent uniform in
    [-60, 54]); no square or sum of squares overflows at dim <= 1536 (1536 * 4 * 2^110 < 2^128)"""
    assert dim <= 1536
    rng = np.random.default_rng([seed, n, dim, 4])

    def make(m):
        mant = (1.0 + rng.random((m, dim))).astype(np.float32)
        sign = np.where(rng.random((m, dim)) < 0.5, np.float32(-1.0), np.float32(1.0))
        return mant * sign * np.exp2(rng.integers(-60, 55, size=(m, dim))).astype(np.float32)

    return _finish(make(n), make(nq))


def l2_overflow(n, dim, nq=40, seed=0):
    """scaled() with about 2 % of the rows (half of them the nearest row of some query) and 2 of the queries replaced by vectors of components +-2^66: against an
    ordinary vector the first square of a difference already exceeds f32::MAX, so sum (a-b)^2 is +inf in every
    summation order; two such vectors differ by 0 or +-2^67 per component (distance 0 or +inf).  L2 only.  With finite
    inputs every difference is finite and every term is >= 0, so L2 cannot make a NaN; asserted below in f64, together
    with "no sum is near the threshold": each is below f32::MAX / 4 or has one term above 2^130.
    Returns the ids of the replaced rows and queries as well."""
    rows, queries = scaled(n, dim, nq, seed)
    rows = rows[:, :dim].copy()
    rng = np.random.default_rng([seed, n, dim, 5])

    def huge(m):
        return np.where(rng.random((m, dim)) < 0.5, np.float32(-1.0), np.float32(1.0)) * np.float32(2.0 ** 66)

    # half of them picked at random, half the nearest row of a query: a search of that query meets them for certain
    near = np.argmin(l2_sums64(rows, queries[::max(1, nq // max(1, n // 100))]), axis=1)
    big_rows = np.union1d(rng.choice(n, size=max(2, n // 100), replace=False), near)
    rows[big_rows] = huge(len(big_rows))
    big_q = np.array([1, nq - 2] if nq >= 4 else [0])
    queries[big_q] = huge(len(big_q))
    rows, queries = _finish(rows, queries, overflow_ok=True)
    for a in (queries, rows[big_rows, :dim]):  # every pair with a replaced vector on either side
        s = l2_sums64(rows, a)
        t = np.array([((rows[:, :dim].astype(np.float64) - x.astype(np.float64)) ** 2).max(1) for x in a])
        assert np.isfinite(s).all() and not np.isnan(s).any()  # f64 holds every sum
        assert ((s < FMAX / 4) | (t > 2.0 ** 130)).all()
    assert (l2_sums64(rows, queries) > FMAX).any()
    return rows, queries, big_rows, big_q


# ---------------------------------------------------------------- the reference
def _dim(rows, queries):
    return np.atleast_2d(queries).shape[1]


def l2_sums64(rows, queries):
    """[nq, n] float64: sum (q - r)^2"""
    q = np.atleast_2d(queries).astype(np.float64)
    r = rows[:, :q.shape[1]].astype(np.float64)
    out = np.empty((len(q), len(r)))
    for i in range(len(q)):
        out[i] = ((r - q[i]) ** 2).sum(1)
    return out


def ref64(rows, queries, metric):
    """[nq, n] float64: (1 - <q, r>) / 2, 1 - <q, r>, sqrt(sum (q - r)^2) with every operation in float64"""
    q = np.atleast_2d(queries).astype(np.float64)
    r = rows[:, :q.shape[1]].astype(np.float64)
    if metric == L2:
        return np.sqrt(l2_sums64(rows, queries))
    dot = q @ r.T
    return (1.0 - dot) / 2.0 if metric == COSINE_HALF else 1.0 - dot


def ref32(rows, queries, metric):
    """ref64 rounded once to f32 (float64 holds 2 * 24 + 2 bits and more, so for sqrt the double rounding is
    innocuous).  An L2 sum of squares above f32::MAX is +inf in f32 before the root is taken, so there the distance
    is +inf (l2_overflow keeps every sum far from that threshold, on one side or the other)"""
    with np.errstate(over="ignore"):
        d = ref64(rows, queries, metric).astype(np.float32)
    if metric == L2:
        d[l2_sums64(rows, queries) > FMAX] = np.inf
    return d


def bound(rows, queries, metric):
    """[nq, n] float64: a bound on |f32 result - ref64| for ANY summation order, fused or not.

    Model: fl(x op y) = (x op y)(1 + d) + e, |d| <= u = 2^-24, |e| <= 2^-150 (e only where the result is subnormal;
    sums and differences that land among the subnormals are exact).
      dot:  dim products and dim - 1 additions in any tree: |fl(dot) - dot| <= g * sum|a_i b_i| + dim * 2^-149 =: E,
            g = dim u / (1 - dim u).  Then fl(1 - r) errs by u |1 - r| <= u (|1 - dot| + E); halving is exact.
      L2:   a difference is one more rounding and enters squared: S' in [S (1 - g2) - e, S (1 + g2) + e],
            g2 = (dim + 2) u / (1 - (dim + 2) u), e = dim * 2^-149; the square root is correctly rounded: its
            image of that interval (the relative error halves) plus u on the result, plus 2^-149 should it be subnormal.
    The float64 reference's own error (dim * 2^-53 relative to the same sums) is added, so the bound holds against
    ref64 as computed, not only against the real number."""
    q = np.atleast_2d(queries).astype(np.float64)
    dim = q.shape[1]
    r = rows[:, :dim].astype(np.float64)
    eta = dim * ETA
    u64 = dim * 2.0 ** -53
    if metric == L2:
        g2 = (dim + 2) * U / (1.0 - (dim + 2) * U) + u64
        out = np.empty((len(q), len(r)))
        for i in range(len(q)):
            s = ((r - q[i]) ** 2).sum(1)
            hi = np.sqrt(s * (1.0 + g2) + eta)
            lo = np.sqrt(np.maximum(s * (1.0 - g2) - eta, 0.0))
            root = np.sqrt(s)
            out[i] = np.maximum(hi - root, root - lo) + U * hi + ETA
        return out
    g = dim * U / (1.0 - dim * U) + u64
    e = g * (np.abs(q) @ np.abs(r).T) + eta
    dot = q @ r.T
    b = e + U * (np.abs(1.0 - dot) + e)
    return b / 2.0 if metric == COSINE_HALF else b


def topk64(rows, queries, metric, k):
    """exact top k by (distance, id): the order every queue of the reference keeps (OrderedFloat, then id), on the
    distance it keeps -- ref64 rounded to f32 (-0.0 == +0.0).  -> ids [nq, k] u64, d [nq, k] f32"""
    d = ref32(rows, queries, metric)
    n = d.shape[1]
    ids = np.empty((len(d), k), dtype=np.uint64)
    out = np.empty((len(d), k), dtype=np.float32)
    idx = np.arange(n)
    for i in range(len(d)):
        order = np.lexsort((idx, d[i] + np.float32(0.0)))[:k]
        ids[i], out[i] = order, d[i][order]
    return ids, out


FAMILIES = {"lattice": lattice, "scaled": scaled, "cancelling": cancelling, "tiny": tiny, "wide": wide}


def make(family, n, dim, nq=40, seed=0):
    """(rows, queries) of a family by name; "lattice1" is the lattice on [-1, 1] (massive exact ties)"""
    if family == "lattice1":
        return lattice(n, dim, -1, 1, nq=nq, seed=seed)
    if family == "l2_overflow":
        return l2_overflow(n, dim, nq=nq, seed=seed)[:2]
    return FAMILIES[family](n, dim, nq=nq, seed=seed)


# ---------------------------------------------------------------- shared by the test files: the oracle's side
SMALL_BP = dict(order=6, neighborhood_size=6, zero_layer_neighborhood_size=12, max_link_rounds=1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle_matrix(rows, queries, metric, mode):
    """[nq, n] f32: every oracle distance, through one exhaustive orc_bruteforce (k = n) scattered back by id"""
    import oracle
    ix = oracle.Index(rows, dim=queries.shape[1], metric=metric)
    ids, d = ix.bruteforce(queries, rows.shape[0], sum_mode=mode)
    out = np.empty_like(d)
    np.put_along_axis(out, ids.astype(np.int64), d, axis=1)
    return out


def graph_over(rows, dim, metric, seed=1, **kw):
    """oracle.Index.generate in SUM_BLOCKED64 with small layers and one link round"""
    import oracle
    bp = oracle.default_build_params(seed=seed, **dict(SMALL_BP, **kw))
    return oracle.Index.generate(rows, np.arange(rows.shape[0]), bp, dim=dim, metric=metric, sum_mode=oracle.SUM_BLOCKED64)
