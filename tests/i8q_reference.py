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


def lattice(n, dim, rng, k_range=12):
    """rows c * 2^k: integer codes c in [-127, 127] with one component per row forced to +-127, a per-row power of two
    with k in [-k_range, k_range].  quantize() returns exactly (c, 2^k) for them.  -> rows f32, c int8, k"""
    c = np.clip(np.rint(40.0 * rng.standard_normal((n, dim))), -127, 127).astype(np.int32)
    c[np.arange(n), rng.integers(0, dim, size=n)] = np.where(rng.integers(0, 2, size=n) == 1, 127, -127)
    k = rng.integers(-k_range, k_range + 1, size=n)
    rows = (c.astype(np.float64) * np.exp2(k.astype(np.float64))[:, None]).astype(np.float32)
    return rows, c.astype(np.int8), k
