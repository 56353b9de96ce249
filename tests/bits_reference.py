"""The bits row store restated in numpy: the sign rule, the packing, the Hamming distance h, the three metrics and the
re-rank.  The tests compare the device's words, rows and distances with these, bit for bit."""
import numpy as np

METRIC_COSINE_HALF, METRIC_ONE_MINUS_DOT, METRIC_L2 = 0, 1, 2


def sign_bits(x):
    """bit j = x[j] < 0.0f: +0, -0 and every non-negative value give 0 (NaN, which no row holds, gives 0 too)"""
    return (np.asarray(x, dtype=np.float32) < np.float32(0.0)).astype(np.uint8)


def pack(x):
    """[n, dim] f32 -> [n, ceil(dim / 32)] uint32: component j is bit j & 31 of word j >> 5, padding bits 0"""
    b = sign_bits(np.atleast_2d(x))
    n, dim = b.shape
    nw = (dim + 31) // 32
    padded = np.zeros((n, nw * 32), dtype=np.uint8)
    padded[:, :dim] = b
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (padded.reshape(n, nw, 32).astype(np.uint64) * weights).sum(axis=2).astype(np.uint32)


def unpack(words, dim):
    """the rows phnsw_store_read returns: +1.0f for bit 0, -1.0f for bit 1, [n, dim]"""
    words = np.atleast_2d(words).astype(np.uint32)
    j = np.arange(dim)
    b = (words[:, j >> 5] >> (j & 31).astype(np.uint32)) & np.uint32(1)
    return np.where(b == 1, np.float32(-1.0), np.float32(1.0)).astype(np.float32)


def signed_query(q):
    """the f32 query the bit distance corresponds to: where(q < 0, -1, +1)"""
    return np.where(sign_bits(q) == 1, np.float32(-1.0), np.float32(1.0)).astype(np.float32)


_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint32)


def hamming(words_a, words_b):
    """popcount(a XOR b) over the words: [..., nw] x [..., nw] -> [...] uint32"""
    x = np.bitwise_xor(np.asarray(words_a, dtype=np.uint32), np.asarray(words_b, dtype=np.uint32))
    x = np.ascontiguousarray(x)
    return _POP8[x.view(np.uint8).reshape(x.shape + (4,))].sum(axis=(-1, -2)).astype(np.uint32)


def distance(h, dim, metric):
    """ph_bits_distance: r = dim - 2 h (dot metrics) or 4 h (L2) as f32, then the metric's last step in f32"""
    h = np.asarray(h, dtype=np.int64)
    if metric == METRIC_L2:
        return np.sqrt((4 * h).astype(np.float32)).astype(np.float32)
    r = (dim - 2 * h).astype(np.float32)
    if metric == METRIC_COSINE_HALF:
        return ((np.float32(1.0) - r) / np.float32(2.0)).astype(np.float32)
    return (np.float32(1.0) - r).astype(np.float32)


def distances(rows_words, query_words, dim, metric):
    """[n, nw] rows against one query's words -> [n] f32"""
    return distance(hamming(rows_words, np.asarray(query_words)[None, :]), dim, metric)


def rerank(ids, lens, full_d, k):
    """the re-ranked search: of row q's first lens[q] ids, with their f32 distances full_d[q], the k smallest by
    (distance, id).  -> ids [nq, k] (0xFFFF... padded), d [nq, k], len [nq]; the distance order is the total order of
    the search queues (-0.0 == +0.0, then the id)"""
    nq = len(ids)
    out_ids = np.full((nq, k), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    out_d = np.full((nq, k), np.finfo(np.float32).max, dtype=np.float32)
    out_len = np.zeros(nq, dtype=np.uint64)
    for q in range(nq):
        m = int(lens[q])
        i, d = np.asarray(ids[q][:m], dtype=np.uint64), np.asarray(full_d[q][:m], dtype=np.float32) + np.float32(0.0)
        order = np.lexsort((i, d))[:k]
        out_ids[q, :len(order)] = i[order]
        out_d[q, :len(order)] = np.asarray(full_d[q][:m], dtype=np.float32)[order]
        out_len[q] = len(order)
    return out_ids, out_d, out_len


def bit_edge_rows(dim):
    """rows whose sign bits sit on every edge of the rule and of the layout"""
    tiny = np.float32(2.0 ** -149)
    rows = [np.zeros(dim, dtype=np.float32),                      # all zero: no bit
            np.full(dim, -0.0, dtype=np.float32),                 # -0.0 is not below zero: no bit
            np.full(dim, tiny, dtype=np.float32),                 # positive subnormals: no bit
            np.full(dim, -tiny, dtype=np.float32),                # negative subnormals: every bit
            np.full(dim, -1.0, dtype=np.float32)]
    edges = sorted({0, dim - 1} | {j for w in range(32, dim, 32) for j in (w - 1, w)})
    for j in edges:                                               # one negative component, at every word boundary
        r = np.ones(dim, dtype=np.float32)
        r[j] = -3.0
        rows.append(r)
    return np.stack(rows)
