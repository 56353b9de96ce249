"""phnsw_search_exact_filtered restated in numpy: the k candidates with the smallest (distance, id).  The distances come
from the caller (a matrix D[nq, n] made by a yardstick that is not the code under test), so nothing here computes one."""
import numpy as np

EMPTY = 0xFFFFFFFFFFFFFFFF
FMAX = np.float32(3.4028234663852886e38)


def candidates(n, allow=None, exclude=None, members=None, q=0):
    """bool [n]: v is a candidate of query q iff its bit is set (allow: bool [n] or [nq, n], None = all), it is in the
    index (members: bool [n], None = all) and it is not exclude[q]"""
    c = np.ones(n, dtype=np.bool_) if allow is None else np.array(allow if np.ndim(allow) == 1 else allow[q], dtype=np.bool_)
    if members is not None:
        c &= np.asarray(members, dtype=np.bool_)
    if exclude is not None and int(exclude[q]) < n:
        c[int(exclude[q])] = False
    return c


def exact_topk(D, allow=None, exclude=None, members=None, k=10):
    """-> ids[nq, k] u64, d[nq, k] f32, len[nq] u64: ascending (D, id) by a stable sort over ascending ids, padded"""
    D = np.asarray(D, dtype=np.float32)
    nq, n = D.shape
    ids = np.full((nq, k), EMPTY, dtype=np.uint64)
    d = np.full((nq, k), FMAX, dtype=np.float32)
    ln = np.zeros(nq, dtype=np.uint64)
    for q in range(nq):
        v = np.nonzero(candidates(n, allow, exclude, members, q))[0]
        v = v[np.argsort(D[q, v], kind="stable")][:k]
        ids[q, :len(v)], d[q, :len(v)], ln[q] = v, D[q, v], len(v)
    return ids, d, ln
