"""phnsw_search_exact_radius_labeled / _ranged restated in numpy: per query, radius_reference.exact_radius with THAT
query's own allow mask -- the listed vectors of its label, or the listed vectors inside its key range.  The distances
come from the caller, as there; nothing here computes one."""
import numpy as np

import radius_reference as rr

NONE = 0xFFFFFFFF  # PHNSW_LABEL_NONE, PHNSW_ATTR_NONE


def label_masks(labels, want, members=None):
    """bool [nq, n]: v is listed under want[q] -- labels[v] == want[q], the label is not NONE, v is in the index"""
    labels = np.asarray(labels, dtype=np.uint32)
    want = np.asarray(want, dtype=np.int64) & 0xFFFFFFFF
    m = (labels[None, :] == want[:, None].astype(np.uint32)) & (labels != NONE)[None, :]
    return m if members is None else m & np.asarray(members, dtype=bool)[None, :]


def range_masks(keys, lo, hi, members=None):
    """bool [nq, n]: v is listed (a key that is not NONE, in the index) and lo[q] <= keys[v] <= hi[q]; lo > hi: nothing"""
    keys = np.asarray(keys, dtype=np.uint32).astype(np.int64)
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    m = (keys[None, :] >= lo[:, None]) & (keys[None, :] <= hi[:, None]) & (keys != NONE)[None, :]
    return m if members is None else m & np.asarray(members, dtype=bool)[None, :]


def by_masks(D, radius, masks, exclude=None):
    """-> first[nq + 1] u64, ids[total] u64, d[total] f32: query by query, exact_radius over the query's own mask"""
    D = np.asarray(D, dtype=np.float32)
    nq = D.shape[0]
    r = rr.radii(radius, nq)
    first = np.zeros(nq + 1, dtype=np.uint64)
    ids, d = [np.zeros(0, np.uint64)], [np.zeros(0, np.float32)]
    for q in range(nq):
        e = None if exclude is None else exclude[q:q + 1]
        _, i, x = rr.exact_radius(D[q:q + 1], r[q:q + 1], masks[q], e)
        ids.append(i)
        d.append(x)
        first[q + 1] = first[q] + np.uint64(len(i))
    return first, np.concatenate(ids), np.concatenate(d)


def exact_radius_labeled(D, radius, labels, want, exclude=None, members=None):
    return by_masks(D, radius, label_masks(labels, want, members), exclude)


def exact_radius_ranged(D, radius, keys, lo, hi, exclude=None, members=None):
    return by_masks(D, radius, range_masks(keys, lo, hi, members), exclude)
