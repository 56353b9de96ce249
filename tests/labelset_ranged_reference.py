"""Yardstick of the searches by a SET of row labels AND a numeric range (phnsw_label_attr_count_set_device,
phnsw_search_*_labelset_ranged*): the per-query bitmaps a (set, range) stands for, in numpy, written from the contract in
include/phnsw.h and independent of parallel_hnsw_amd/hnsw.py.  Everything the calls return is measured against the
existing bitmap calls over masks_of's bitmaps.  It is the only yardstick of what a set with a range means."""
import numpy as np

LABEL_NONE = 0xFFFFFFFF
ATTR_NONE = 0xFFFFFFFF


def masks_of(labels, keys, want_sets, lo, hi, members=None):
    """bool [nq, n]: vector v is a candidate of query q iff it carries a label and a value (labels[v] != LABEL_NONE,
    keys[v] != ATTR_NONE), labels[v] is one of want_sets[q] (a sequence of u32 labels; LABEL_NONE in it matches nothing,
    a label twice counts once, an empty set holds nothing), lo[q] <= keys[v] <= hi[q] (u32 keys, both ends inclusive, one
    range per query; lo > hi: nothing) and, with `members` (bool [n]), the index holds v"""
    labels = np.asarray(labels, dtype=np.uint32).astype(np.int64)
    keys = np.asarray(keys, dtype=np.uint32).astype(np.int64)
    lo = np.asarray(lo, dtype=np.uint32).astype(np.int64)
    hi = np.asarray(hi, dtype=np.uint32).astype(np.int64)
    nq = len(want_sets)
    assert lo.shape == (nq,) and hi.shape == (nq,)
    listed = (labels != LABEL_NONE) & (keys != ATTR_NONE)
    if members is not None:
        listed &= np.asarray(members, dtype=bool)
    m = np.zeros((nq, len(labels)), dtype=bool)
    for q, s in enumerate(want_sets):
        wanted = np.array([int(x) & 0xFFFFFFFF for x in s if (int(x) & 0xFFFFFFFF) != LABEL_NONE], dtype=np.int64)
        m[q] = listed & np.isin(labels, wanted) & (keys >= lo[q]) & (keys <= hi[q])
    return m
