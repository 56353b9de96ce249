"""Yardstick of the searches by a row label AND a numeric range (phnsw_label_attr_*, phnsw_search_*_label_ranged): the
per-query bitmaps a (label, range) pair stands for, in numpy, written from the contract in include/phnsw.h and
independent of parallel_hnsw_amd/hnsw.py.  Everything the calls return is measured against the existing bitmap calls
over masks_of's bitmaps.  It is the only yardstick of what a pair means."""
import numpy as np

LABEL_NONE = 0xFFFFFFFF
ATTR_NONE = 0xFFFFFFFF


def masks_of(labels, keys, want, lo, hi, members=None):
    """bool [nq, n]: vector v is a candidate of query q iff it carries a label and a value (labels[v] != LABEL_NONE,
    keys[v] != ATTR_NONE), labels[v] == want[q], lo[q] <= keys[v] <= hi[q] (u32 keys, both ends inclusive; lo > hi:
    nothing; want == LABEL_NONE: nothing) and, with `members` (bool [n]), the index holds v"""
    labels = np.asarray(labels, dtype=np.uint32).astype(np.int64)
    keys = np.asarray(keys, dtype=np.uint32).astype(np.int64)
    want = np.asarray(want, dtype=np.uint32).astype(np.int64)
    lo = np.asarray(lo, dtype=np.uint32).astype(np.int64)
    hi = np.asarray(hi, dtype=np.uint32).astype(np.int64)
    listed = (labels != LABEL_NONE) & (keys != ATTR_NONE)
    m = (labels[None, :] == want[:, None]) & (keys[None, :] >= lo[:, None]) & (keys[None, :] <= hi[:, None]) & listed[None, :]
    m &= (want != LABEL_NONE)[:, None]
    if members is not None:
        m &= np.asarray(members, dtype=bool)[None, :]
    return m
