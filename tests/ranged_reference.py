"""Yardstick of the searches by a numeric range (phnsw_attr_*, phnsw_search_*_ranged): the order-preserving key maps
and the per-query bitmaps a range stands for, in numpy, written from the contract in include/phnsw.h and independent of
parallel_hnsw_amd/hnsw.py.  Everything the range calls return is measured against the existing bitmap calls over
masks_of's bitmaps."""
import struct

import numpy as np

ATTR_NONE = 0xFFFFFFFF


def keys_of(values):
    """u32 keys whose unsigned order is the order of `values` (uint32, int32 or float32), one value at a time"""
    a = np.asarray(values)
    flat = a.reshape(-1)
    out = np.empty(len(flat), dtype=np.uint32)
    if a.dtype == np.uint32:
        for i, x in enumerate(flat.tolist()):
            if x == ATTR_NONE:
                raise ValueError("index %d: 0xFFFFFFFF is no value" % i)
            out[i] = x
    elif a.dtype == np.int32:
        for i, x in enumerate(flat.tolist()):
            out[i] = (x + 2 ** 31) & 0xFFFFFFFF  # x ^ 0x80000000 on the two's complement bits
    elif a.dtype == np.float32:
        for i, x in enumerate(flat.tolist()):
            if x != x:
                raise ValueError("index %d: NaN" % i)
            if x == 0.0:
                x = 0.0  # -0.0 -> +0.0
            (bits,) = struct.unpack("<I", struct.pack("<f", x))
            out[i] = (~bits & 0xFFFFFFFF) if bits >> 31 else (bits | 0x80000000)
    else:
        raise TypeError("uint32, int32 or float32, got %s" % a.dtype)
    return out.reshape(a.shape)


def masks_of(keys, lo, hi, members=None):
    """bool [nq, n]: vector v is a candidate of query q iff keys[v] is a value (not ATTR_NONE), lo[q] <= keys[v] <= hi[q]
    (u32 keys, both ends inclusive; lo > hi: nothing) and, with `members` (bool [n]), the index holds v"""
    keys = np.asarray(keys, dtype=np.uint32).astype(np.int64)
    lo = np.asarray(lo, dtype=np.uint32).astype(np.int64)
    hi = np.asarray(hi, dtype=np.uint32).astype(np.int64)
    m = (keys[None, :] >= lo[:, None]) & (keys[None, :] <= hi[:, None]) & (keys[None, :] != ATTR_NONE)
    if members is not None:
        m &= np.asarray(members, dtype=bool)[None, :]
    return m
