"""Host-side mirror of the reference crate's public surface for the hot path
(terminusdb-labs/parallel-hnsw src/lib.rs:585-1686, src/parameters.rs, src/types.rs),
implemented over the C ABI of libphnsw.  Names, argument meaning and result ordering
follow the reference so tests read like its own tests:

    Hnsw.generate(c, vs, bp)            lib.rs:825-830
    hnsw.search(AbstractVector, sp)     lib.rs:663-665   -> [(VectorId, f32)] sorted (d, id)
    hnsw.improve_index(bp)              lib.rs:1664-1669
    hnsw.knn(k, probe_depth)            lib.rs:905-928
    hnsw.layers[i].nodes / .neighbors   lib.rs:85-91  (top first)

`VectorStore` plays the role of the Comparator (store + metric, bigvec.rs:38-57); the
per-pair compare_raw seam is replaced by batches (distance_batch / search_batch).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import BuildParams, OptimizationParams, PhnswError, SearchParams, check, lib

EMPTY = 0xFFFFFFFFFFFFFFFF  # VectorId::MAX / NodeId::MAX (types.rs:8-13)
METRIC_COSINE_HALF, METRIC_ONE_MINUS_DOT, METRIC_L2 = 0, 1, 2


def stream_create_beside(device=0, other_stream=0):
    """phnsw_stream_create_beside: a non-blocking hipStream_t (as an integer) that was seen to run beside `other_stream`
    (0 = the default stream) -- the second lane of a caller that keeps two batches in flight.  Streams that share a
    hardware queue do not overlap; hipStreamDestroy is the caller's."""
    import ctypes
    out = ctypes.c_void_p()
    check(lib().phnsw_stream_create_beside(int(device), ctypes.c_void_p(int(other_stream) or None), ctypes.byref(out)))
    return int(out.value or 0)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


FILTER_STRICT = 1  # PHNSW_FILTER_STRICT
FILTER_ALL = 0xFFFFFFFF  # PHNSW_FILTER_ALL: a selector of search_exact_grouped that names no bitmap
ROUTE_GRAPH, ROUTE_SCAN, ROUTE_GRAPH_THEN_SCAN = 0, 1, 2  # PHNSW_ROUTE_*
LABEL_NONE = 0xFFFFFFFF  # PHNSW_LABEL_NONE: a vector that is not listed; a wanted label with an empty row
COLLECT_EXTEND = 1  # PHNSW_COLLECT_EXTEND: a hop that improved the kept rows counts as one that did something


def pack_allow(allow, n, nq):
    """the allow-list of a filtered search as phnsw.h wants it -> (u32 words or None, filter_stride_words): bit v % 32 of
    word v // 32 set = VectorId v may be returned.  A bool array [n] is one bitmap for all queries (stride 0), [nq, n] one
    per query (stride ceil(n/32)); u32 arrays are taken as already packed ([>= ceil(n/32)] or [nq, stride])"""
    if allow is None:
        return None, 0
    a = np.asarray(allow)
    nw = (int(n) + 31) // 32
    if a.dtype == np.bool_:
        if a.ndim not in (1, 2) or a.shape[-1] != n or (a.ndim == 2 and a.shape[0] != nq):
            raise ValueError("allow: a bool array of shape [n] or [nq, n] (n = %d, nq = %d), got %r" % (n, nq, a.shape))
        rows = np.zeros((a.shape[0] if a.ndim == 2 else 1, nw * 32), dtype=np.bool_)  # bits at or past n stay clear
        rows[:, :n] = a
        words = np.ascontiguousarray(np.packbits(rows, axis=1, bitorder="little")).view("<u4")
        return (words, nw) if a.ndim == 2 else (words.reshape(-1), 0)
    if a.dtype != np.uint32:
        raise TypeError("allow: a bool mask or packed uint32 words, got %s" % a.dtype)
    if a.ndim not in (1, 2) or a.shape[-1] < nw or (a.ndim == 2 and a.shape[0] != nq):
        raise ValueError("allow: packed words of shape [>= %d] or [%d, >= %d], got %r" % (nw, nq, nw, a.shape))
    a = np.ascontiguousarray(a)
    return (a, a.shape[1]) if a.ndim == 2 else (a, 0)


def pack_allow_table(allows, n):
    """the bitmap table of search_exact_grouped as phnsw.h wants it -> (u32 words [nb, stride], stride): a bool array
    [nb, n] is packed (bits at or past n clear, stride ceil(n/32)); a u32 array [nb, >= ceil(n/32)] is taken as already
    packed, its row length the stride"""
    if allows is None:
        raise ValueError("allows: a table of bitmaps, bool [nb, n] or packed uint32 [nb, >= ceil(n/32)], is required")
    a = np.asarray(allows)
    nw = (int(n) + 31) // 32
    if a.dtype == np.bool_:
        if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != n:
            raise ValueError("allows: a bool array of shape [nb >= 1, n] (n = %d), got %r" % (n, a.shape))
        rows = np.zeros((a.shape[0], nw * 32), dtype=np.bool_)
        rows[:, :n] = a
        return np.ascontiguousarray(np.packbits(rows, axis=1, bitorder="little")).view("<u4"), nw
    if a.dtype != np.uint32:
        raise TypeError("allows: a bool mask table or packed uint32 words, got %s" % a.dtype)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < nw:
        raise ValueError("allows: packed words of shape [nb >= 1, >= %d], got %r" % (nw, a.shape))
    a = np.ascontiguousarray(a)
    return a, a.shape[1]


def pack_allow_of(allow_of, nq):
    """the selectors of search_exact_grouped -> u32 [nq]: integers, -1 or FILTER_ALL = no bitmap"""
    if allow_of is None:
        raise ValueError("allow_of: one selector per query is required")
    a = np.asarray(allow_of)
    if a.dtype.kind not in "iu":
        raise TypeError("allow_of: an integer array, got %s" % a.dtype)
    if a.ndim != 1 or a.shape[0] != nq:
        raise ValueError("allow_of: an integer array of shape [nq] (nq = %d), got %r" % (nq, a.shape))
    a = a.astype(np.int64)
    if ((a < -1) | (a > FILTER_ALL)).any():
        raise ValueError("allow_of: selectors are bitmap numbers, -1 or FILTER_ALL")
    a[a == -1] = FILTER_ALL
    return np.ascontiguousarray(a, dtype=np.uint32)


def pack_labels(values, count, what):
    """labels of Labels / wanted labels of search_exact_labeled -> u32 [count]: integers within u32, -1 or LABEL_NONE =
    none"""
    if values is None:
        raise ValueError("%s: an integer array of shape [%d] is required" % (what, count))
    a = np.asarray(values)
    if a.dtype.kind not in "iu":
        raise TypeError("%s: an integer array, got %s" % (what, a.dtype))
    if a.ndim != 1 or a.shape[0] != count:
        raise ValueError("%s: an integer array of shape [%d], got %r" % (what, count, a.shape))
    if a.dtype != np.uint32:
        if a.dtype == np.uint64:
            if (a > LABEL_NONE).any():
                raise ValueError("%s: labels are 32-bit values, -1 or LABEL_NONE" % what)
        else:
            a = a.astype(np.int64)
            if ((a < -1) | (a > LABEL_NONE)).any():
                raise ValueError("%s: labels are 32-bit values, -1 or LABEL_NONE" % what)
            a[a == -1] = LABEL_NONE
    return np.ascontiguousarray(a, dtype=np.uint32)


LABELSET_NWANT_MAX = 0x7FFFFFFE  # wanted labels of one call by label sets


def pack_label_sets(want, nq):
    """the sets of wanted labels of search_exact_labelset -> CSR (first u32 [nq + 1], values u32 [nwant]): query i wants
    values[first[i]:first[i + 1]].  want: a sequence of nq integer sequences (empty ones included), or a ready (first,
    values) pair of arrays.  Values as pack_labels takes them: within u32, -1 or LABEL_NONE = none"""
    if want is None:
        raise ValueError("want: %d sets of labels are required" % nq)
    ready = (isinstance(want, tuple) and len(want) == 2 and all(isinstance(x, np.ndarray) for x in want))
    if ready:
        first, values = want
        if first.dtype.kind not in "iu":
            raise TypeError("want: integer offsets, got %s" % first.dtype)
        if first.ndim != 1 or first.shape[0] != nq + 1:
            raise ValueError("want: offsets of shape [%d] (nq + 1), got %r" % (nq + 1, first.shape))
        first = first.astype(np.int64)
    else:
        sets = list(want)
        if len(sets) != nq:
            raise ValueError("want: %d sets of labels (one per query), got %d" % (nq, len(sets)))
        rows = []
        for i, s in enumerate(sets):
            if np.ndim(s) != 1:
                raise ValueError("want: set %d is not a sequence of labels" % i)
            rows.append(np.asarray(s) if len(s) else np.zeros(0, dtype=np.int64))
        first = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum([len(r) for r in rows], out=first[1:])
        for i, r in enumerate(rows):
            if r.dtype.kind not in "iu":
                raise TypeError("want: set %d: integer labels, got %s" % (i, r.dtype))
        if any(r.dtype == np.uint64 and (r > LABEL_NONE).any() for r in rows):
            raise ValueError("want: labels are 32-bit values, -1 or LABEL_NONE")
        values = np.concatenate([r.astype(np.int64) for r in rows]) if rows else np.zeros(0, dtype=np.int64)
    if first[0] != 0 or (np.diff(first) < 0).any():
        bad = 0 if first[0] != 0 else int(np.flatnonzero(np.diff(first) < 0)[0])
        raise ValueError("want: offsets start at 0 and never run backwards (query %d)" % bad)
    if first[-1] > LABELSET_NWANT_MAX:
        raise ValueError("want: at most 2^31 - 2 wanted labels in one call")
    values = pack_labels(values, int(first[-1]), "want values")
    return np.ascontiguousarray(first, dtype=np.uint32), values


ATTR_NONE = 0xFFFFFFFF  # PHNSW_ATTR_NONE: a row that carries no value


def attr_keys(values, what="values"):
    """a numeric column (or bounds) -> the u32 keys of Attribute, whose unsigned order is the values' order (phnsw.h,
    "VALUE TYPES"): uint32 as it is, int32 x ^ 0x80000000, float32 with -0.0 made +0.0, then bits | 0x80000000 for a
    value that is not negative and ~bits for a negative one.  NaN has no place in an order and a uint32 0xFFFFFFFF cannot
    be told from ATTR_NONE: both are a ValueError naming the first index.  Other dtypes are a TypeError (64-bit columns
    are out of scope)"""
    a = np.asarray(values)
    if a.dtype == np.uint32:
        bad = np.flatnonzero(a.reshape(-1) == ATTR_NONE)
        if len(bad):
            raise ValueError("%s: index %d: 0xFFFFFFFF is ATTR_NONE, not a uint32 value" % (what, int(bad[0])))
        return np.ascontiguousarray(a)
    if a.dtype == np.int32:
        return np.ascontiguousarray(a).view(np.uint32) ^ np.uint32(0x80000000)
    if a.dtype == np.float32:
        bad = np.flatnonzero(np.isnan(a.reshape(-1)))
        if len(bad):
            raise ValueError("%s: index %d: NaN has no place in an order" % (what, int(bad[0])))
        bits = np.ascontiguousarray(a + np.float32(0.0)).view(np.uint32)  # -0.0 + 0.0 = +0.0
        neg = (bits >> np.uint32(31)).astype(bool)
        return np.where(neg, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    raise TypeError("%s: a uint32, int32 or float32 array, got %s" % (what, a.dtype))


class Attribute:
    """phnsw_attr: one numeric value per vector of `hnsw`'s store, sorted once on the device by (key, id), so that every
    range lo <= value <= hi is one contiguous span (twelve bytes per vector).  values: a uint32, int32 or float32 array
    [n] (attr_keys maps it; the dtype is remembered and bounds are given in it); missing: a bool mask [n], True = the row
    carries no value.  A vector is listed iff it has a value and the index's bottom layer holds it.  The handle is a
    snapshot like Labels: after store.append, or with another index, the calls refuse it as stale.  Keep `hnsw` alive
    while it is used.  search_exact_ranged, search_batch_ranged and search_ranged take it."""

    def __init__(self, hnsw, values, missing=None):
        self._h = None
        if not isinstance(hnsw, Hnsw):
            raise TypeError("Attribute: hnsw must be an Hnsw")
        n = int(hnsw.store.n)
        if values is None:
            raise ValueError("Attribute: values: an array of shape [%d] is required" % n)
        a = np.asarray(values)
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError("Attribute: values: an array of shape [%d], got %r" % (n, a.shape))
        if missing is not None:
            m = np.asarray(missing)
            if m.dtype != np.bool_ or m.shape != a.shape:
                raise ValueError("Attribute: missing: a bool mask of shape [%d], got %s %r" % (n, m.dtype, m.shape))
            a = a.copy()
            a[m] = 0  # whatever stood there (a NaN, 0xFFFFFFFF) is no value
        keys = attr_keys(a, "Attribute: values").copy()
        bad = np.flatnonzero(keys == ATTR_NONE)  # int32: 2**31 - 1 maps onto it (as a bound: "no upper end")
        if len(bad):
            raise ValueError("Attribute: values: index %d: %r maps onto ATTR_NONE; mark the row missing" % (int(bad[0]), a[bad[0]]))
        if missing is not None:
            keys[m] = ATTR_NONE
        h = C.c_void_p()
        check(lib().phnsw_attr_create(hnsw._h, _p(keys), len(keys), C.byref(h)))
        self._h, self.hnsw, self.dtype = h, hnsw, a.dtype

    @classmethod
    def from_device(cls, hnsw, ptr, dtype=np.uint32, stream=0):
        """phnsw_attr_create_device: ptr = u32 KEYS [store n] in device memory (an integer; mapped already, ATTR_NONE =
        no value), read on `stream`, which is synchronised.  dtype: what key() maps bounds from"""
        if not isinstance(hnsw, Hnsw):
            raise TypeError("Attribute.from_device: hnsw must be an Hnsw")
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.uint32), np.dtype(np.int32), np.dtype(np.float32)):
            raise TypeError("Attribute.from_device: dtype uint32, int32 or float32, got %s" % dtype)
        self = cls.__new__(cls)
        self._h = None
        h = C.c_void_p()
        check(lib().phnsw_attr_create_device(hnsw._h, C.c_void_p(ptr or None), int(hnsw.store.n), C.c_void_p(stream or None),
                                             C.byref(h)))
        self._h, self.hnsw, self.dtype = h, hnsw, dtype
        return self

    def key(self, x):
        """the u32 key of a bound given in the column's dtype (a scalar or an array)"""
        return attr_keys(np.asarray(x).astype(self.dtype, copy=False), "bound")

    def bounds(self, call, lo, hi, nq):
        """lo / hi of a call -> u32 keys [nq] each: a scalar is broadcast, an array is [nq] in the column's dtype, None
        is an open end.  Errors name the call and the first offending query"""
        out = []
        for name, b, open_end in (("lo", lo, 0), ("hi", hi, ATTR_NONE)):
            if b is None:
                out.append(np.full(nq, open_end, dtype=np.uint32))
                continue
            a = np.asarray(b)
            if a.ndim == 0:
                a = np.full(nq, a[()])
            if a.ndim != 1 or a.shape[0] != nq:
                raise ValueError("%s: %s: a scalar or an array of shape [%d], got %r" % (call, name, nq, a.shape))
            if a.dtype.kind not in "iuf" or (a.dtype.kind == "f") != (self.dtype.kind == "f"):
                raise TypeError("%s: %s: bounds in the column's dtype %s, got %s" % (call, name, self.dtype, a.dtype))
            if a.dtype != self.dtype:
                c = a.astype(self.dtype)
                bad = np.flatnonzero(~((c == a) | ((a != a) & (c != c))))
                if len(bad):
                    raise ValueError("%s: %s: query %d: %r is not a value of dtype %s" % (call, name, int(bad[0]), a[bad[0]],
                                                                                         self.dtype))
                a = c
            try:
                out.append(np.ascontiguousarray(attr_keys(a, name), dtype=np.uint32))
            except ValueError as e:
                raise ValueError("%s: %s" % (call, str(e).replace("index", "query"))) from None
        return out[0], out[1]

    def info(self):
        """(n, listed, key_min, key_max): the vector count the handle was made for, the listed vectors, the smallest and
        the largest KEY (0xFFFFFFFF and 0 when nothing is listed)"""
        a, b = C.c_uint64(), C.c_uint64()
        c, d = C.c_uint32(), C.c_uint32()
        check(lib().phnsw_attr_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return int(a.value), int(b.value), int(c.value), int(d.value)

    listed = property(lambda self: self.info()[1])

    def count_device(self, nq, lo, hi, out_count, stream=0):
        """phnsw_attr_count_device: device pointers as integers, u32 [nq] each (lo and hi are KEYS); enqueued"""
        check(lib().phnsw_attr_count_device(self._h, C.c_void_p(lo or None), C.c_void_p(hi or None), int(nq),
                                            C.c_void_p(out_count or None), C.c_void_p(stream or None)))

    def count(self, lo, hi):
        """the candidates of every range, u32 [nq] (0 where lo > hi): filter_count's figure for the equivalent bitmaps.
        lo / hi as the searches take them, at least one an array.  Host convenience over count_device (needs torch)"""
        import torch
        nq = max([len(np.atleast_1d(x)) for x in (lo, hi) if x is not None] or [1])
        l32, h32 = self.bounds("Attribute.count", lo, hi, nq)
        dev = torch.device("cuda", getattr(self.hnsw.store, "device", 0))
        ld = torch.from_numpy(l32.view(np.int32)).to(dev)
        hd = torch.from_numpy(h32.view(np.int32)).to(dev)
        out = torch.zeros(max(nq, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.count_device(nq, ld.data_ptr(), hd.data_ptr(), out.data_ptr())
        torch.cuda.synchronize(dev)
        return out.cpu().numpy().view(np.uint32)[:nq]

    def close(self):
        if getattr(self, "_h", None):
            lib().phnsw_attr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LabeledAttribute:
    """phnsw_label_attr: one label AND one numeric value per vector of `hnsw`'s store, sorted once on the device by the
    composite (label << 32) | key, then by id, so that every pair (label, lo <= value <= hi) is one contiguous span
    (twenty bytes per vector).  labels: as Labels takes them (integers within u32, -1 or LABEL_NONE = none); values and
    missing: as Attribute takes them.  A vector is listed iff it has a label AND a value and the index's bottom layer
    holds it.  The handle is a snapshot like Labels and Attribute.  Keep `hnsw` alive while it is used.
    search_exact_label_ranged, search_batch_label_ranged and search_label_ranged take it, and so do their forms for a
    SET of labels with one range per query: search_exact_labelset_ranged, search_batch_labelset_ranged and
    search_labelset_ranged."""

    def __init__(self, hnsw, labels, values, missing=None):
        self._h = None
        if not isinstance(hnsw, Hnsw):
            raise TypeError("LabeledAttribute: hnsw must be an Hnsw")
        n = int(hnsw.store.n)
        lab = pack_labels(labels, n, "LabeledAttribute: labels")
        if values is None:
            raise ValueError("LabeledAttribute: values: an array of shape [%d] is required" % n)
        a = np.asarray(values)
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError("LabeledAttribute: values: an array of shape [%d], got %r" % (n, a.shape))
        if missing is not None:
            m = np.asarray(missing)
            if m.dtype != np.bool_ or m.shape != a.shape:
                raise ValueError("LabeledAttribute: missing: a bool mask of shape [%d], got %s %r" % (n, m.dtype, m.shape))
            a = a.copy()
            a[m] = 0  # whatever stood there (a NaN, 0xFFFFFFFF) is no value
        keys = attr_keys(a, "LabeledAttribute: values").copy()
        bad = np.flatnonzero(keys == ATTR_NONE)  # int32: 2**31 - 1 maps onto it (as a bound: "no upper end")
        if len(bad):
            raise ValueError("LabeledAttribute: values: index %d: %r maps onto ATTR_NONE; mark the row missing"
                             % (int(bad[0]), a[bad[0]]))
        if missing is not None:
            keys[m] = ATTR_NONE
        h = C.c_void_p()
        check(lib().phnsw_label_attr_create(hnsw._h, _p(lab), _p(keys), len(keys), C.byref(h)))
        self._h, self.hnsw, self.dtype = h, hnsw, a.dtype

    @classmethod
    def from_device(cls, hnsw, labels_ptr, keys_ptr, dtype=np.uint32, stream=0):
        """phnsw_label_attr_create_device: labels_ptr = u32 labels, keys_ptr = u32 KEYS, [store n] each in device memory
        (integers; LABEL_NONE = no label, ATTR_NONE = no value), read on `stream`, which is synchronised.  dtype: what
        key() maps bounds from"""
        if not isinstance(hnsw, Hnsw):
            raise TypeError("LabeledAttribute.from_device: hnsw must be an Hnsw")
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.uint32), np.dtype(np.int32), np.dtype(np.float32)):
            raise TypeError("LabeledAttribute.from_device: dtype uint32, int32 or float32, got %s" % dtype)
        self = cls.__new__(cls)
        self._h = None
        h = C.c_void_p()
        check(lib().phnsw_label_attr_create_device(hnsw._h, C.c_void_p(labels_ptr or None), C.c_void_p(keys_ptr or None),
                                                   int(hnsw.store.n), C.c_void_p(stream or None), C.byref(h)))
        self._h, self.hnsw, self.dtype = h, hnsw, dtype
        return self

    key = Attribute.key        # the u32 key of a bound given in the column's dtype
    bounds = Attribute.bounds  # lo / hi of a call -> u32 keys [nq] each, Attribute's rules

    @staticmethod
    def wanted(call, want, nq):
        """want of a call -> u32 labels [nq]: a scalar is broadcast, an array is [nq]; -1 or LABEL_NONE = none (an empty
        row).  Errors name the call and the first offending query"""
        if want is None:
            raise ValueError("%s: want: a label or an integer array of shape [%d] is required" % (call, nq))
        a = np.asarray(want)
        if a.ndim == 0:
            a = np.full(nq, a[()])
        if a.dtype.kind not in "iu":
            raise TypeError("%s: want: an integer array, got %s" % (call, a.dtype))
        if a.ndim != 1 or a.shape[0] != nq:
            raise ValueError("%s: want: a scalar or an integer array of shape [%d], got %r" % (call, nq, a.shape))
        wide = a.astype(np.uint64) if a.dtype == np.uint64 else a.astype(np.int64)
        bad = np.flatnonzero(wide > LABEL_NONE) if a.dtype == np.uint64 else np.flatnonzero((wide < -1) | (wide > LABEL_NONE))
        if len(bad):
            raise ValueError("%s: want: query %d: %r is not a 32-bit label, -1 or LABEL_NONE" % (call, int(bad[0]), a[bad[0]]))
        return pack_labels(a, nq, "%s: want" % call)

    def info(self):
        """(n, listed, nlabels, longest): the vector count the handle was made for, the listed vectors, the distinct
        labels that list a row, the most rows listed under one label"""
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().phnsw_label_attr_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return int(a.value), int(b.value), int(c.value), int(d.value)

    listed = property(lambda self: self.info()[1])

    def count_device(self, nq, want, lo, hi, out_count, stream=0):
        """phnsw_label_attr_count_device: device pointers as integers, u32 [nq] each (lo and hi are KEYS); enqueued"""
        check(lib().phnsw_label_attr_count_device(self._h, C.c_void_p(want or None), C.c_void_p(lo or None), C.c_void_p(hi or None),
                                                  int(nq), C.c_void_p(out_count or None), C.c_void_p(stream or None)))

    def count(self, want, lo, hi):
        """the candidates of every (label, range) pair, u32 [nq]: filter_count's figure for the equivalent bitmaps.  want
        / lo / hi as the searches take them, at least one an array.  Host convenience over count_device (needs torch)"""
        import torch
        nq = max([len(np.atleast_1d(x)) for x in (want, lo, hi) if x is not None] or [1])
        w32 = self.wanted("LabeledAttribute.count", want, nq)
        l32, h32 = self.bounds("LabeledAttribute.count", lo, hi, nq)
        dev = torch.device("cuda", getattr(self.hnsw.store, "device", 0))
        wd = torch.from_numpy(w32.view(np.int32)).to(dev)
        ld = torch.from_numpy(l32.view(np.int32)).to(dev)
        hd = torch.from_numpy(h32.view(np.int32)).to(dev)
        out = torch.zeros(max(nq, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.count_device(nq, wd.data_ptr(), ld.data_ptr(), hd.data_ptr(), out.data_ptr())
        torch.cuda.synchronize(dev)
        return out.cpu().numpy().view(np.uint32)[:nq]

    def count_set_device(self, nq, nwant, want_first, want_values, lo, hi, out_count, stream=0):
        """phnsw_label_attr_count_set_device: device pointers as integers; want_first u32 [nq + 1], want_values u32
        [nwant], lo and hi u32 KEYS [nq], out_count u32 [nq]; enqueued"""
        check(lib().phnsw_label_attr_count_set_device(self._h, C.c_void_p(want_first or None), C.c_void_p(want_values or None),
                                                      C.c_void_p(lo or None), C.c_void_p(hi or None), int(nq), int(nwant),
                                                      C.c_void_p(out_count or None), C.c_void_p(stream or None)))

    def count_sets(self, want, lo, hi):
        """per query the candidates of (its set of wanted labels, its range), u32 [nq]: the summed span lengths of the
        DISTINCT labels of the set, filter_count's figure for the equivalent bitmaps.  want: as pack_label_sets takes it;
        lo / hi as the searches take them.  Host convenience over count_set_device (needs torch)"""
        import torch
        nq = len(want[0]) - 1 if isinstance(want, tuple) else len(want)
        first, values = pack_label_sets(want, nq)
        l32, h32 = self.bounds("LabeledAttribute.count_sets", lo, hi, nq)
        dev = torch.device("cuda", getattr(self.hnsw.store, "device", 0))
        fd = torch.from_numpy(first.view(np.int32)).to(dev)
        vd = torch.from_numpy(values.view(np.int32)).to(dev) if len(values) else None
        ld = torch.from_numpy(l32.view(np.int32)).to(dev)
        hd = torch.from_numpy(h32.view(np.int32)).to(dev)
        out = torch.zeros(max(nq, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.count_set_device(nq, len(values), fd.data_ptr(), 0 if vd is None else vd.data_ptr(), ld.data_ptr(), hd.data_ptr(),
                              out.data_ptr())
        torch.cuda.synchronize(dev)
        return out.cpu().numpy().view(np.uint32)[:nq]

    def close(self):
        if getattr(self, "_h", None):
            lib().phnsw_label_attr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Labels:
    """phnsw_labels: one label per vector of `hnsw`'s store, turned once into posting lists on the device (the ascending
    VectorIds of every label).  labels: an integer array [n] within u32; -1 or LABEL_NONE = the vector is not listed.  A
    vector is listed iff the index's bottom layer holds it.  The handle is a snapshot: after store.append, or with
    another index, search_exact_labeled refuses it as stale -- make a new one.  Keep `hnsw` alive while it is used.
    The handle also keeps the label column itself on the device (4 bytes per vector beside the lists): the graph walk by
    label, search_batch_labeled, the routed search_labeled and their forms by a set of labels (search_batch_labelset,
    search_labelset) read it."""

    def __init__(self, hnsw, labels):
        self._h = None
        if not isinstance(hnsw, Hnsw):
            raise TypeError("Labels: hnsw must be an Hnsw")
        lab = pack_labels(labels, int(hnsw.store.n), "labels")
        h = C.c_void_p()
        check(lib().phnsw_labels_create(hnsw._h, _p(lab), len(lab), C.byref(h)))
        self._h, self.hnsw = h, hnsw

    @classmethod
    def from_device(cls, hnsw, ptr, stream=0):
        """phnsw_labels_create_device: ptr = u32 labels [store n] in device memory (an integer), read on `stream`, which
        is synchronised"""
        if not isinstance(hnsw, Hnsw):
            raise TypeError("Labels.from_device: hnsw must be an Hnsw")
        self = cls.__new__(cls)
        self._h = None
        h = C.c_void_p()
        check(lib().phnsw_labels_create_device(hnsw._h, C.c_void_p(ptr or None), int(hnsw.store.n), C.c_void_p(stream or None),
                                               C.byref(h)))
        self._h, self.hnsw = h, hnsw
        return self

    def info(self):
        """(n, nlabels, listed, longest): the vector count the handle was made for, the distinct labels that list a
        vector, the listed vectors, the longest list"""
        v = [C.c_uint64() for _ in range(4)]
        check(lib().phnsw_labels_info(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    nlabels = property(lambda self: self.info()[1])
    listed = property(lambda self: self.info()[2])
    longest = property(lambda self: self.info()[3])

    def count_device(self, nq, want, out_count, stream=0):
        """phnsw_labels_count_device: device pointers as integers, u32 [nq] each"""
        check(lib().phnsw_labels_count_device(self._h, C.c_void_p(want or None), int(nq), C.c_void_p(out_count or None),
                                              C.c_void_p(stream or None)))

    def count(self, want):
        """the length of the list of every wanted label, u32 [nq] (0 for a label nobody carries and for LABEL_NONE):
        filter_count's figure for the equivalent bitmaps.  Host convenience over count_device (needs torch)"""
        import torch
        w = pack_labels(np.atleast_1d(want), len(np.atleast_1d(want)), "want")
        dev = torch.device("cuda", getattr(self.hnsw.store, "device", 0))
        wd = torch.from_numpy(w.view(np.int32)).to(dev)
        out = torch.zeros(max(len(w), 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.count_device(len(w), wd.data_ptr(), out.data_ptr())
        torch.cuda.synchronize(dev)
        return out.cpu().numpy().view(np.uint32)[:len(w)]

    def count_set_device(self, nq, nwant, want_first, want_values, out_count, stream=0):
        """phnsw_labels_count_set_device: device pointers as integers; want_first u32 [nq + 1], want_values u32 [nwant],
        out_count u32 [nq]"""
        check(lib().phnsw_labels_count_set_device(self._h, C.c_void_p(want_first or None), C.c_void_p(want_values or None),
                                                  int(nq), int(nwant), C.c_void_p(out_count or None),
                                                  C.c_void_p(stream or None)))

    def count_sets(self, want):
        """per set of wanted labels (pack_label_sets) the summed list lengths of its DISTINCT labels, u32 [nq]:
        filter_count's figure for the equivalent bitmaps.  Host convenience over count_set_device (needs torch)"""
        import torch
        nq = len(want[0]) - 1 if isinstance(want, tuple) else len(want)
        first, values = pack_label_sets(want, nq)
        dev = torch.device("cuda", getattr(self.hnsw.store, "device", 0))
        fd = torch.from_numpy(first.view(np.int32)).to(dev)
        vd = torch.from_numpy(values.view(np.int32)).to(dev) if len(values) else None
        out = torch.zeros(max(nq, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.count_set_device(nq, len(values), fd.data_ptr(), 0 if vd is None else vd.data_ptr(), out.data_ptr())
        torch.cuda.synchronize(dev)
        return out.cpu().numpy().view(np.uint32)[:nq]

    def close(self):
        if getattr(self, "_h", None):
            lib().phnsw_labels_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def SearchParameters(number_of_candidates=300, upper_layer_candidate_count=300, probe_depth=2):
    return SearchParams(number_of_candidates, upper_layer_candidate_count, probe_depth)


def BuildParameters(**kw):
    bp = BuildParams()
    lib().phnsw_default_build_params(C.byref(bp))
    for k, v in kw.items():
        if not hasattr(bp, k):
            raise TypeError("unknown build parameter %r" % k)
        setattr(bp, k, v)
    return bp


class Stored:
    """AbstractVector::Stored(VectorId)  types.rs:40-43"""

    def __init__(self, vector_id):
        self.id = int(vector_id)


class Unstored:
    """AbstractVector::Unstored(&T)"""

    def __init__(self, vec):
        self.vec = np.ascontiguousarray(vec, dtype=np.float32)


class VectorStore:
    """flat HBM vector store + metric: the Comparator of the GPU path"""

    def __init__(self, rows=None, metric=METRIC_COSINE_HALF, device=0, _handle=None):
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            rows = np.ascontiguousarray(rows, dtype=np.float32)
            assert rows.ndim == 2
            check(lib().phnsw_store_create(_p(rows), rows.shape[0], rows.shape[1], metric, device, C.byref(self._h)))
        self.device = device
        self._refresh()

    def _refresh(self):
        n, dim, ld, m = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_int()
        ptr = C.c_void_p()
        check(lib().phnsw_store_info(self._h, C.byref(n), C.byref(dim), C.byref(ld), C.byref(m), C.byref(ptr)))
        self.n, self.dim, self.ld, self.metric, self.rows_dev = n.value, dim.value, ld.value, m.value, ptr.value

    def append(self, rows):
        """more vectors behind the same comparator; returns the first new VectorId"""
        rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float32)
        assert rows.shape[1] == self.dim
        first = C.c_uint64()
        check(lib().phnsw_store_append(self._h, _p(rows), rows.shape[0], C.byref(first)))
        self._refresh()
        return first.value

    @classmethod
    def synthetic(cls, n, dim, seed=42, first=0, normalize=True, metric=METRIC_COSINE_HALF, device=0):
        """make_random_hnsw's data (bigvec.rs:23-29, 59-65) generated on the GPU"""
        h = C.c_void_p()
        check(lib().phnsw_store_create_synthetic(first, n, dim, seed, int(normalize), metric, device, C.byref(h)))
        return cls(_handle=h, device=device)

    @classmethod
    def clustered(cls, n, dim, seed=42, first=0, n_clusters=1000, noise=1.0, metric=METRIC_COSINE_HALF, device=0):
        """clustered synthetic rows (benchmark dataset)"""
        h = C.c_void_p()
        check(lib().phnsw_store_create_clustered(first, n, dim, seed, n_clusters, noise, metric, device, C.byref(h)))
        return cls(_handle=h, device=device)

    @classmethod
    def from_device(cls, data_ptr, n, dim, ld, metric=METRIC_COSINE_HALF, device=0, keepalive=None):
        h = C.c_void_p()
        check(lib().phnsw_store_create_device(C.c_void_p(data_ptr), n, dim, ld, metric, device, C.byref(h)))
        s = cls(_handle=h, device=device)
        s._keepalive = keepalive
        return s

    def read(self, first=0, count=None, out=None):
        count = self.n - first if count is None else count
        if out is None:
            out = np.empty((count, self.dim), dtype=np.float32)
        assert out.shape == (count, self.dim) and out.dtype == np.float32 and out.flags.c_contiguous
        check(lib().phnsw_store_read(self._h, first, count, _p(out)))
        return out

    def bruteforce_topk(self, queries, k=10):
        """exact k nearest by (distance, id): MFMA GEMM + top-k (ground truth for recall@k)"""
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        assert q.shape[1] == self.dim
        ids = np.empty((q.shape[0], k), dtype=np.uint64)
        d = np.empty((q.shape[0], k), dtype=np.float32)
        check(lib().phnsw_bruteforce_topk(self._h, _p(q), q.shape[0], k, _p(ids), _p(d)))
        return ids, d

    def bruteforce_topk_device(self, queries_ptr, ldq, nq, k, out_ids_ptr, out_d_ptr, stream=0):
        check(lib().phnsw_bruteforce_topk_device(self._h, C.c_void_p(queries_ptr), ldq, nq, k, C.c_void_p(out_ids_ptr),
                                                 C.c_void_p(out_d_ptr), C.c_void_p(stream or None)))
        return lib().phnsw_bruteforce_last_gemm_ms()

    def compare_vec(self, v, ids):
        """Comparator::compare_vec batched (lib.rs:69-73): distances from v to Stored(ids)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        out = np.empty(len(ids), dtype=np.float32)
        if isinstance(v, Stored):
            check(lib().phnsw_distance_batch(self._h, None, v.id, _p(ids), len(ids), _p(out)))
        else:
            q = v.vec if isinstance(v, Unstored) else np.ascontiguousarray(v, dtype=np.float32)
            assert q.shape[-1] == self.dim
            check(lib().phnsw_distance_batch(self._h, _p(q), 0, _p(ids), len(ids), _p(out)))
        return out

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().phnsw_store_destroy(h)
            except Exception:  # interpreter shutdown
                pass


class PqStore(VectorStore):
    """product-quantised view of a VectorStore (pq.rs): u8 codes over per-sub-space codebooks"""

    TABLE_MODES = {"f32": 0, "f16": 1, "u8": 2}

    def __init__(self, full, m, ksub=256, seed=0, table_f16=False, table_mode=None, kmeans_iters=0, kmeans_sample=0,
                 comm=None):
        """table_mode: "f32" (reference arithmetic), "f16" or "u8" (phnsw_pq_set_table_mode); kmeans_iters: Lloyd
        iterations on the codebooks (0 = the reference's random_centroids, pq.rs:261-285); comm: a communicator of
        parallel_hnsw_amd.sharded -- the encode of pq.rs:326-333 split over its ranks, codes all-gathered"""
        h = C.c_void_p()
        cc = C.byref(comm.c_comm(full.device)) if comm is not None else None
        check(lib().phnsw_store_create_pq_sharded(full._h, m, ksub, seed, kmeans_iters, kmeans_sample, cc, C.byref(h)))
        VectorStore.__init__(self, _handle=h, device=full.device)
        mode = self.TABLE_MODES[table_mode] if table_mode is not None else int(table_f16)
        if mode:
            check(lib().phnsw_pq_set_table_mode(self._h, mode))
        self.table_mode = mode
        self.table_f16 = mode == 1

        self.full = full
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().phnsw_pq_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.m, self.ksub, self.dsub = a.value, b.value, c.value

    def set_table_mode(self, table_mode):
        """switch the lookup-table storage; "u8" is search-only (see phnsw_pq_set_table_mode)"""
        mode = self.TABLE_MODES[table_mode] if isinstance(table_mode, str) else int(table_mode)
        check(lib().phnsw_pq_set_table_mode(self._h, mode))
        self.table_mode, self.table_f16 = mode, mode == 1

    def quantize(self, rows):
        """Quantizer::quantize  pq.rs:61-71 -> codes [n, m]"""
        rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float32)
        assert rows.shape[1] == self.dim
        out = np.empty((rows.shape[0], self.m), dtype=np.uint8)
        check(lib().phnsw_pq_quantize(self._h, _p(rows), rows.shape[0], _p(out)))
        return out

    def reconstruct(self, codes):
        """Quantizer::reconstruct  pq.rs:73-81 -> rows [n, dim]"""
        codes = np.ascontiguousarray(np.atleast_2d(codes), dtype=np.uint8)
        assert codes.shape[1] == self.m
        out = np.empty((codes.shape[0], self.dim), dtype=np.float32)
        check(lib().phnsw_pq_reconstruct(self._h, _p(codes), codes.shape[0], _p(out)))
        return out

    def codes(self):
        out = np.empty((self.n, self.m), dtype=np.uint8)
        check(lib().phnsw_pq_read(self._h, _p(out), None))
        return out

    def codebook(self):
        out = np.empty((self.m, self.ksub, self.dsub), dtype=np.float32)
        check(lib().phnsw_pq_read(self._h, None, _p(out)))
        return out


class F16Store(VectorStore):
    """half-precision view of an f32 VectorStore (phnsw_store_create_f16): the rows rounded to IEEE binary16, half the
    bytes per vector.  Distances widen the halves and run the f32 arithmetic, so read() returns exactly the rows the
    searches see.  Search-only: adopt a graph built over the f32 store with Hnsw.from_layers(f16_store, ...)"""

    def __init__(self, full):
        h = C.c_void_p()
        check(lib().phnsw_store_create_f16(full._h, C.byref(h)))
        VectorStore.__init__(self, _handle=h, device=full.device)
        self.full = full

    @classmethod
    def from_full(cls, store):
        return cls(store)


class _Int8Rows(VectorStore):
    """what I8Store and I8QStore share: the rows of an f32 store as int8 codes with one f32 scale per row"""

    _create = None  # the constructor of the kind

    def __init__(self, full):
        h = C.c_void_p()
        check(getattr(lib(), self._create)(full._h, C.byref(h)))
        VectorStore.__init__(self, _handle=h, device=full.device)
        self.full = full

    @classmethod
    def from_full(cls, store):
        return cls(store)

    def _read_i8(self):
        codes = np.empty((self.n, self.dim), dtype=np.int8)
        scales = np.empty(self.n, dtype=np.float32)
        check(lib().phnsw_i8_read(self._h, _p(codes), _p(scales)))
        return codes, scales

    def codes(self):
        """the stored codes [n, dim] int8"""
        return self._read_i8()[0]

    def scales(self):
        """the rows' scales [n] f32"""
        return self._read_i8()[1]


class I8Store(_Int8Rows):
    """int8 view of an f32 VectorStore (phnsw_store_create_i8): every row scalar-quantised with its own scale
    (maxabs / 127), a quarter of the bytes per vector.  Distances dequantise (scale * code) and run the f32
    arithmetic, so read() returns exactly the rows the searches see.  Search-only, like F16Store"""

    _create = "phnsw_store_create_i8"


class I8QStore(_Int8Rows):
    """the rows of an I8Store, byte for byte (phnsw_store_create_i8q: same codes(), scales() and read()), searched
    symmetrically: a distance quantises the query the way the rows were quantised and is
    (scale_q * scale_r) * (integer dot product of the codes), put through the metric -- tests/i8q_reference.py restates
    it.  Dot-product metrics only (an L2 store is refused).  Search-only, like I8Store"""

    _create = "phnsw_store_create_i8q"


class BitStore(VectorStore):
    """one sign bit per component of an f32 VectorStore (phnsw_store_create_bits): bit j of a row is row[j] < 0, 96
    bytes per 768-component vector.  A distance comes from the Hamming distance h of row and query (the query reduced
    by the same rule): dim - 2 h for the dot-product metrics, 4 h for L2, then the metric's last step -- exactly the f32
    search over read()'s +1 / -1 rows with the query where(q < 0, -1, +1); tests/bits_reference.py restates it.  The
    plain searches return these sign-vector distances; Hnsw.search_batch_reranked returns true f32 distances.  All
    three metrics.  Plain searches, distance batches and the re-ranked search only: every filtered, exact, radius or
    build call refuses it.  Adopt a graph built over the f32 store with Hnsw.from_layers(bit_store, ...)"""

    def __init__(self, full):
        h = C.c_void_p()
        check(lib().phnsw_store_create_bits(full._h, C.byref(h)))
        VectorStore.__init__(self, _handle=h, device=full.device)
        self.full = full

    @classmethod
    def from_full(cls, store):
        return cls(store)

    def words(self):
        """the sign bits [n, ceil(dim / 32)] uint32: component j is bit j & 31 of word j >> 5"""
        out = np.empty((self.n, (self.dim + 31) // 32), dtype=np.uint32)
        check(lib().phnsw_bits_read(self._h, _p(out)))
        return out


def _reranked_kind(store):
    """the name a converted store's re-ranked search calls carry"""
    if isinstance(store, BitStore):
        return "bits"
    return "i8q" if isinstance(store, I8QStore) else ("i8" if isinstance(store, I8Store) else "f16")


class SharedPqStore(VectorStore):
    """the reference's quantizer shape (pq.rs:19-27, 61-81, 261-285): ONE codebook of up to 65535 centroid
    sub-vectors shared by all sub-spaces, u16 codes, quantize = top-1 of an HNSW search over the centroids"""

    def __init__(self, full, centroid_size, number_of_centroids, seed=0, centroid_bp=None, quantized_search=None,
                 centroid_metric=METRIC_L2, comm=None):
        h = C.c_void_p()
        cbp = centroid_bp or BuildParameters()
        qs = quantized_search or SearchParameters()
        cc = C.byref(comm.c_comm(full.device)) if comm is not None else None
        check(lib().phnsw_store_create_pq_shared_sharded(full._h, centroid_size, number_of_centroids, seed, C.byref(cbp),
                                                         C.byref(qs), centroid_metric, cc, C.byref(h)))
        VectorStore.__init__(self, _handle=h, device=full.device)
        self.full = full
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().phnsw_pq_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.m, self.ksub, self.dsub = a.value, b.value, c.value

    def codes(self):
        out = np.empty((self.n, self.m), dtype=np.uint16)
        check(lib().phnsw_pq_shared_read(self._h, _p(out), None))
        return out

    def codebook(self):
        out = np.empty((self.ksub, self.dsub), dtype=np.float32)
        check(lib().phnsw_pq_shared_read(self._h, None, _p(out)))
        return out

    def reconstruct_store(self):
        """the reconstructions as an f32 VectorStore (same distance bits as the code rows)"""
        h = C.c_void_p()
        check(lib().phnsw_pq_shared_reconstruct_store(self._h, C.byref(h)))
        return VectorStore(_handle=h, device=self.device)


class QuantizedHnsw:
    """QuantizedHnsw (pq.rs:120-131, 287-364): quantizer + Hnsw over the codes + full comparator"""

    @classmethod
    def reference_shaped(cls, number_of_centroids, comparator, centroid_size, bp=None, centroid_bp=None,
                         quantized_search=None, seed=0, centroid_metric=METRIC_L2, improve_neighbors=False):
        """QuantizedHnsw::new(number_of_centroids, comparator, PqBuildParameters{centroids, hnsw, quantized_search})
        pq.rs:287-344 in its own shape: shared codebook, HNSW quantizer, u16 codes, Hnsw over the quantised
        vectors (built on their materialised reconstructions -- identical distance bits -- and adopted over
        the codes)"""
        self = cls.__new__(cls)
        self.full = comparator
        self.store = SharedPqStore(comparator, centroid_size, number_of_centroids, seed, centroid_bp, quantized_search,
                                   centroid_metric)
        rec = self.store.reconstruct_store()
        g = Hnsw.generate(rec, np.arange(comparator.n, dtype=np.uint64), bp or BuildParameters(promote=0))
        # QuantizedHnsw::improve_neighbors (pq.rs:372-380, what test_pq_recall asserts on): run on the graph over
        # the reconstructions before it is adopted over the codes (same distance bits; the code rows themselves
        # are searched, not built on)
        self.improve_neighbors_recall = (g.improve_neighbors_upto(g.layer_count(), g.build_parameters, None)
                                         if improve_neighbors else None)
        self.hnsw = Hnsw.from_layers(self.store, [(l.nodes, l.neighbors) for l in g.layers], g.build_parameters)
        del g, rec
        return self

    def __init__(self, number_of_centroids, comparator, bp=None, m=None, seed=0, vids=None, table_f16=False,
                 table_mode=None, kmeans_iters=0, kmeans_sample=0, graph=None):
        """QuantizedHnsw::new(number_of_centroids, comparator, bp): per-sub-space codebooks of
        `number_of_centroids` (<= 256) centroids, encode, Hnsw::generate over the codes.

        Without an explicit `bp` the graph over the codes is built with promote=0: a
        reconstruction is not unit length, so a stored code's distance to itself is not within
        the 1e-5 of match_within_epsilon (search.rs:173-187), every vector counts as
        "unreachable" and promote_at_layer's sequential thinning (lib.rs:1243-1262, quadratic in
        the candidates) never finishes at scale -- in the reference as much as here."""
        m = m or max(4, comparator.dim // 8)
        self.full = comparator
        self.store = PqStore(comparator, m, number_of_centroids, seed, table_f16, table_mode, kmeans_iters, kmeans_sample)
        vids = np.arange(comparator.n, dtype=np.uint64) if vids is None else vids
        if graph is not None:
            # `graph`: an Hnsw built over the full-precision comparator; its layers are adopted over the code rows
            # (phnsw_index_from_layers), so the traversal follows the full-precision graph with quantised distances
            self.hnsw = Hnsw.from_layers(self.store, [(l.nodes, l.neighbors) for l in graph.layers], graph.build_parameters)
        else:
            self.hnsw = Hnsw.generate(self.store, vids, bp or BuildParameters(promote=0))

    def search_batch(self, queries, sp=None, quantize_query=False, stats=False):
        sp = sp or SearchParameters()
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        assert q.shape[1] == self.full.dim
        nq, ef = q.shape[0], sp.number_of_candidates
        ids = np.empty((nq, ef), dtype=np.uint64)
        d = np.empty((nq, ef), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        st = np.zeros((nq, 2), dtype=np.uint64) if stats else None
        check(lib().phnsw_pq_search_batch(self.hnsw._h, self.full._h, _p(q), nq, C.byref(sp), int(quantize_query),
                                          _p(ids), _p(d), _p(ln), _p(st)))
        return (ids, d, ln, st) if stats else (ids, d, ln)

    def search_batch_device(self, nq, sp, queries, ldq, out_ids, out_d, out_len, status, out_stats=0, stream=0):
        check(lib().phnsw_pq_search_batch_device(self.hnsw._h, self.full._h, C.c_void_p(queries), ldq, nq, C.byref(sp),
                                                 C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len),
                                                 C.c_void_p(out_stats or None), C.c_void_p(status),
                                                 C.c_void_p(stream or None)))

    def search(self, v, sp=None):
        """QuantizedHnsw::search(v, sp)  pq.rs:346-364"""
        ids, d, ln = self.search_batch(v.vec if isinstance(v, Unstored) else v, sp)
        return [(int(ids[0, i]), d[0, i]) for i in range(int(ln[0]))]

    def vector_count(self):
        return self.hnsw.vector_count()

    # QuantizedHnsw forwards these to the Hnsw over the codes  pq.rs:366-411
    def improve_index(self, bp=None, last_recall=None, progress=None):
        return self.hnsw.improve_index(bp or self.build_parameters_for_improve_index(), last_recall, progress)

    def improve_neighbors_upto(self, upto, bp=None, last_recall=None):
        return self.hnsw.improve_neighbors_upto(upto, bp or self.build_parameters_for_improve_index(), last_recall)

    def promote_at_layer(self, layer_from_top, bp=None):
        return self.hnsw.promote_at_layer(layer_from_top, bp or self.hnsw.build_parameters)

    def threshold_nn(self, threshold, probe_depth, initial_search_depth, max_out=64):
        return self.hnsw.threshold_nn(threshold, probe_depth, initial_search_depth, max_out)

    def stochastic_recall(self, op=None):
        return self.hnsw.stochastic_recall(op)

    def build_parameters_for_improve_index(self):
        return self.hnsw.build_parameters


class Layer:
    """Layer { neighborhood_size, nodes, neighbors }  lib.rs:85-91 (host copies, u64)"""

    def __init__(self, nodes, neighbors, neighborhood_size):
        self.nodes = nodes
        self.neighbors = neighbors
        self.neighborhood_size = neighborhood_size

    def node_count(self):
        return len(self.nodes)

    def get_neighbors(self, n):
        row = self.neighbors[n]
        return row[row != EMPTY]  # trailing sentinels trimmed (lib.rs:114-125)


class Hnsw:
    def __init__(self, store, handle, build_parameters=None):
        self.store = store
        self._h = handle
        self.build_parameters = build_parameters or BuildParameters()

    # -- construction -------------------------------------------------------
    @classmethod
    def generate(cls, c, vs, bp=None, progress=None):
        """Hnsw::generate(c, vs, bp, progress)  lib.rs:825-893"""
        bp = bp or BuildParameters()
        vs = np.ascontiguousarray(vs, dtype=np.uint64)
        h = C.c_void_p()
        cb = _lib.PROGRESS_CB(progress) if progress else None
        check(lib().phnsw_build(c._h, _p(vs), len(vs), C.byref(bp), cb, None, C.byref(h)))
        return cls(c, h, bp)

    @classmethod
    def from_layers(cls, c, layers, bp=None):
        """adopt [(nodes, neighbors[n, W])...] top first, e.g. deserialised from the Rust crate"""
        L = len(layers)
        nodes = [np.ascontiguousarray(l[0], dtype=np.uint64) for l in layers]
        nbs = [np.ascontiguousarray(l[1], dtype=np.uint64).reshape(len(nodes[i]), -1) for i, l in enumerate(layers)]
        counts = np.array([len(x) for x in nodes], dtype=np.uint64)
        widths = np.array([nb.shape[1] for nb in nbs], dtype=np.uint64)
        pn = (C.c_void_p * L)(*[x.ctypes.data for x in nodes])
        pb = (C.c_void_p * L)(*[x.ctypes.data for x in nbs])
        h = C.c_void_p()
        check(lib().phnsw_index_from_layers(c._h, L, _p(counts), _p(widths), pn, pb, C.byref(h)))
        return cls(c, h, bp)

    def generate_layer(self, vs, neighborhood_size, bp=None):
        vs = np.ascontiguousarray(vs, dtype=np.uint64)
        check(lib().phnsw_generate_layer(self._h, _p(vs), len(vs), neighborhood_size,
                                         C.byref(bp or self.build_parameters)))

    def link_layer_to_better_neighbors(self, layer_from_top, sp):
        """lib.rs:1070-1082; returns the number of new edges"""
        added = C.c_uint64()
        check(lib().phnsw_link_layer(self._h, layer_from_top, C.byref(sp), self.build_parameters.neighborhood_size,
                                     C.byref(added)))
        return added.value

    def improve_index(self, bp=None, last_recall=None, progress=None):
        """Hnsw::improve_index(bp, last_recall: Option<f32>, progress)  lib.rs:1664-1686"""
        out = C.c_float()
        cb = _lib.PROGRESS_CB(progress) if progress else None
        check(lib().phnsw_improve_index(self._h, C.byref(bp or self.build_parameters),
                                        float("nan") if last_recall is None else last_recall, cb, None, C.byref(out)))
        return out.value

    def improve_neighbors_upto(self, upto, bp=None, last_recall=None):
        out = C.c_float()
        check(lib().phnsw_improve_neighbors_upto(self._h, upto, C.byref(bp or self.build_parameters),
                                                 float("nan") if last_recall is None else last_recall,
                                                 C.byref(out)))
        return out.value

    def extend_layer(self, layer_from_top, vecs):
        """Hnsw::extend_layer  lib.rs:1039-1068"""
        v = np.ascontiguousarray(vecs, dtype=np.uint64)
        check(lib().phnsw_extend_layer(self._h, layer_from_top, _p(v), len(v)))

    def promote_at_layer(self, layer_from_top, bp=None):
        """lib.rs:1273-1427"""
        out = C.c_int()
        check(lib().phnsw_promote_at_layer(self._h, layer_from_top, C.byref(bp or self.build_parameters), C.byref(out)))
        return bool(out.value)

    def discover_unreachable_vectors(self, layer_from_top, sp):
        """lib.rs:1002-1037"""
        n = self._layer(layer_from_top).node_count()
        out = np.empty(n, dtype=np.uint64)
        cnt = C.c_uint64()
        check(lib().phnsw_discover_unreachable(self._h, layer_from_top, C.byref(sp), _p(out), C.byref(cnt)))
        return out[:cnt.value].copy()

    def stochastic_recall_at(self, at, op=None):
        out = C.c_float()
        op = op or self.build_parameters.optimization
        check(lib().phnsw_stochastic_recall_at(self._h, at, C.byref(op), C.byref(out)))
        return out.value

    def stochastic_recall(self, op=None):
        return self.stochastic_recall_at(self.layer_count() - 1, op)

    # -- accessors ----------------------------------------------------------
    def layer_count(self):
        return lib().phnsw_index_layer_count(self._h)

    def _layer(self, lft):
        n, w = C.c_uint64(), C.c_uint64()
        check(lib().phnsw_index_layer_info(self._h, lft, C.byref(n), C.byref(w)))
        nodes = np.empty(n.value, dtype=np.uint64)
        nb = np.empty((n.value, w.value), dtype=np.uint64)
        check(lib().phnsw_index_layer_read(self._h, lft, _p(nodes), _p(nb)))
        return Layer(nodes, nb, w.value)

    @property
    def layers(self):
        """Vec<Layer>, top first (lib.rs:587)"""
        return [self._layer(i) for i in range(self.layer_count())]

    def get_layer(self, i):
        """counts from the bottom (lib.rs:604-606)"""
        return self._layer(self.layer_count() - i - 1)

    def get_layer_from_top(self, i):
        """lib.rs:617-624 (None past the stack)"""
        return self._layer(i) if 0 <= i < self.layer_count() else None

    def get_layer_above(self, i):
        """lib.rs:631-637: the layer above layer-from-top i"""
        return None if i == 0 else self.get_layer_from_top(i - 1)

    def neighborhood_size(self):
        return int(self.build_parameters.neighborhood_size)  # lib.rs:596-598

    def zero_neighborhood_size(self):
        return int(self.build_parameters.zero_layer_neighborhood_size)  # lib.rs:600-602

    def comparator(self):
        return self.store  # lib.rs:648-650

    def __len__(self):
        return self.vector_count()  # lib.rs:895-897

    def is_empty(self):
        return self.vector_count() == 0  # lib.rs:899-901

    def all_vectors(self):
        """lib.rs:968-975: the bottom layer's VectorIds"""
        return self._layer(self.layer_count() - 1).nodes

    def supers_for_layer(self, layer_id):
        """lib.rs:977-984: the VectorIds of the layer above `layer_id` (counted from the bottom); the top
        layer's only super is its entry node"""
        if self.layer_count() == layer_id + 1:
            return self.get_layer(layer_id).nodes[0:1]
        return self.get_layer(layer_id + 1).nodes

    def entry_vector(self):
        return int(self._layer(0).nodes[0])

    def vector_count(self):
        n = C.c_uint64()
        check(lib().phnsw_index_layer_info(self._h, self.layer_count() - 1, C.byref(n), None))
        return n.value

    # -- search -------------------------------------------------------------
    def search_batch(self, queries=None, qids=None, sp=None, exclude=None, upto=0, stats=False, k=None):
        """Hnsw::search for many queries; returns (ids[nq, ef] u64, d[nq, ef] f32, len[nq]); with k only the best k
        results of each query are transferred (phnsw_search_batch_topk): ids[nq, k], d[nq, k]"""
        sp = sp or SearchParameters()
        ef = sp.number_of_candidates
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            assert q.shape[1] == self.store.dim
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        w = ef if k is None else int(k)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        st = np.zeros((nq, 2), dtype=np.uint64) if stats else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        if k is not None:
            assert not stats
            check(lib().phnsw_search_batch_topk(self._h, _p(q), _p(qi), nq, C.byref(sp), upto, _p(ex), w, _p(ids), _p(d),
                                                _p(ln)))
        elif queries is not None:
            check(lib().phnsw_search_batch(self._h, _p(q), nq, C.byref(sp), upto, _p(ex), _p(ids), _p(d), _p(ln), _p(st)))
        else:
            check(lib().phnsw_search_batch_stored(self._h, _p(qi), nq, C.byref(sp), upto, _p(ex), _p(ids), _p(d),
                                                  _p(ln), _p(st)))
        return (ids, d, ln, st) if stats else (ids, d, ln)

    def search_batch_filtered(self, queries=None, qids=None, sp=None, allow=None, strict=False, exclude=None, upto=0,
                              stats=False, k=None):
        """search_batch restricted to allowed VectorIds (phnsw_search_batch_filtered): closest_vectors' `include`
        (lib.rs:250-277) as a bitmap.  allow: a bool array [n] (one filter for all queries) or [nq, n] (one per query), or
        the packed u32 words themselves ([ceil(n/32)] or [nq, stride]); None = the default of set_filter, else no
        filter.  A post-filter on each layer's queue: about density * number_of_candidates results come back, so
        selective filters want a larger number_of_candidates (or search_exact_filtered, which scans the allowed rows
        instead; filter_count tells how many there are).  The entry vector may be returned although it is
        disallowed (as the reference returns it although excluded); strict=True removes it.
        Returns (ids[nq, k or ef] u64, d f32, len[nq]) and the stats with stats=True"""
        sp = sp or SearchParameters()
        ef = sp.number_of_candidates
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            assert q.shape[1] == self.store.dim
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        words, stride = pack_allow(allow, self.store.n, nq)
        w = ef if k is None else int(k)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        st = np.zeros((nq, 2), dtype=np.uint64) if stats else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_batch_filtered(self._h, _p(q), _p(qi), nq, C.byref(sp), upto, _p(ex), _p(words), stride,
                                                FILTER_STRICT if strict else 0, 0 if k is None else w, _p(ids), _p(d),
                                                _p(ln), _p(st)))
        return (ids, d, ln, st) if stats else (ids, d, ln)

    def search_batch_filtered_device(self, nq, sp, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                                     allow=0, allow_stride=0, strict=False, out_stats=0, upto=0, stream=0):
        """zero-copy form (phnsw_search_batch_filtered_device): search_batch_device with `allow`, a device pointer to
        the packed words -- one bitmap (allow_stride 0) or nq bitmaps allow_stride words apart; 0 = the default of
        set_filter"""
        check(lib().phnsw_search_batch_filtered_device(
            self._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp), upto,
            C.c_void_p(exclude or None), C.c_void_p(allow or None), int(allow_stride), FILTER_STRICT if strict else 0,
            C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(out_stats or None), C.c_void_p(status),
            C.c_void_p(stream or None)))

    def set_filter(self, allow_dev=0):
        """tombstones (phnsw_index_set_filter_device): a device pointer to one packed bitmap of ceil(n/32) words, kept
        alive by the caller, becomes the filter of every filtered call that passes none; 0 clears it.  search_batch and
        the other unfiltered calls never see it.  Not while searches on the index are in flight"""
        check(lib().phnsw_index_set_filter_device(self._h, C.c_void_p(allow_dev or None)))

    def search_exact_filtered(self, queries=None, qids=None, allow=None, exclude=None, k=10):
        """the exact top-k of the allowed vectors (phnsw_search_exact_filtered): a scan of the allow-list instead of the
        graph search -- the call for selective filters, where search_batch_filtered returns about density *
        number_of_candidates results.  Candidates: ids below n whose bit is set (allow as for search_batch_filtered;
        None = the default of set_filter, else every vector), that are not exclude[q] and that the index holds.  A
        disallowed id is never returned.  1 <= k <= 1024.  filter_count(allow) tells how many candidates there are.
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq]): ascending (distance, id), the distance bits of compare_vec,
        padded with EMPTY / f32::MAX"""
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            assert q.shape[1] == self.store.dim
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        words, stride = pack_allow(allow, self.store.n, nq)
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_exact_filtered(self._h, _p(q), _p(qi), nq, _p(ex), _p(words), stride, int(k), _p(ids), _p(d),
                                                _p(ln)))
        return ids, d, ln

    def search_exact_filtered_device(self, nq, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                                     allow=0, allow_stride=0, stream=0):
        """zero-copy form (phnsw_search_exact_filtered_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF, enqueued on `stream`; allow = one packed bitmap (allow_stride 0) or nq bitmaps allow_stride words
        apart, 0 = the default of set_filter"""
        check(lib().phnsw_search_exact_filtered_device(
            self._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.c_void_p(exclude or None),
            C.c_void_p(allow or None), int(allow_stride), int(k), C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len),
            C.c_void_p(status), C.c_void_p(stream or None)))

    def exact_shared_supported(self, k=10):
        """phnsw_exact_shared_supported: 0, or the code search_exact_shared would refuse this index and k with (a PQ
        store, rows longer than 1536 floats, k outside 1..1024); runs nothing"""
        return int(lib().phnsw_exact_shared_supported(self._h, int(k)))

    def search_exact_shared(self, queries=None, qids=None, allow=None, exclude=None, k=10):
        """search_exact_filtered for ONE allow-list shared by all queries, computed as a queries x candidates distance
        table on the table kernels of the dense top layers (phnsw_search_exact_shared) instead of a per-query scan: the
        same rows, bit for bit.  allow: one bool mask [n] or its packed u32 words, None = the default of set_filter,
        else every vector of the index; a 2-D allow (one bitmap per query) raises ValueError -- that is
        search_exact_filtered's.  Exactly one of queries / qids.  f32, f16, i8 and i8q stores with rows up to 1536 floats.
        Measured on 1M x 768 f32 rows, 10 000 queries, k = 10: 6 to 18 times faster than the scan from 1 000 candidates
        up, and faster than the approximate graph walk below roughly 20 000 to 99 000 candidates
        (profiles/filter_dense/README.md).
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq])"""
        if (queries is None) == (qids is None):
            raise ValueError("search_exact_shared: pass queries or qids (exactly one)")
        if allow is not None and np.ndim(allow) != 1:
            raise ValueError("search_exact_shared: allow is ONE bitmap for all queries, a mask [n] or its packed words; "
                             "per-query bitmaps are search_exact_filtered's")
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            assert q.shape[1] == self.store.dim
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        words, _ = pack_allow(allow, self.store.n, nq)
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_exact_shared(self._h, _p(q), _p(qi), nq, _p(ex), _p(words), int(k), _p(ids), _p(d), _p(ln)))
        return ids, d, ln

    def search_exact_shared_device(self, nq, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                                   allow=0, stream=0):
        """zero-copy form (phnsw_search_exact_shared_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF; allow = one packed bitmap, 0 = the default of set_filter.  status 4 = a stored query id at or past n
        (an empty row).  Synchronises `stream` once, to read the candidate count back"""
        check(lib().phnsw_search_exact_shared_device(
            self._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.c_void_p(exclude or None),
            C.c_void_p(allow or None), int(k), C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len),
            C.c_void_p(status), C.c_void_p(stream or None)))

    def _exact_radius_call(self, who, queries, qids, radius, allow, exclude):
        """the arguments of phnsw_search_exact_radius, checked and packed -> call(room) -> (first, total, ids, d)"""
        if (queries is None) == (qids is None):
            raise ValueError("%s: pass queries or qids (exactly one)" % who)
        if radius is None:
            raise ValueError("%s: pass radius (a scalar or one per query)" % who)
        if allow is not None and np.ndim(allow) != 1:
            raise ValueError("%s: allow is ONE bitmap for all queries, a mask [n] or its packed words" % who)
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            assert q.shape[1] == self.store.dim
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))
        words, _ = pack_allow(allow, self.store.n, nq)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)

        def call(room):
            first = np.zeros(nq + 1, dtype=np.uint64)
            total = C.c_uint64(0)
            ids = np.empty(room, dtype=np.uint64) if room else None
            d = np.empty(room, dtype=np.float32) if room else None
            check(lib().phnsw_search_exact_radius(self._h, _p(q), _p(qi), nq, _p(ex), _p(words), _p(r), int(room), _p(first),
                                                  _p(ids), _p(d), C.byref(total)))
            return first, int(total.value), ids, d
        return nq, call

    def search_exact_radius(self, queries=None, qids=None, radius=None, allow=None, exclude=None, cap=None):
        """every candidate closer to a query than its radius (phnsw_search_exact_radius): d(q, v) < radius[q] as an f32
        comparison, strict; a NaN, zero or negative radius matches nothing and a row at +inf is never returned.  radius:
        one per query or a scalar for all.  Candidates, allow, exclude and stores as for search_exact_shared, whose
        distance tables this call computes; exactly one of queries / qids.  The library negotiates sizes as snprintf
        does: this method calls once with room for `cap` entries (default 64 per query) and, when told that more are
        inside the radii, once more with exactly that room.
        Returns (first[nq + 1] u64, ids[total] u64, d[total] f32): the rows of query i are ids / d[first[i]:first[i + 1]],
        ascending by (distance, id).  Measured on 1M x 768 f32 rows, 10 000 queries: 2 to 25 ms more than
        search_exact_shared at k = 10 (177 ms) for 10 to 1000 rows inside the radius per query (profiles/radius/README.md)."""
        nq, call = self._exact_radius_call("search_exact_radius", queries, qids, radius, allow, exclude)
        room = max(64 * nq, 1) if cap is None else int(cap)
        first, total, ids, d = call(room)
        if total > room:
            first, total, ids, d = call(total)
        if ids is None:
            ids, d = np.empty(0, dtype=np.uint64), np.empty(0, dtype=np.float32)
        return first, ids[:total], d[:total]

    def count_exact_radius(self, queries=None, qids=None, radius=None, allow=None, exclude=None):
        """the count-only form of search_exact_radius (cap 0, no arrays): first[nq + 1] u64; no record is kept or sorted"""
        _, call = self._exact_radius_call("count_exact_radius", queries, qids, radius, allow, exclude)
        return call(0)[0]

    def search_exact_radius_device(self, nq, radius, cap, out_first, out_ids, out_d, status, out_total, queries=0, ldq=0,
                                   qids=0, exclude=0, allow=0, stream=0):
        """zero-copy form (phnsw_search_exact_radius_device): device pointers as integers; radius f32 [nq], u64 first
        [nq + 1], u32 ids [cap], f32 d [cap], u32 status [nq] (4 = a stored query id at or past n: an empty segment),
        one u64 total.  ids / d are written only if the total is at most cap; cap 0 with out_ids = out_d = 0 counts
        only.  Synchronises `stream` twice (the candidate count, the total), once with cap 0"""
        check(lib().phnsw_search_exact_radius_device(
            self._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.c_void_p(exclude or None),
            C.c_void_p(allow or None), C.c_void_p(radius or None), int(cap), C.c_void_p(out_first or None),
            C.c_void_p(out_ids or None), C.c_void_p(out_d or None), C.c_void_p(status or None), C.c_void_p(out_total or None),
            C.c_void_p(stream or None)))

    @staticmethod
    def _negotiate(call, nq, cap):
        """the two calls of the radius methods: room for `cap` entries (default 64 per query), then exactly the total"""
        room = max(64 * nq, 1) if cap is None else int(cap)
        first, total, ids, d = call(room)
        if total > room:
            first, total, ids, d = call(total)
        if ids is None:
            ids, d = np.empty(0, dtype=np.uint64), np.empty(0, dtype=np.float32)
        return first, ids[:total], d[:total]

    def _exact_radius_list_call(self, who, fn, handle, queries, qids, filt, radius, exclude):
        """the arguments of phnsw_search_exact_radius_labeled / _ranged, packed -> call(room) -> (first, total, ids, d);
        filt: the u32 arrays [nq] that take the bitmap's place (want, or lo and hi)"""
        if radius is None:
            raise ValueError("%s: pass radius (a scalar or one per query)" % who)
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            if q.shape[1] != self.store.dim:
                raise ValueError("%s: queries of shape [nq, %d], got %r" % (who, self.store.dim, q.shape))
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        filt = filt(nq)

        def call(room):
            first = np.zeros(nq + 1, dtype=np.uint64)
            total = C.c_uint64(0)
            ids = np.empty(room, dtype=np.uint64) if room else None
            d = np.empty(room, dtype=np.float32) if room else None
            check(fn(self._h, handle._h, _p(q), _p(qi), nq, _p(ex), *[_p(f) for f in filt], _p(r), int(room), _p(first), _p(ids),
                     _p(d), C.byref(total)))
            return first, int(total.value), ids, d
        return nq, call

    def _radius_labeled_call(self, who, queries, qids, labels, want, radius, exclude):
        if (queries is None) == (qids is None):
            raise ValueError("%s: pass queries or qids (exactly one)" % who)
        if not isinstance(labels, Labels):
            raise TypeError("%s: labels must be a Labels made for this index" % who)
        return self._exact_radius_list_call(who, lib().phnsw_search_exact_radius_labeled, labels, queries, qids,
                                            lambda nq: (pack_labels(want, nq, "want"),), radius, exclude)

    def _radius_ranged_call(self, who, queries, qids, attr, lo, hi, radius, exclude):
        if (queries is None) == (qids is None):
            raise ValueError("%s: pass queries or qids (exactly one)" % who)
        if not isinstance(attr, Attribute):
            raise TypeError("%s: attr must be an Attribute made for this index" % who)
        return self._exact_radius_list_call(who, lib().phnsw_search_exact_radius_ranged, attr, queries, qids,
                                            lambda nq: attr.bounds(who, lo, hi, nq), radius, exclude)

    def search_exact_radius_labeled(self, queries=None, qids=None, labels=None, want=None, radius=None, exclude=None, cap=None):
        """search_exact_radius by row label (phnsw_search_exact_radius_labeled): every vector `labels` lists under want[i]
        closer to query i than radius[i] -- the segments of search_exact_radius(allow=(label column == want[i])) called
        once per query, bit for bit, in ONE call from posting lists.  want as for search_exact_labeled (-1, LABEL_NONE or a
        label nobody carries: an empty segment); radius, exclude, cap and the size negotiation as for search_exact_radius.
        Every store kind the label scan takes (a per-sub-space PqStore too).  Measured on 1M x 768 f32 rows, 10 000
        queries: the time of search_exact_labeled's per-query scan plus 0.2 to 1.2 ms of sort and unpack (4.1 / 31 / 320 ms
        at lists of 1000 / 10 000 / 100 000 rows); against one search_exact_radius call per label it wins at 1000 labels
        (about 40 to 1), is level at 64 and LOSES ten to one at 8 (profiles/radius_list/README.md).  Returns (first[nq + 1] u64, ids[total] u64, d[total] f32)"""
        nq, call = self._radius_labeled_call("search_exact_radius_labeled", queries, qids, labels, want, radius, exclude)
        return self._negotiate(call, nq, cap)

    def count_exact_radius_labeled(self, queries=None, qids=None, labels=None, want=None, radius=None, exclude=None):
        """the count-only form of search_exact_radius_labeled (cap 0, no arrays): first[nq + 1] u64"""
        _, call = self._radius_labeled_call("count_exact_radius_labeled", queries, qids, labels, want, radius, exclude)
        return call(0)[0]

    def search_exact_radius_labeled_device(self, labels, nq, radius, cap, out_first, out_ids, out_d, status, out_total, queries=0,
                                           ldq=0, qids=0, exclude=0, want=0, stream=0):
        """zero-copy form (phnsw_search_exact_radius_labeled_device): device pointers as integers, as for
        search_exact_radius_device with want = u32 labels [nq] in the bitmap's place.  Synchronises `stream` once (the
        total) when cap > 0, never with cap 0"""
        if not isinstance(labels, Labels):
            raise TypeError("search_exact_radius_labeled_device: labels must be a Labels made for this index")
        check(lib().phnsw_search_exact_radius_labeled_device(
            self._h, labels._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.c_void_p(exclude or None),
            C.c_void_p(want or None), C.c_void_p(radius or None), int(cap), C.c_void_p(out_first or None),
            C.c_void_p(out_ids or None), C.c_void_p(out_d or None), C.c_void_p(status or None), C.c_void_p(out_total or None),
            C.c_void_p(stream or None)))

    def search_exact_radius_ranged(self, queries=None, qids=None, attr=None, lo=None, hi=None, radius=None, exclude=None, cap=None):
        """search_exact_radius by a numeric range (phnsw_search_exact_radius_ranged): every vector `attr` lists with
        lo[i] <= value <= hi[i] closer to query i than radius[i] -- the segments of search_exact_radius(allow=(the listed
        vectors inside the range)) called once per query, bit for bit, in ONE call from spans of the sorted column.  lo / hi
        as for search_exact_ranged (lo > hi: an empty segment); radius, exclude, cap and the size negotiation as for
        search_exact_radius.  Measured on 1M x 768 f32 rows, 10 000 queries: the time of search_exact_ranged plus 0.2 to
        1.2 ms of sort and unpack (4.4 / 42 / 391 ms at windows of 1000 / 10 000 / 100 000 rows; profiles/radius_list/README.md).
        Returns (first[nq + 1] u64, ids[total] u64, d[total] f32)"""
        nq, call = self._radius_ranged_call("search_exact_radius_ranged", queries, qids, attr, lo, hi, radius, exclude)
        return self._negotiate(call, nq, cap)

    def count_exact_radius_ranged(self, queries=None, qids=None, attr=None, lo=None, hi=None, radius=None, exclude=None):
        """the count-only form of search_exact_radius_ranged (cap 0, no arrays): first[nq + 1] u64"""
        _, call = self._radius_ranged_call("count_exact_radius_ranged", queries, qids, attr, lo, hi, radius, exclude)
        return call(0)[0]

    def search_exact_radius_ranged_device(self, attr, nq, radius, cap, out_first, out_ids, out_d, status, out_total, queries=0,
                                          ldq=0, qids=0, exclude=0, lo=0, hi=0, stream=0):
        """zero-copy form (phnsw_search_exact_radius_ranged_device): as search_exact_radius_labeled_device with lo, hi =
        u32 KEYS [nq] (Attribute.key) in want's place"""
        if not isinstance(attr, Attribute):
            raise TypeError("search_exact_radius_ranged_device: attr must be an Attribute made for this index")
        check(lib().phnsw_search_exact_radius_ranged_device(
            self._h, attr._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.c_void_p(exclude or None),
            C.c_void_p(lo or None), C.c_void_p(hi or None), C.c_void_p(radius or None), int(cap), C.c_void_p(out_first or None),
            C.c_void_p(out_ids or None), C.c_void_p(out_d or None), C.c_void_p(status or None), C.c_void_p(out_total or None),
            C.c_void_p(stream or None)))

    def search_radius(self, queries=None, qids=None, radius=None, sp=None, exclude=None, max_out=64, stats=False,
                      exact_fallback=False):
        """radius search by graph walk (phnsw_search_batch_radius): the plain descent, then threshold_nn's doubling-queue
        loop on the bottom layer against radius[q] (a scalar broadcasts); approximate, like every walk.  Rows of max_out
        entries (1..1024), the nearest of the entries inside the radius; len[q] counts ALL of them and may exceed
        max_out.  status[q]: 0, or 6 when the queue would pass 1024 entries (an empty row, len 0).
        Returns (ids[nq, max_out] u64, d f32, len[nq] u64, status[nq] u32) and the stats [nq, 2] with stats=True.
        exact_fallback=True: the queries with status 6 or len > max_out are answered again by search_exact_radius, and
        the return is CSR as from that call, (first[nq + 1], ids, d) -- the walk's rows elsewhere -- then status (0 for
        the re-answered queries) and the stats with stats=True.  With sp.upper_layer_candidate_count equal to
        sp.number_of_candidates the queue starts full and the loop ends after one call: pass a smaller upper count.
        Measured on 1M x 768 f32 rows: 1.5 to 3 times the plain walk, 0.40 to 0.96 of the exact rows (profiles/radius/README.md)."""
        if (queries is None) == (qids is None):
            raise ValueError("search_radius: pass queries or qids (exactly one)")
        if radius is None:
            raise ValueError("search_radius: pass radius (a scalar or one per query)")
        sp = sp or SearchParameters()
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            assert q.shape[1] == self.store.dim
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,)))
        w = max(int(max_out), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        st = np.zeros((nq, 2), dtype=np.uint64) if stats else None
        status = np.zeros(nq, dtype=np.uint32)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_batch_radius(self._h, _p(q), _p(qi), nq, C.byref(sp), _p(ex), _p(r), int(max_out), _p(ids),
                                              _p(d), _p(ln), _p(st), _p(status)))
        if not exact_fallback:
            return (ids, d, ln, status, st) if stats else (ids, d, ln, status)
        again = np.nonzero((status == 6) | (ln > w))[0]
        seg_i = [ids[i, :int(ln[i])] for i in range(nq)]
        seg_d = [d[i, :int(ln[i])] for i in range(nq)]
        if len(again):
            f, xi, xd = self.search_exact_radius(queries=None if q is None else q[again], qids=None if qi is None else qi[again],
                                                 radius=r[again], exclude=None if ex is None else ex[again])
            for j, i in enumerate(again):
                seg_i[i], seg_d[i] = xi[int(f[j]):int(f[j + 1])], xd[int(f[j]):int(f[j + 1])]
            status = status.copy()
            status[again] = 0
        first = np.zeros(nq + 1, dtype=np.uint64)
        first[1:] = np.cumsum([len(x) for x in seg_i], dtype=np.uint64)
        out_i = np.concatenate(seg_i) if nq else np.empty(0, dtype=np.uint64)
        out_d = np.concatenate(seg_d) if nq else np.empty(0, dtype=np.float32)
        return (first, out_i, out_d, status, st) if stats else (first, out_i, out_d, status)

    def search_radius_device(self, nq, sp, radius, max_out, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0,
                             exclude=0, out_stats=0, stream=0):
        """zero-copy form (phnsw_search_batch_radius_device): device pointers as integers; radius f32 [nq], u32 ids
        [nq, max_out] padded with 0xFFFFFFFF, u32 len / status [nq], u32 stats [nq, 2]; enqueued on `stream`"""
        check(lib().phnsw_search_batch_radius_device(
            self._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp), C.c_void_p(exclude or None),
            C.c_void_p(radius or None), int(max_out), C.c_void_p(out_ids or None), C.c_void_p(out_d or None),
            C.c_void_p(out_len or None), C.c_void_p(out_stats or None), C.c_void_p(status or None), C.c_void_p(stream or None)))

    def search_exact_grouped(self, queries=None, qids=None, allows=None, allow_of=None, exclude=None, k=10):
        """search_exact_filtered for a TABLE of allow-lists and one selector per query (phnsw_search_exact_grouped): the
        batch is grouped by bitmap on the device and every group runs as search_exact_shared runs its batch -- the same
        rows as search_exact_filtered(allow=allows[allow_of]), bit for bit, without a bitmap per query.  allows: a bool
        array [nb, n] or packed u32 words [nb, >= ceil(n/32)] (the row length is the stride); allow_of: integers [nq],
        a bitmap's number, or FILTER_ALL / -1 = no bitmap, every vector of the index.  The default of set_filter is not
        consulted.  Exactly one of queries / qids.  f32, f16, i8 and i8q stores with rows up to 1536 floats.
        Measured on 1M x 768 f32 rows, 10 000 queries, k = 10: 1.8 to 11.7 times faster than the scan with per-query
        bitmaps at 1 to 64 bitmaps, four times SLOWER at 1000 bitmaps of 10 queries each
        (profiles/filter_grouped/README.md).
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq])"""
        if (queries is None) == (qids is None):
            raise ValueError("search_exact_grouped: pass queries or qids (exactly one)")
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            assert q.shape[1] == self.store.dim
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        words, stride = pack_allow_table(allows, self.store.n)
        sel = pack_allow_of(allow_of, nq)
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_exact_grouped(self._h, _p(q), _p(qi), nq, _p(ex), _p(words), stride, words.shape[0], _p(sel),
                                               int(k), _p(ids), _p(d), _p(ln)))
        return ids, d, ln

    def search_exact_grouped_device(self, nq, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                                    allows=0, allow_stride=0, nallows=0, allow_of=0, stream=0):
        """zero-copy form (phnsw_search_exact_grouped_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF; allows = nallows packed bitmaps allow_stride words apart, allow_of = u32 selectors [nq].  status 4 =
        a stored query id at or past n, 6 = a selector outside the table, 7 = a bitmap changed under the call (empty
        rows).  Synchronises `stream` once, to read the groups and their candidate counts back"""
        check(lib().phnsw_search_exact_grouped_device(
            self._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.c_void_p(exclude or None),
            C.c_void_p(allows or None), int(allow_stride), int(nallows), C.c_void_p(allow_of or None), int(k),
            C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(status), C.c_void_p(stream or None)))

    def search_exact_labeled(self, queries=None, qids=None, labels=None, want=None, exclude=None, k=10):
        """search_exact_filtered by row label (phnsw_search_exact_labeled): query i may return the vectors `labels` lists
        under want[i] -- the same rows as search_exact_filtered(allow=(label column == want[i])), bit for bit, from
        posting lists instead of bitmaps.  labels: a Labels made for this index; want: integers [nq] within u32, -1 or
        LABEL_NONE (or a label nobody carries) = an empty row.  Exactly one of queries / qids.  Every store kind the
        scan takes.  Measured on 1M x 768 f32 rows, 10 000 queries, k = 10: 1.4 to 3.8 times faster than the scan with
        per-query bitmaps; 0.26 to 0.69 times as fast as search_exact_grouped at 1 and 8 labels (it LOSES there), 1.5 and 35
        times faster at 64 and 1000 labels (profiles/filter_labeled/README.md).
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq])"""
        if (queries is None) == (qids is None):
            raise ValueError("search_exact_labeled: pass queries or qids (exactly one)")
        if not isinstance(labels, Labels):
            raise TypeError("search_exact_labeled: labels must be a Labels made for this index")
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            assert q.shape[1] == self.store.dim
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        w32 = pack_labels(want, nq, "want")
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_exact_labeled(self._h, labels._h, _p(q), _p(qi), nq, _p(ex), _p(w32), int(k), _p(ids), _p(d),
                                               _p(ln)))
        return ids, d, ln

    def search_exact_labeled_device(self, labels, nq, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                                    want=0, stream=0):
        """zero-copy form (phnsw_search_exact_labeled_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF; want = u32 labels [nq].  status 4 = a stored query id at or past n (an empty row).  Enqueued on
        `stream`; never synchronises it"""
        if not isinstance(labels, Labels):
            raise TypeError("search_exact_labeled_device: labels must be a Labels made for this index")
        check(lib().phnsw_search_exact_labeled_device(
            self._h, labels._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.c_void_p(exclude or None),
            C.c_void_p(want or None), int(k), C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(status),
            C.c_void_p(stream or None)))

    def search_exact_labelset(self, queries=None, qids=None, labels=None, want=None, exclude=None, k=10):
        """search_exact_labeled for a SET of labels per query, `label IN (a, b, c)` (phnsw_search_exact_labelset): query i
        may return the vectors `labels` lists under any label of want[i] -- the same rows as
        search_exact_filtered(allow=(label column in want[i])), bit for bit.  want: as pack_label_sets takes it; an empty
        set, LABEL_NONE and labels nobody carries give nothing, a label twice counts once.  Exactly one of queries / qids.
        This is the exact scan; search_batch_labelset is the graph walk by set, search_labelset the routed call.
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq])"""
        if (queries is None) == (qids is None):
            raise ValueError("search_exact_labelset: pass queries or qids (exactly one)")
        if not isinstance(labels, Labels):
            raise TypeError("search_exact_labelset: labels must be a Labels made for this index")
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            assert q.shape[1] == self.store.dim
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        first, values = pack_label_sets(want, nq)
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_exact_labelset(self._h, labels._h, _p(q), _p(qi), nq, _p(ex), _p(first),
                                                _p(values) if len(values) else None, int(k), _p(ids), _p(d), _p(ln)))
        return ids, d, ln

    def search_exact_labelset_device(self, labels, nq, nwant, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0,
                                     exclude=0, want_first=0, want_values=0, stream=0):
        """zero-copy form (phnsw_search_exact_labelset_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF; want_first = u32 offsets [nq + 1], want_values = u32 labels [nwant].  status 4 = a stored query id at
        or past n, 8 = a range of want_first that is not sound (empty rows).  Enqueued on `stream`; never synchronises
        it"""
        if not isinstance(labels, Labels):
            raise TypeError("search_exact_labelset_device: labels must be a Labels made for this index")
        check(lib().phnsw_search_exact_labelset_device(
            self._h, labels._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.c_void_p(exclude or None),
            C.c_void_p(want_first or None), C.c_void_p(want_values or None), int(nwant), int(k), C.c_void_p(out_ids),
            C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(status), C.c_void_p(stream or None)))

    def _labeled_args(self, call, queries, qids, labels, want):
        """the checks the calls by label make before they reach the library: a Labels, exactly one of queries / qids,
        want as pack_labels takes it.  Returns (q, qi, nq, want u32 [nq])"""
        q, qi, nq = self._label_queries(call, queries, qids, labels)
        return q, qi, nq, pack_labels(want, nq, "want")

    def _labelset_args(self, call, queries, qids, labels, want):
        """... of the calls by a set of labels: want as pack_label_sets takes it.  Returns (q, qi, nq, first u32 [nq + 1],
        values u32 [nwant])"""
        q, qi, nq = self._label_queries(call, queries, qids, labels)
        first, values = pack_label_sets(want, nq)
        return q, qi, nq, first, values

    def _label_queries(self, call, queries, qids, labels):
        if not isinstance(labels, Labels):
            raise TypeError("%s: labels must be a Labels made for this index" % call)
        if (queries is None) == (qids is None):
            raise ValueError("%s: pass queries or qids (exactly one)" % call)
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            if q.shape[1] != self.store.dim:
                raise ValueError("%s: queries of shape [nq, %d], got %r" % (call, self.store.dim, q.shape))
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        return q, qi, nq

    def search_batch_labeled(self, queries=None, qids=None, sp=None, labels=None, want=None, strict=False, exclude=None,
                             upto=0, stats=False, k=None):
        """search_batch_filtered by row label (phnsw_search_batch_labeled): the graph walk of query i restricted to the
        vectors `labels` lists under want[i] -- the rows, lengths and stats of search_batch_filtered(allow=(the vectors
        listed under want[i])), bit for bit, without a bitmap per query: the kernels test the handle's label column.
        labels: a Labels made for this index; want: integers [nq] within u32, -1 or LABEL_NONE (or a label nobody carries)
        = the row an all-zero bitmap gives.  A post-filter like search_batch_filtered: about number_of_candidates * list
        length / vector_count results come back (search_labeled completes rows).  The entry vector may be returned
        although its label differs; strict=True removes it.  set_filter's default is not consulted.  Measured on 1M x 768
        f32 rows, ef 256 / probe_depth 8, 10 000 queries, 2 to 1000 labels: the device form took 0.990 to 0.997 of the
        bitmap call's kernel time (run-to-run spread of either: under 1 %) and 0.36 to 0.54 of it with the bitmaps' upload
        counted (profiles/labeled_walk/README.md); the host forms were not timed.
        Returns (ids[nq, k or ef] u64, d f32, len[nq]) and the stats with stats=True"""
        q, qi, nq, w32 = self._labeled_args("search_batch_labeled", queries, qids, labels, want)
        sp = sp or SearchParameters()
        ef = sp.number_of_candidates
        w = ef if k is None else int(k)
        if w < 0:
            raise ValueError("search_batch_labeled: k must not be negative")
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        st = np.zeros((nq, 2), dtype=np.uint64) if stats else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_batch_labeled(self._h, labels._h, _p(q), _p(qi), nq, C.byref(sp), upto, _p(ex), _p(w32),
                                               FILTER_STRICT if strict else 0, 0 if k is None else w, _p(ids), _p(d), _p(ln),
                                               _p(st)))
        return (ids, d, ln, st) if stats else (ids, d, ln)

    def search_batch_labeled_device(self, labels, nq, sp, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                                    want=0, strict=False, out_stats=0, upto=0, stream=0):
        """zero-copy form (phnsw_search_batch_labeled_device): search_batch_filtered_device with want = u32 labels [nq] (a
        device pointer, alive until the work on `stream` is done) in place of the bitmaps.  Enqueued on `stream`; never
        synchronises it"""
        if not isinstance(labels, Labels):
            raise TypeError("search_batch_labeled_device: labels must be a Labels made for this index")
        check(lib().phnsw_search_batch_labeled_device(
            self._h, labels._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp), upto,
            C.c_void_p(exclude or None), C.c_void_p(want or None), FILTER_STRICT if strict else 0, C.c_void_p(out_ids),
            C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(out_stats or None), C.c_void_p(status),
            C.c_void_p(stream or None)))

    def search_labeled(self, queries=None, qids=None, sp=None, labels=None, want=None, exclude=None, k=10, scan_below=0,
                       route=False):
        """search_filtered by row label (phnsw_search_labeled_auto): per query the posting-list scan
        (search_exact_labeled) where the list of want[i] is short (length <= scan_below, or length *
        number_of_candidates < k * vector_count), the strict graph walk by label otherwise, and the scan again for every
        query whose walk came back short.  Every row holds exactly min(k, list length - e) entries and only listed vectors
        of want[i] (e = 1 iff exclude[i] is one of them): the rows of search_filtered with the equivalent per-query
        bitmaps, bit for bit.  scan_below 0 = the library's threshold for labels, 20 000: the measured crossover of the two
        calls on 1M x 768 f32 rows, ef 256, k = 10 (scan 17.8 ms against the walk's 22.0 at 20 000 rows per label, 22.0
        against 21.5 at 25 000; profiles/labeled_walk/README.md), other shapes unmeasured; 2**64 - 1 = always scan.
        1 <= k <= sp.number_of_candidates.
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq]) and, with route=True, route[nq] u32: ROUTE_GRAPH, ROUTE_SCAN or
        ROUTE_GRAPH_THEN_SCAN"""
        q, qi, nq, w32 = self._labeled_args("search_labeled", queries, qids, labels, want)
        sp = sp or SearchParameters()
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        rt = np.zeros(nq, dtype=np.uint32) if route else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_labeled_auto(self._h, labels._h, _p(q), _p(qi), nq, C.byref(sp), _p(ex), _p(w32), int(k),
                                              int(scan_below), _p(ids), _p(d), _p(ln), _p(rt)))
        return (ids, d, ln, rt) if route else (ids, d, ln)

    def search_labeled_device(self, labels, nq, sp, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                              want=0, scan_below=0, out_route=0, stream=0):
        """device form (phnsw_search_labeled_auto_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF; want = u32 labels [nq]; out_route u32 [nq] or 0.  Like search_filtered_device it synchronises
        `stream`, up to twice"""
        if not isinstance(labels, Labels):
            raise TypeError("search_labeled_device: labels must be a Labels made for this index")
        check(lib().phnsw_search_labeled_auto_device(
            self._h, labels._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp),
            C.c_void_p(exclude or None), C.c_void_p(want or None), int(k), int(scan_below), C.c_void_p(out_ids),
            C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(out_route or None), C.c_void_p(status),
            C.c_void_p(stream or None)))

    def _ranged_args(self, call, queries, qids, attr, lo, hi):
        """the checks the calls by range make before they reach the library: an Attribute, exactly one of queries / qids,
        lo / hi as Attribute.bounds takes them.  Returns (q, qi, nq, lo u32 [nq], hi u32 [nq])"""
        if not isinstance(attr, Attribute):
            raise TypeError("%s: attr must be an Attribute made for this index" % call)
        if (queries is None) == (qids is None):
            raise ValueError("%s: pass queries or qids (exactly one)" % call)
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            if q.shape[1] != self.store.dim:
                raise ValueError("%s: queries of shape [nq, %d], got %r" % (call, self.store.dim, q.shape))
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        l32, h32 = attr.bounds(call, lo, hi, nq)
        return q, qi, nq, l32, h32

    def search_exact_ranged(self, queries=None, qids=None, attr=None, lo=None, hi=None, exclude=None, k=10):
        """search_exact_filtered by a numeric range (phnsw_search_exact_ranged): query i may return the vectors `attr`
        lists with lo[i] <= value <= hi[i], both ends inclusive -- the same rows as search_exact_filtered(allow=(the
        listed vectors inside the range)), bit for bit, from one span of the sorted column instead of a bitmap.  attr: an
        Attribute made for this index; lo / hi: scalars (broadcast), arrays [nq] in the column's dtype, or None for an
        open end; lo > hi is an empty row.  Exactly one of queries / qids.  Not measured yet (profiles/ranged/README.md).
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq])"""
        q, qi, nq, l32, h32 = self._ranged_args("search_exact_ranged", queries, qids, attr, lo, hi)
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_exact_ranged(self._h, attr._h, _p(q), _p(qi), nq, _p(ex), _p(l32), _p(h32), int(k), _p(ids),
                                              _p(d), _p(ln)))
        return ids, d, ln

    def search_exact_ranged_device(self, attr, nq, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                                   lo=0, hi=0, stream=0):
        """zero-copy form (phnsw_search_exact_ranged_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF; lo, hi = u32 KEYS [nq] (Attribute.key).  status 4 = a stored query id at or past n (an empty row).
        Enqueued on `stream`; never synchronises it"""
        if not isinstance(attr, Attribute):
            raise TypeError("search_exact_ranged_device: attr must be an Attribute made for this index")
        check(lib().phnsw_search_exact_ranged_device(
            self._h, attr._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.c_void_p(exclude or None),
            C.c_void_p(lo or None), C.c_void_p(hi or None), int(k), C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len),
            C.c_void_p(status), C.c_void_p(stream or None)))

    def search_batch_ranged(self, queries=None, qids=None, sp=None, attr=None, lo=None, hi=None, strict=False, exclude=None,
                            upto=0, stats=False, k=None):
        """search_batch_filtered by a numeric range (phnsw_search_batch_ranged): the graph walk of query i restricted to
        the vectors `attr` lists with lo[i] <= value <= hi[i] -- the rows, lengths and stats of
        search_batch_filtered(allow=(those vectors)), bit for bit, without a bitmap per query: the kernels test the
        handle's column.  A post-filter like search_batch_filtered (search_ranged completes rows); the entry vector may
        be returned although it is outside the range, strict=True removes it.  set_filter's default is not consulted.
        Not measured yet (profiles/ranged/README.md).
        Returns (ids[nq, k or ef] u64, d f32, len[nq]) and the stats with stats=True"""
        q, qi, nq, l32, h32 = self._ranged_args("search_batch_ranged", queries, qids, attr, lo, hi)
        sp = sp or SearchParameters()
        ef = sp.number_of_candidates
        w = ef if k is None else int(k)
        if w < 0:
            raise ValueError("search_batch_ranged: k must not be negative")
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        st = np.zeros((nq, 2), dtype=np.uint64) if stats else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_batch_ranged(self._h, attr._h, _p(q), _p(qi), nq, C.byref(sp), upto, _p(ex), _p(l32), _p(h32),
                                              FILTER_STRICT if strict else 0, 0 if k is None else w, _p(ids), _p(d), _p(ln),
                                              _p(st)))
        return (ids, d, ln, st) if stats else (ids, d, ln)

    def search_batch_ranged_device(self, attr, nq, sp, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                                   lo=0, hi=0, strict=False, out_stats=0, upto=0, stream=0):
        """zero-copy form (phnsw_search_batch_ranged_device): search_batch_filtered_device with lo, hi = u32 KEYS [nq]
        (device pointers, alive until the work on `stream` is done) in place of the bitmaps.  Enqueued on `stream`; never
        synchronises it"""
        if not isinstance(attr, Attribute):
            raise TypeError("search_batch_ranged_device: attr must be an Attribute made for this index")
        check(lib().phnsw_search_batch_ranged_device(
            self._h, attr._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp), upto,
            C.c_void_p(exclude or None), C.c_void_p(lo or None), C.c_void_p(hi or None), FILTER_STRICT if strict else 0,
            C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(out_stats or None), C.c_void_p(status),
            C.c_void_p(stream or None)))

    def search_ranged(self, queries=None, qids=None, sp=None, attr=None, lo=None, hi=None, exclude=None, k=10, scan_below=0,
                      route=False):
        """search_filtered by a numeric range (phnsw_search_ranged_auto): per query the span scan (search_exact_ranged)
        where the range holds few rows (count <= scan_below, or count * number_of_candidates < k * vector_count), the
        strict graph walk by range otherwise, and the scan again for every query whose walk came back short.  Every row
        holds exactly min(k, count - e) entries and only listed vectors inside the range (e = 1 iff exclude[i] is one of
        them): the rows of search_filtered with the equivalent per-query bitmaps, bit for bit.  scan_below 0 = the
        library's threshold for ranges, 20 000: UNMEASURED, the one-label figure (the true crossover is expected below
        it: the range scan has no tile path); 2**64 - 1 = always scan.  1 <= k <= sp.number_of_candidates.
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq]) and, with route=True, route[nq] u32: ROUTE_GRAPH, ROUTE_SCAN or
        ROUTE_GRAPH_THEN_SCAN"""
        q, qi, nq, l32, h32 = self._ranged_args("search_ranged", queries, qids, attr, lo, hi)
        sp = sp or SearchParameters()
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        rt = np.zeros(nq, dtype=np.uint32) if route else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_ranged_auto(self._h, attr._h, _p(q), _p(qi), nq, C.byref(sp), _p(ex), _p(l32), _p(h32), int(k),
                                             int(scan_below), _p(ids), _p(d), _p(ln), _p(rt)))
        return (ids, d, ln, rt) if route else (ids, d, ln)

    def search_ranged_device(self, attr, nq, sp, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0, lo=0,
                             hi=0, scan_below=0, out_route=0, stream=0):
        """device form (phnsw_search_ranged_auto_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF; lo, hi = u32 KEYS [nq]; out_route u32 [nq] or 0.  Like search_filtered_device it synchronises
        `stream`, up to twice"""
        if not isinstance(attr, Attribute):
            raise TypeError("search_ranged_device: attr must be an Attribute made for this index")
        check(lib().phnsw_search_ranged_auto_device(
            self._h, attr._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp),
            C.c_void_p(exclude or None), C.c_void_p(lo or None), C.c_void_p(hi or None), int(k), int(scan_below),
            C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(out_route or None), C.c_void_p(status),
            C.c_void_p(stream or None)))

    def _label_ranged_args(self, call, queries, qids, attr, want, lo, hi):
        """the checks the calls by label and range make before they reach the library: a LabeledAttribute, exactly one of
        queries / qids, want as LabeledAttribute.wanted and lo / hi as Attribute.bounds take them.  Returns (q, qi, nq,
        want u32 [nq], lo u32 [nq], hi u32 [nq])"""
        if not isinstance(attr, LabeledAttribute):
            raise TypeError("%s: attr must be a LabeledAttribute made for this index" % call)
        if (queries is None) == (qids is None):
            raise ValueError("%s: pass queries or qids (exactly one)" % call)
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            if q.shape[1] != self.store.dim:
                raise ValueError("%s: queries of shape [nq, %d], got %r" % (call, self.store.dim, q.shape))
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        w32 = attr.wanted(call, want, nq)
        l32, h32 = attr.bounds(call, lo, hi, nq)
        return q, qi, nq, w32, l32, h32

    def search_exact_label_ranged(self, queries=None, qids=None, attr=None, want=None, lo=None, hi=None, exclude=None, k=10):
        """search_exact_filtered by a label and a numeric range (phnsw_search_exact_label_ranged): query i may return the
        vectors `attr` lists under label want[i] with lo[i] <= value <= hi[i], both ends inclusive -- the same rows as
        search_exact_filtered(allow=(those vectors)), bit for bit, from one span of the sorted column instead of a
        bitmap.  attr: a LabeledAttribute made for this index; want: a label or an array [nq] (-1 or LABEL_NONE: an empty
        row); lo / hi: scalars (broadcast), arrays [nq] in the column's dtype, or None for an open end; lo > hi is an
        empty row.  Exactly one of queries / qids.  Not measured yet (profiles/label_ranged/README.md).
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq])"""
        q, qi, nq, w32, l32, h32 = self._label_ranged_args("search_exact_label_ranged", queries, qids, attr, want, lo, hi)
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_exact_label_ranged(self._h, attr._h, _p(q), _p(qi), nq, _p(ex), _p(w32), _p(l32), _p(h32),
                                                    int(k), _p(ids), _p(d), _p(ln)))
        return ids, d, ln

    def search_exact_label_ranged_device(self, attr, nq, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0,
                                         exclude=0, want=0, lo=0, hi=0, stream=0):
        """zero-copy form (phnsw_search_exact_label_ranged_device): device pointers as integers, u32 ids [nq, k] padded
        with 0xFFFFFFFF; want = u32 labels [nq], lo, hi = u32 KEYS [nq] (LabeledAttribute.key).  status 4 = a stored query
        id at or past n (an empty row).  Enqueued on `stream`; never synchronises it"""
        if not isinstance(attr, LabeledAttribute):
            raise TypeError("search_exact_label_ranged_device: attr must be a LabeledAttribute made for this index")
        check(lib().phnsw_search_exact_label_ranged_device(
            self._h, attr._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.c_void_p(exclude or None),
            C.c_void_p(want or None), C.c_void_p(lo or None), C.c_void_p(hi or None), int(k), C.c_void_p(out_ids),
            C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(status), C.c_void_p(stream or None)))

    def search_batch_label_ranged(self, queries=None, qids=None, sp=None, attr=None, want=None, lo=None, hi=None, strict=False,
                                  exclude=None, upto=0, stats=False, k=None):
        """search_batch_filtered by a label and a numeric range (phnsw_search_batch_label_ranged): the graph walk of query
        i restricted to the vectors `attr` lists under want[i] with lo[i] <= value <= hi[i] -- the rows, lengths and stats
        of search_batch_filtered(allow=(those vectors)), bit for bit, without a bitmap per query: the kernels test the
        handle's column of composites, one 8-byte load per id.  A post-filter like search_batch_filtered
        (search_label_ranged completes rows); the entry vector may be returned although it does not pass, strict=True
        removes it.  set_filter's default is not consulted.  Not measured yet (profiles/label_ranged/README.md).
        Returns (ids[nq, k or ef] u64, d f32, len[nq]) and the stats with stats=True"""
        q, qi, nq, w32, l32, h32 = self._label_ranged_args("search_batch_label_ranged", queries, qids, attr, want, lo, hi)
        sp = sp or SearchParameters()
        ef = sp.number_of_candidates
        w = ef if k is None else int(k)
        if w < 0:
            raise ValueError("search_batch_label_ranged: k must not be negative")
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        st = np.zeros((nq, 2), dtype=np.uint64) if stats else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_batch_label_ranged(self._h, attr._h, _p(q), _p(qi), nq, C.byref(sp), upto, _p(ex), _p(w32),
                                                    _p(l32), _p(h32), FILTER_STRICT if strict else 0, 0 if k is None else w,
                                                    _p(ids), _p(d), _p(ln), _p(st)))
        return (ids, d, ln, st) if stats else (ids, d, ln)

    def search_batch_label_ranged_device(self, attr, nq, sp, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0,
                                         exclude=0, want=0, lo=0, hi=0, strict=False, out_stats=0, upto=0, stream=0):
        """zero-copy form (phnsw_search_batch_label_ranged_device): search_batch_filtered_device with want = u32 labels
        [nq] and lo, hi = u32 KEYS [nq] (device pointers, alive until the work on `stream` is done) in place of the
        bitmaps.  Enqueued on `stream`; never synchronises it"""
        if not isinstance(attr, LabeledAttribute):
            raise TypeError("search_batch_label_ranged_device: attr must be a LabeledAttribute made for this index")
        check(lib().phnsw_search_batch_label_ranged_device(
            self._h, attr._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp), upto,
            C.c_void_p(exclude or None), C.c_void_p(want or None), C.c_void_p(lo or None), C.c_void_p(hi or None),
            FILTER_STRICT if strict else 0, C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len),
            C.c_void_p(out_stats or None), C.c_void_p(status), C.c_void_p(stream or None)))

    def search_label_ranged(self, queries=None, qids=None, sp=None, attr=None, want=None, lo=None, hi=None, exclude=None, k=10,
                            scan_below=0, route=False):
        """search_filtered by a label and a numeric range (phnsw_search_label_ranged_auto): per query the span scan
        (search_exact_label_ranged) where the pair holds few rows (count <= scan_below, or count * number_of_candidates <
        k * vector_count), the strict graph walk otherwise, and the scan again for every query whose walk came back
        short.  Every row holds exactly min(k, count - e) entries and only listed vectors of the label inside the range
        (e = 1 iff exclude[i] is one of them): the rows of search_filtered with the equivalent per-query bitmaps, bit for
        bit.  scan_below 0 = the library's threshold, 20 000: UNMEASURED, the ranged figure; 2**64 - 1 = always scan.
        1 <= k <= sp.number_of_candidates.
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq]) and, with route=True, route[nq] u32: ROUTE_GRAPH, ROUTE_SCAN or
        ROUTE_GRAPH_THEN_SCAN"""
        q, qi, nq, w32, l32, h32 = self._label_ranged_args("search_label_ranged", queries, qids, attr, want, lo, hi)
        sp = sp or SearchParameters()
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        rt = np.zeros(nq, dtype=np.uint32) if route else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_label_ranged_auto(self._h, attr._h, _p(q), _p(qi), nq, C.byref(sp), _p(ex), _p(w32), _p(l32),
                                                   _p(h32), int(k), int(scan_below), _p(ids), _p(d), _p(ln), _p(rt)))
        return (ids, d, ln, rt) if route else (ids, d, ln)

    def search_label_ranged_device(self, attr, nq, sp, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                                   want=0, lo=0, hi=0, scan_below=0, out_route=0, stream=0):
        """device form (phnsw_search_label_ranged_auto_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF; want = u32 labels [nq], lo, hi = u32 KEYS [nq]; out_route u32 [nq] or 0.  Like search_filtered_device
        it synchronises `stream`, up to twice"""
        if not isinstance(attr, LabeledAttribute):
            raise TypeError("search_label_ranged_device: attr must be a LabeledAttribute made for this index")
        check(lib().phnsw_search_label_ranged_auto_device(
            self._h, attr._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp),
            C.c_void_p(exclude or None), C.c_void_p(want or None), C.c_void_p(lo or None), C.c_void_p(hi or None), int(k),
            int(scan_below), C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(out_route or None),
            C.c_void_p(status), C.c_void_p(stream or None)))

    def _labelset_ranged_args(self, call, queries, qids, attr, want, lo, hi):
        """the checks the calls by a set of labels and a range make before they reach the library: a LabeledAttribute,
        exactly one of queries / qids, want as pack_label_sets and lo / hi as Attribute.bounds take them.  Returns (q, qi,
        nq, first u32 [nq + 1], values u32 [nwant], lo u32 [nq], hi u32 [nq])"""
        if not isinstance(attr, LabeledAttribute):
            raise TypeError("%s: attr must be a LabeledAttribute made for this index" % call)
        if (queries is None) == (qids is None):
            raise ValueError("%s: pass queries or qids (exactly one)" % call)
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            if q.shape[1] != self.store.dim:
                raise ValueError("%s: queries of shape [nq, %d], got %r" % (call, self.store.dim, q.shape))
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        first, values = pack_label_sets(want, nq)
        l32, h32 = attr.bounds(call, lo, hi, nq)
        return q, qi, nq, first, values, l32, h32

    def search_exact_labelset_ranged(self, queries=None, qids=None, attr=None, want=None, lo=None, hi=None, exclude=None, k=10):
        """search_exact_label_ranged for a SET of labels per query, `label IN (a, b, c) AND lo <= value <= hi`
        (phnsw_search_exact_labelset_ranged): query i may return the vectors `attr` lists under any label of want[i] with
        lo[i] <= value <= hi[i], both ends inclusive, one range per query for all its labels -- the same rows as
        search_exact_filtered(allow=(those vectors)), bit for bit, from one span of the sorted column per label.  attr: a
        LabeledAttribute made for this index; want: as pack_label_sets takes it (a list of sequences, or a (first, values)
        pair); an empty set, LABEL_NONE and labels nobody carries give nothing, a label twice counts once; lo / hi as
        search_exact_label_ranged takes them.  Exactly one of queries / qids.  Measured on 1M x 768 f32 rows, 10 000
        queries, k = 10: the device form took 1.00 to 0.74 of the scan with per-query bitmaps at sets of 1 to 32 labels
        and 0.23 to 0.67 of it with the upload counted (profiles/labelset_ranged/README.md); the host forms were not timed.
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq])"""
        q, qi, nq, first, values, l32, h32 = self._labelset_ranged_args("search_exact_labelset_ranged", queries, qids, attr, want,
                                                                        lo, hi)
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_exact_labelset_ranged(self._h, attr._h, _p(q), _p(qi), nq, _p(ex), _p(first),
                                                       _p(values) if len(values) else None, _p(l32), _p(h32), int(k), _p(ids),
                                                       _p(d), _p(ln)))
        return ids, d, ln

    def search_exact_labelset_ranged_device(self, attr, nq, nwant, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0,
                                            exclude=0, want_first=0, want_values=0, lo=0, hi=0, stream=0):
        """zero-copy form (phnsw_search_exact_labelset_ranged_device): device pointers as integers, u32 ids [nq, k] padded
        with 0xFFFFFFFF; want_first = u32 offsets [nq + 1], want_values = u32 labels [nwant], lo, hi = u32 KEYS [nq]
        (LabeledAttribute.key).  status 4 = a stored query id at or past n, 8 = a range of want_first that is not sound
        or overlaps a lower query's (empty rows; 8 wins).  Enqueued on `stream`; never synchronises it"""
        if not isinstance(attr, LabeledAttribute):
            raise TypeError("search_exact_labelset_ranged_device: attr must be a LabeledAttribute made for this index")
        check(lib().phnsw_search_exact_labelset_ranged_device(
            self._h, attr._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.c_void_p(exclude or None),
            C.c_void_p(want_first or None), C.c_void_p(want_values or None), int(nwant), C.c_void_p(lo or None),
            C.c_void_p(hi or None), int(k), C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(status),
            C.c_void_p(stream or None)))

    def search_batch_labelset_ranged(self, queries=None, qids=None, sp=None, attr=None, want=None, lo=None, hi=None,
                                     strict=False, exclude=None, upto=0, stats=False, k=None):
        """search_batch_label_ranged for a SET of labels per query (phnsw_search_batch_labelset_ranged): the graph walk of
        query i restricted to the vectors `attr` lists under any label of want[i] with lo[i] <= value <= hi[i] -- the rows,
        lengths and stats of search_batch_filtered(allow=(those vectors)), bit for bit, without a bitmap per query: the
        kernels test the handle's column of composites, one 8-byte load per id, against the set and the range.  A
        post-filter like search_batch_filtered (search_labelset_ranged completes rows); the entry vector may be returned
        although it does not pass, strict=True removes it.  The membership test costs time linear in the length of a set.
        set_filter's default is not consulted.  Measured on 1M x 768 f32 rows, ef 256 / probe_depth 8, 10 000 queries: the
        device form took 1.00 to 1.01 of the bitmap call's kernel time and 0.46 to 0.52 of it with the upload counted
        (profiles/labelset_ranged/README.md); the host forms were not timed.
        Returns (ids[nq, k or ef] u64, d f32, len[nq]) and the stats with stats=True"""
        q, qi, nq, first, values, l32, h32 = self._labelset_ranged_args("search_batch_labelset_ranged", queries, qids, attr, want,
                                                                        lo, hi)
        sp = sp or SearchParameters()
        ef = sp.number_of_candidates
        w = ef if k is None else int(k)
        if w < 0:
            raise ValueError("search_batch_labelset_ranged: k must not be negative")
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        st = np.zeros((nq, 2), dtype=np.uint64) if stats else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_batch_labelset_ranged(self._h, attr._h, _p(q), _p(qi), nq, C.byref(sp), upto, _p(ex), _p(first),
                                                       _p(values) if len(values) else None, _p(l32), _p(h32),
                                                       FILTER_STRICT if strict else 0, 0 if k is None else w, _p(ids), _p(d),
                                                       _p(ln), _p(st)))
        return (ids, d, ln, st) if stats else (ids, d, ln)

    def search_batch_labelset_ranged_device(self, attr, nq, nwant, sp, out_ids, out_d, out_len, status, queries=0, ldq=0,
                                            qids=0, exclude=0, want_first=0, want_values=0, lo=0, hi=0, strict=False,
                                            out_stats=0, upto=0, stream=0):
        """zero-copy form (phnsw_search_batch_labelset_ranged_device): search_batch_labelset_device with the handle and lo,
        hi = u32 KEYS [nq] (device pointers, alive until the work on `stream` is done).  status 8 = a range of want_first
        that is not inside [0, nwant] or runs backwards: that query does not walk (empty row, stats 0); overlapping ranges
        are not detected here.  Enqueued on `stream`; never synchronises it"""
        if not isinstance(attr, LabeledAttribute):
            raise TypeError("search_batch_labelset_ranged_device: attr must be a LabeledAttribute made for this index")
        check(lib().phnsw_search_batch_labelset_ranged_device(
            self._h, attr._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp), upto,
            C.c_void_p(exclude or None), C.c_void_p(want_first or None), C.c_void_p(want_values or None), int(nwant),
            C.c_void_p(lo or None), C.c_void_p(hi or None), FILTER_STRICT if strict else 0, C.c_void_p(out_ids),
            C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(out_stats or None), C.c_void_p(status),
            C.c_void_p(stream or None)))

    def search_labelset_ranged(self, queries=None, qids=None, sp=None, attr=None, want=None, lo=None, hi=None, exclude=None,
                               k=10, scan_below=0, route=False):
        """search_label_ranged for a SET of labels per query (phnsw_search_labelset_ranged_auto): per query the span scan
        (search_exact_labelset_ranged) where the set and the range hold few rows (count <= scan_below, or count *
        number_of_candidates < k * vector_count, count as LabeledAttribute.count_sets gives it), the strict graph walk
        otherwise, and the scan again for every query whose walk came back short.  Every row holds exactly min(k, count -
        e) entries and only candidates (e = 1 iff exclude[i] is one of them): the rows of search_filtered with the
        equivalent per-query bitmaps, bit for bit.  scan_below 0 = the library's threshold, 5 000 rows of the union: measured
        at sets of 4 labels on 1M x 768 f32 rows, ef 256, k = 10 (scan 20.8 ms against the walk's 23.6 at 5 000, 40.2
        against 22.3 at 10 000; profiles/labelset_ranged/README.md), other shapes unmeasured; 2**64 - 1 = always scan.
        1 <= k <= sp.number_of_candidates.
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq]) and, with route=True, route[nq] u32: ROUTE_GRAPH, ROUTE_SCAN or
        ROUTE_GRAPH_THEN_SCAN"""
        q, qi, nq, first, values, l32, h32 = self._labelset_ranged_args("search_labelset_ranged", queries, qids, attr, want, lo, hi)
        sp = sp or SearchParameters()
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        rt = np.zeros(nq, dtype=np.uint32) if route else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_labelset_ranged_auto(self._h, attr._h, _p(q), _p(qi), nq, C.byref(sp), _p(ex), _p(first),
                                                      _p(values) if len(values) else None, _p(l32), _p(h32), int(k),
                                                      int(scan_below), _p(ids), _p(d), _p(ln), _p(rt)))
        return (ids, d, ln, rt) if route else (ids, d, ln)

    def search_labelset_ranged_device(self, attr, nq, nwant, sp, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0,
                                      exclude=0, want_first=0, want_values=0, lo=0, hi=0, scan_below=0, out_route=0, stream=0):
        """device form (phnsw_search_labelset_ranged_auto_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF; want_first = u32 offsets [nq + 1], want_values = u32 labels [nwant], lo, hi = u32 KEYS [nq]; out_route
        u32 [nq] or 0.  status 8 where search_exact_labelset_ranged_device reports it (a range fault, an overlap with a
        lower query): scanned, empty.  Like search_label_ranged_device it synchronises `stream`, up to twice"""
        if not isinstance(attr, LabeledAttribute):
            raise TypeError("search_labelset_ranged_device: attr must be a LabeledAttribute made for this index")
        check(lib().phnsw_search_labelset_ranged_auto_device(
            self._h, attr._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp),
            C.c_void_p(exclude or None), C.c_void_p(want_first or None), C.c_void_p(want_values or None), int(nwant),
            C.c_void_p(lo or None), C.c_void_p(hi or None), int(k), int(scan_below), C.c_void_p(out_ids), C.c_void_p(out_d),
            C.c_void_p(out_len), C.c_void_p(out_route or None), C.c_void_p(status), C.c_void_p(stream or None)))

    def search_batch_labelset(self, queries=None, qids=None, sp=None, labels=None, want=None, strict=False, exclude=None,
                              upto=0, stats=False, k=None):
        """search_batch_labeled for a SET of labels per query, `label IN (a, b, c)` (phnsw_search_batch_labelset): the
        graph walk of query i restricted to the vectors `labels` lists under any label of want[i] -- the rows, lengths and
        stats of search_batch_filtered(allow=(label column in want[i])), bit for bit, without a bitmap per query.  want: as
        pack_label_sets takes it; an empty set, LABEL_NONE and labels nobody carries give what an all-zero bitmap gives, a
        label twice counts once, the order inside a set does not matter.  A post-filter like search_batch_labeled
        (search_labelset completes rows); the entry vector may be returned although its label is not wanted, strict=True
        removes it.  The membership test costs time linear in the length of a set.  Measured on 1M x 768 f32 rows, ef 256 /
        probe_depth 8, 10 000 queries, sets of 1, 4 and 32 out of 1000 labels: the device form took 0.99 to 1.00 of the
        bitmap call's kernel time and 0.49 to 0.54 of it with the upload counted (profiles/labelset_walk/README.md); the
        host forms were not timed.
        Returns (ids[nq, k or ef] u64, d f32, len[nq]) and the stats with stats=True"""
        q, qi, nq, first, values = self._labelset_args("search_batch_labelset", queries, qids, labels, want)
        sp = sp or SearchParameters()
        ef = sp.number_of_candidates
        w = ef if k is None else int(k)
        if w < 0:
            raise ValueError("search_batch_labelset: k must not be negative")
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        st = np.zeros((nq, 2), dtype=np.uint64) if stats else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_batch_labelset(self._h, labels._h, _p(q), _p(qi), nq, C.byref(sp), upto, _p(ex), _p(first),
                                                _p(values) if len(values) else None, FILTER_STRICT if strict else 0,
                                                0 if k is None else w, _p(ids), _p(d), _p(ln), _p(st)))
        return (ids, d, ln, st) if stats else (ids, d, ln)

    def search_batch_labelset_device(self, labels, nq, nwant, sp, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0,
                                     exclude=0, want_first=0, want_values=0, strict=False, out_stats=0, upto=0, stream=0):
        """zero-copy form (phnsw_search_batch_labelset_device): search_batch_labeled_device with want_first = u32 offsets
        [nq + 1] and want_values = u32 labels [nwant] (device pointers, alive until the work on `stream` is done) in place
        of want.  status 8 = a range of want_first that is not inside [0, nwant] or runs backwards: that query does not
        walk (empty row, stats 0); overlapping ranges are not detected here.  Enqueued on `stream`; never synchronises
        it"""
        if not isinstance(labels, Labels):
            raise TypeError("search_batch_labelset_device: labels must be a Labels made for this index")
        check(lib().phnsw_search_batch_labelset_device(
            self._h, labels._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp), upto,
            C.c_void_p(exclude or None), C.c_void_p(want_first or None), C.c_void_p(want_values or None), int(nwant),
            FILTER_STRICT if strict else 0, C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len),
            C.c_void_p(out_stats or None), C.c_void_p(status), C.c_void_p(stream or None)))

    def search_labelset(self, queries=None, qids=None, sp=None, labels=None, want=None, exclude=None, k=10, scan_below=0,
                        route=False):
        """search_labeled for a SET of labels per query (phnsw_search_labelset_auto): per query the scan by set
        (search_exact_labelset) where the union of the lists is short (count <= scan_below, or count *
        number_of_candidates < k * vector_count, count as Labels.count_sets gives it), the strict graph walk by set
        otherwise, and the scan again for every query whose walk came back short.  Every row holds exactly min(k, count - e)
        entries and only listed vectors of the labels of want[i] (e = 1 iff exclude[i] is one of them): the rows of
        search_filtered with the equivalent per-query bitmaps, bit for bit.  scan_below 0 = the library's threshold for
        sets, 20 000 rows of the union: measured at sets of 4 labels on 1M x 768 f32 rows, ef 256, k = 10 (scan 17.6 ms
        against the walk's 22.0 at 20 000, 34.2 against 20.3 at 40 000; profiles/labelset_walk/README.md), other shapes
        unmeasured; 2**64 - 1 = always scan.
        1 <= k <= sp.number_of_candidates.
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq]) and, with route=True, route[nq] u32: ROUTE_GRAPH, ROUTE_SCAN or
        ROUTE_GRAPH_THEN_SCAN"""
        q, qi, nq, first, values = self._labelset_args("search_labelset", queries, qids, labels, want)
        sp = sp or SearchParameters()
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        rt = np.zeros(nq, dtype=np.uint32) if route else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_labelset_auto(self._h, labels._h, _p(q), _p(qi), nq, C.byref(sp), _p(ex), _p(first),
                                               _p(values) if len(values) else None, int(k), int(scan_below), _p(ids), _p(d),
                                               _p(ln), _p(rt)))
        return (ids, d, ln, rt) if route else (ids, d, ln)

    def search_labelset_device(self, labels, nq, nwant, sp, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0,
                               exclude=0, want_first=0, want_values=0, scan_below=0, out_route=0, stream=0):
        """device form (phnsw_search_labelset_auto_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF; want_first = u32 offsets [nq + 1], want_values = u32 labels [nwant]; out_route u32 [nq] or 0.  status
        8 where search_exact_labelset_device reports it (a range fault, an overlap with a lower query): scanned, empty.
        Like search_labeled_device it synchronises `stream`, up to twice"""
        if not isinstance(labels, Labels):
            raise TypeError("search_labelset_device: labels must be a Labels made for this index")
        check(lib().phnsw_search_labelset_auto_device(
            self._h, labels._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp),
            C.c_void_p(exclude or None), C.c_void_p(want_first or None), C.c_void_p(want_values or None), int(nwant), int(k),
            int(scan_below), C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(out_route or None),
            C.c_void_p(status), C.c_void_p(stream or None)))

    def search_collect(self, queries=None, qids=None, sp=None, allow=None, exclude=None, upto=0, stats=False, k=10,
                       extend=False):
        """the collecting search (phnsw_search_collect): search_batch with the same sp, upto and exclude, whose walk of the
        last layer also keeps the best k ALLOWED rows it evaluates (allowed, not excluded, distance <= f32::MAX) and
        returns those -- where search_batch_filtered filters the layer's queue afterwards and comes back with about
        density * number_of_candidates results.  allow as in search_batch_filtered (None = the default of set_filter,
        else every row).  Without extend the traversal and its stats are search_batch's, bit for bit; extend=True lets a
        hop that improved the kept rows count as one that did something, so probe_depth counts the hops that improve
        neither queue; probe_depth idle hops in all (not in a row) still end the walk, so a short row does not mean that fewer than k
        allowed rows are reachable.  The row holds the first k allowed entries of search_batch's row or better ones (not
        of search_batch_filtered's, whose descent differs below the top layer).  1 <= k <= 64; k may exceed
        number_of_candidates.  An approximate result: only rows the walk evaluated.  profiles/collect/README.md.
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq]) and the stats with stats=True"""
        if (queries is None) == (qids is None):
            raise ValueError("search_collect: pass queries or qids (exactly one)")
        sp = sp or SearchParameters()
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            assert q.shape[1] == self.store.dim
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        words, stride = pack_allow(allow, self.store.n, nq)
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        st = np.zeros((nq, 2), dtype=np.uint64) if stats else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_collect(self._h, _p(q), _p(qi), nq, C.byref(sp), upto, _p(ex), _p(words), stride,
                                         COLLECT_EXTEND if extend else 0, int(k), _p(ids), _p(d), _p(ln), _p(st)))
        return (ids, d, ln, st) if stats else (ids, d, ln)

    def search_collect_device(self, nq, sp, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                              allow=0, allow_stride=0, extend=False, out_stats=0, upto=0, stream=0):
        """zero-copy form (phnsw_search_collect_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF; allow as in search_batch_filtered_device.  Enqueued on `stream`; never synchronises it"""
        check(lib().phnsw_search_collect_device(
            self._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp), upto,
            C.c_void_p(exclude or None), C.c_void_p(allow or None), int(allow_stride), COLLECT_EXTEND if extend else 0, int(k),
            C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(out_stats or None), C.c_void_p(status),
            C.c_void_p(stream or None)))

    def search_collect_labeled(self, queries=None, qids=None, sp=None, labels=None, want=None, exclude=None, upto=0,
                               stats=False, k=10, extend=False):
        """search_collect by row label (phnsw_search_collect_labeled): the rows, lengths and stats of
        search_collect(allow=(the vectors listed under want[i])), bit for bit, without a bitmap per query.  labels: a
        Labels made for this index; want: integers [nq] within u32, -1 or LABEL_NONE (or a label nobody carries) = an empty
        row.  set_filter's default is not consulted.
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq]) and the stats with stats=True"""
        q, qi, nq, w32 = self._labeled_args("search_collect_labeled", queries, qids, labels, want)
        sp = sp or SearchParameters()
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        st = np.zeros((nq, 2), dtype=np.uint64) if stats else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_collect_labeled(self._h, labels._h, _p(q), _p(qi), nq, C.byref(sp), upto, _p(ex), _p(w32),
                                                 COLLECT_EXTEND if extend else 0, int(k), _p(ids), _p(d), _p(ln), _p(st)))
        return (ids, d, ln, st) if stats else (ids, d, ln)

    def search_collect_labeled_device(self, labels, nq, sp, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0,
                                      exclude=0, want=0, extend=False, out_stats=0, upto=0, stream=0):
        """zero-copy form (phnsw_search_collect_labeled_device): search_collect_device with want = u32 labels [nq] (a
        device pointer, alive until the work on `stream` is done) in place of the bitmaps.  Enqueued on `stream`; never
        synchronises it"""
        if not isinstance(labels, Labels):
            raise TypeError("search_collect_labeled_device: labels must be a Labels made for this index")
        check(lib().phnsw_search_collect_labeled_device(
            self._h, labels._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp), upto,
            C.c_void_p(exclude or None), C.c_void_p(want or None), COLLECT_EXTEND if extend else 0, int(k),
            C.c_void_p(out_ids), C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(out_stats or None), C.c_void_p(status),
            C.c_void_p(stream or None)))

    def filter_count_device(self, nbitmaps, out_count, allow=0, allow_stride=0, stream=0):
        """phnsw_filter_count_device: the number of candidates of each of nbitmaps device bitmaps into out_count (u32
        [nbitmaps], a device pointer)"""
        check(lib().phnsw_filter_count_device(self._h, C.c_void_p(allow or None), int(allow_stride), int(nbitmaps),
                                              C.c_void_p(out_count), C.c_void_p(stream or None)))

    def filter_count(self, allow=None):
        """how many candidates search_exact_filtered would choose among: allowed ids below n that the index holds (no
        exclude).  allow: a bool mask [n] or [nq, n] or packed words, None = the default of set_filter, else every
        vector of the index.  Host convenience over filter_count_device (needs torch for the device buffers); returns
        an int for one bitmap, a u32 array [nq] for one per query.  What to choose the search call by"""
        import torch
        a = None if allow is None else np.asarray(allow)
        nb = a.shape[0] if a is not None and a.ndim == 2 else 1
        words, stride = pack_allow(a, self.store.n, nb)
        dev = torch.device("cuda", getattr(self.store, "device", 0))
        wd = None if words is None else torch.from_numpy(words.view(np.int32)).to(dev)
        out = torch.zeros(nb, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.filter_count_device(nb, out.data_ptr(), allow=0 if wd is None else wd.data_ptr(), allow_stride=stride)
        torch.cuda.synchronize(dev)
        counts = out.cpu().numpy().view(np.uint32)
        return counts if a is not None and a.ndim == 2 else int(counts[0])

    def search_filtered(self, queries=None, qids=None, sp=None, allow=None, exclude=None, k=10, scan_below=0, route=False):
        """one filtered call that picks its method per query (phnsw_search_filtered_auto): the exact scan where few rows
        are allowed (candidates <= scan_below, or candidates * number_of_candidates < k * vector_count), the graph walk
        with a strict filter otherwise, and the scan again for every query whose walk came back short.  Every row holds
        exactly min(k, candidates) entries and only candidates (as search_exact_filtered defines them; allow and exclude
        as there).  scan_below 0 = the library's threshold (13 000 shared / 10 000 per query, measured on 1M x 768 f32
        rows), 2**64 - 1 = always scan.  A graph-routed row is approximate: the guarantee is completeness, not recall.
        1 <= k <= sp.number_of_candidates.
        Returns (ids[nq, k] u64, d[nq, k] f32, len[nq]) and, with route=True, route[nq] u32: ROUTE_GRAPH, ROUTE_SCAN or
        ROUTE_GRAPH_THEN_SCAN"""
        sp = sp or SearchParameters()
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            assert q.shape[1] == self.store.dim
            nq = q.shape[0]
        if qids is not None:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        if q is None and qi is None:
            raise ValueError("search_filtered: pass queries or qids")
        words, stride = pack_allow(allow, self.store.n, nq)
        w = max(int(k), 0)
        ids = np.empty((nq, w), dtype=np.uint64)
        d = np.empty((nq, w), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        rt = np.zeros(nq, dtype=np.uint32) if route else None
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        check(lib().phnsw_search_filtered_auto(self._h, _p(q), _p(qi), nq, C.byref(sp), _p(ex), _p(words), stride, int(k),
                                               int(scan_below), _p(ids), _p(d), _p(ln), _p(rt)))
        return (ids, d, ln, rt) if route else (ids, d, ln)

    def search_filtered_device(self, nq, sp, k, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                               allow=0, allow_stride=0, scan_below=0, out_route=0, stream=0):
        """device form (phnsw_search_filtered_auto_device): device pointers as integers, u32 ids [nq, k] padded with
        0xFFFFFFFF; allow = one packed bitmap (allow_stride 0) or nq bitmaps allow_stride words apart, 0 = the default
        of set_filter; out_route u32 [nq] or 0.  Unlike the other _device calls it synchronises `stream`, up to twice"""
        check(lib().phnsw_search_filtered_auto_device(
            self._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq, C.byref(sp), C.c_void_p(exclude or None),
            C.c_void_p(allow or None), int(allow_stride), int(k), int(scan_below), C.c_void_p(out_ids), C.c_void_p(out_d),
            C.c_void_p(out_len), C.c_void_p(out_route or None), C.c_void_p(status), C.c_void_p(stream or None)))

    def search_batch_reranked(self, full, queries, sp=None, k=10):
        """an index over an F16Store, I8Store, I8QStore or BitStore: search it, recompute every result's distance on the
        f32 store `full`, sort by (distance, id), keep the best k (phnsw_f16_search_batch / phnsw_i8_search_batch /
        phnsw_i8q_search_batch / phnsw_bits_search_batch)
        -> ids[nq, k] u64, d[nq, k] f32, len[nq]"""
        sp = sp or SearchParameters()
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        assert q.shape[1] == self.store.dim
        nq, k = q.shape[0], int(k)
        ids = np.empty((nq, k), dtype=np.uint64)
        d = np.empty((nq, k), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        fn = getattr(lib(), "phnsw_%s_search_batch" % _reranked_kind(self.store))
        check(fn(self._h, full._h, _p(q), nq, C.byref(sp), k, _p(ids), _p(d), _p(ln)))
        return ids, d, ln

    def search_batch_reranked_device(self, full, nq, sp, k, queries, ldq, out_ids, out_d, out_len, status, out_stats=0,
                                     stream=0):
        """zero-copy form of search_batch_reranked (device pointers as ints, u32 ids, rows of number_of_candidates)"""
        fn = getattr(lib(), "phnsw_%s_search_batch_device" % _reranked_kind(self.store))
        check(fn(self._h, full._h, C.c_void_p(queries), ldq, nq, C.byref(sp), int(k), C.c_void_p(out_ids),
                 C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(out_stats or None), C.c_void_p(status),
                 C.c_void_p(stream or None)))

    def search_instrumented_batch(self, queries=None, qids=None, sp=None):
        """Hnsw::search_instrumented (lib.rs:667-673) for many queries -> ids, d, len, index_distance[nq] u64"""
        sp = sp or SearchParameters()
        ef = sp.number_of_candidates
        q = qi = None
        if queries is not None:
            q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
            assert q.shape[1] == self.store.dim
            nq = q.shape[0]
        else:
            qi = np.ascontiguousarray(qids, dtype=np.uint64)
            nq = len(qi)
        ids = np.empty((nq, ef), dtype=np.uint64)
        d = np.empty((nq, ef), dtype=np.float32)
        ln = np.zeros(nq, dtype=np.uint64)
        idx = np.zeros(nq, dtype=np.uint64)
        check(lib().phnsw_search_instrumented(self._h, _p(q), _p(qi), nq, C.byref(sp), _p(ids), _p(d), _p(ln), _p(idx)))
        return ids, d, ln, idx

    def search_instrumented(self, v, sp=None):
        """Hnsw::search_instrumented(v, sp) -> (Vec<(VectorId, f32)>, usize)  lib.rs:667-673"""
        if isinstance(v, Stored):
            ids, d, ln, idx = self.search_instrumented_batch(qids=[v.id], sp=sp)
        else:
            ids, d, ln, idx = self.search_instrumented_batch(queries=v.vec if isinstance(v, Unstored) else v, sp=sp)
        return [(int(ids[0, i]), d[0, i]) for i in range(int(ln[0]))], int(idx[0])

    def search_batch_device(self, nq, sp, out_ids, out_d, out_len, status, queries=0, ldq=0, qids=0, exclude=0,
                            out_stats=0, upto=0, stream=0):
        """zero-copy launch: every argument is a device pointer (int); u32 ids; returns after
        enqueueing on `stream` (a hipStream_t value, 0 = default stream)"""
        check(lib().phnsw_search_batch_device(self._h, C.c_void_p(queries or None), ldq, C.c_void_p(qids or None), nq,
                                              C.byref(sp), upto, C.c_void_p(exclude or None), C.c_void_p(out_ids),
                                              C.c_void_p(out_d), C.c_void_p(out_len), C.c_void_p(out_stats or None),
                                              C.c_void_p(status), C.c_void_p(stream or None)))

    def search(self, v, sp=None):
        """Hnsw::search(v, sp) -> Vec<(VectorId, f32)>  lib.rs:663-665"""
        if isinstance(v, Stored):
            ids, d, ln = self.search_batch(qids=[v.id], sp=sp)
        else:
            ids, d, ln = self.search_batch(queries=v.vec if isinstance(v, Unstored) else v, sp=sp)
        return [(int(ids[0, i]), d[0, i]) for i in range(int(ln[0]))]

    def search_upto(self, v, sp, upto_layer_from_top):
        """lib.rs:654-661"""
        if isinstance(v, Stored):
            ids, d, ln = self.search_batch(qids=[v.id], sp=sp, upto=upto_layer_from_top)
        else:
            ids, d, ln = self.search_batch(queries=v.vec, sp=sp, upto=upto_layer_from_top)
        return [(int(ids[0, i]), d[0, i]) for i in range(int(ln[0]))]

    def knn(self, k, probe_depth):
        """Hnsw::knn  lib.rs:905-928 -> [(VectorId, [(VectorId, f32)])]"""
        n = self.vector_count()
        ids = np.empty((n, k), dtype=np.uint64)
        d = np.empty((n, k), dtype=np.float32)
        ln = np.zeros(n, dtype=np.uint64)
        check(lib().phnsw_knn(self._h, k, probe_depth, _p(ids), _p(d), _p(ln)))
        nodes = self._layer(self.layer_count() - 1).nodes
        return [(int(nodes[i]), [(int(ids[i, j]), d[i, j]) for j in range(int(ln[i]))]) for i in range(n)]

    def threshold_nn(self, threshold, probe_depth, initial_search_depth, max_out=64):
        """Hnsw::threshold_nn  lib.rs:930-962 -> [(VectorId, [(VectorId, f32)])]"""
        n = self.vector_count()
        ids = np.empty((n, max_out), dtype=np.uint64)
        d = np.empty((n, max_out), dtype=np.float32)
        ln = np.zeros(n, dtype=np.uint64)
        check(lib().phnsw_threshold_nn(self._h, threshold, probe_depth, initial_search_depth, max_out, _p(ids), _p(d),
                                       _p(ln)))
        nodes = self._layer(self.layer_count() - 1).nodes
        return [(int(nodes[i]), [(int(ids[i, j]), d[i, j]) for j in range(int(ln[i]))]) for i in range(n)]

    # -- Serializable (lib.rs:1688-1699, serialize.rs) -------------------------------
    def serialize(self, path):
        check(lib().phnsw_index_serialize(self._h, str(path).encode()))

    @classmethod
    def deserialize(cls, path, store):
        """Hnsw::deserialize(path, params): `store` plays the role of the comparator params"""
        h = C.c_void_p()
        check(lib().phnsw_index_deserialize(store._h, str(path).encode(), C.byref(h)))
        bp = BuildParams()
        check(lib().phnsw_index_build_params(h, C.byref(bp)))
        return cls(store, h, bp)

    def counters(self):
        """(distance evaluations, hops) of every search launched on this index, build rounds included"""
        a, b = C.c_uint64(), C.c_uint64()
        check(lib().phnsw_index_counters(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def kernel_ms(self):
        ms = C.c_float()
        check(lib().phnsw_last_search_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def dispatches(self):
        """the last descent dispatch by dispatch: [{"layers": (lo, hi), "ms", "n_dist", "n_hops", "n_table"}];
        entry 0 is the dense-top-layer tile pass (layers (0, 0)); n_table of n_dist evaluations were table look-ups"""
        cap = 32
        cnt = C.c_uint32()
        ms = np.zeros(cap, dtype=np.float32)
        nd, nh = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
        lo, hi = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        check(lib().phnsw_last_search_dispatches(self._h, cap, C.byref(cnt), _p(ms), _p(nd), _p(nh), _p(lo), _p(hi)))
        nt = np.zeros(cap, dtype=np.uint64)
        c2 = C.c_uint32()
        check(lib().phnsw_last_search_table_evals(self._h, cap, C.byref(c2), _p(nt)))
        return [{"layers": (int(lo[i]), int(hi[i])), "ms": float(ms[i]), "n_dist": int(nd[i]), "n_hops": int(nh[i]),
                 "n_table": int(nt[i])} for i in range(min(cap, cnt.value))]

    def dense_top_layers(self, number_of_candidates):
        """(layers walked through the dense distance table, nodes of the largest, built on the matrix cores?)"""
        t, n, m = C.c_uint32(), C.c_uint64(), C.c_uint32()
        check(lib().phnsw_dense_top_layers(self._h, int(number_of_candidates), C.byref(t), C.byref(n), C.byref(m)))
        return int(t.value), int(n.value), bool(m.value)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().phnsw_index_destroy(h)
            except Exception:  # interpreter shutdown
                pass
