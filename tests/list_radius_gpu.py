"""What tests/test_gpu_radius_labeled.py and tests/test_gpu_radius_ranged.py share: the world of
tests/test_gpu_radius_exact.py (N = 5000 rows, 40 copies of row 0, 65 raw and 65 stored queries, one-layer ring indexes),
a `By` object per handle kind that says how a call is made and which rows a query may return, and the check against the
three yardsticks.  Every comparison is on offsets, ids and distance bits, no tolerance anywhere."""
import ctypes as C

import numpy as np

import parallel_hnsw_amd as ph

import list_radius_reference as lrr
import radius_reference as rr
from test_gpu_exact_filter import DUPS, EMPTY, N
from test_gpu_exact_shared import NQX
from test_gpu_i8 import bits
from test_gpu_radius_exact import same

MS = (0, 1, 63, 64, 65, 1000)
UP = np.float32(np.inf)
STAGE = 256  # PH_LIST_RADIUS_STAGE: keys a wave stages before it flushes


class By:
    """how the calls of one handle kind are made.  `filt`: a tuple of [nq] arrays -- (want,) or (lo, hi)"""
    name = slices_knob = None

    def masks(self, filt, members=None):
        raise NotImplementedError

    def kw(self, h, filt):
        raise NotImplementedError

    def take(self, filt, idx):
        return tuple(np.asarray(f)[idx] for f in filt)

    def distinct(self, filt):
        """{value: the queries that have it}"""
        out = {}
        for q, key in enumerate(zip(*[np.asarray(f).tolist() for f in filt])):
            out.setdefault(key, []).append(q)
        return out

    def search(self, hix, h, filt, **kw):
        return getattr(hix, "search_exact_radius_" + self.name)(**self.kw(h, filt), **kw)

    def count(self, hix, h, filt, **kw):
        return getattr(hix, "count_exact_radius_" + self.name)(**self.kw(h, filt), **kw)

    def topk(self, hix, h, filt, k, **kw):
        return getattr(hix, "search_exact_" + self.name)(k=k, **self.kw(h, filt), **kw)

    def u32(self, h, filt):
        """the u32 arrays the C calls take"""
        raise NotImplementedError

    def raw(self, hix, h, filt, radius, cap, queries=None, qids=None, exclude=None, null_arrays=False):
        """the host C call as it stands -> first, total, ids[cap], d[cap]; the arrays are prefilled"""
        nq = len(queries) if queries is not None else len(qids)
        q = None if queries is None else np.ascontiguousarray(queries, dtype=np.float32)
        qi = None if qids is None else np.ascontiguousarray(qids, dtype=np.uint64)
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
        r = rr.radii(radius, nq)
        first = np.full(nq + 1, 77, dtype=np.uint64)
        ids = np.full(max(min(cap, 1 << 22), 1), 7, dtype=np.uint64)
        d = np.full(len(ids), -1.0, dtype=np.float32)
        total = C.c_uint64(99)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        fn = getattr(ph.lib(), "phnsw_search_exact_radius_" + self.name)
        f32 = self.u32(h, filt)
        ph.hnsw.check(fn(hix._h, h._h, p(q), p(qi), nq, p(ex), *[p(f) for f in f32], p(r), cap, p(first),
                         None if null_arrays else p(ids), None if null_arrays else p(d), C.byref(total)))
        return first, int(total.value), ids, d

    def device(self, hix, h, filt, radius, cap, queries=None, qids=None, exclude=None, null_arrays=False, stream=None, sync=True):
        """the device form with torch buffers -> (first, ids u64, d) cut at the total, status, total, and the whole
        prefilled ids / d buffers; sync=False: a function that fetches them"""
        import torch
        dev = torch.device("cuda", 0)
        keep = []

        def up(a, dt):
            a = np.array(a, order="C")  # a copy: the columns and the worlds' arrays are read-only
            t = torch.from_numpy(a.view(dt) if dt is not None else a).to(dev)
            keep.append(t)
            return t

        nq = len(queries) if queries is not None else len(qids)
        qd = qi = ex = ld = 0
        if queries is not None:
            ld = hix.store.ld
            qp = np.zeros((nq, ld), dtype=np.float32)
            qp[:, :queries.shape[1]] = queries
            qd = up(qp, None).data_ptr()
        else:
            qi = up(np.asarray(qids, dtype=np.uint32), np.int32).data_ptr()
        if exclude is not None:
            e = np.asarray(exclude, dtype=np.uint64).copy()
            e[e > 0xFFFFFFFF] = 0xFFFFFFFF
            ex = up(e.astype(np.uint32), np.int32).data_ptr()
        fd = [up(f, np.int32).data_ptr() for f in self.u32(h, filt)]
        rd = up(rr.radii(radius, nq), None)
        G = 64  # guard words behind every output
        first = torch.full((nq + 1 + G,), 77, dtype=torch.int64, device=dev)
        ids = torch.full((max(cap, 1) + G,), 7, dtype=torch.int32, device=dev)
        d = torch.full((max(cap, 1) + G,), -1.0, dtype=torch.float32, device=dev)
        status = torch.full((nq + G,), -1, dtype=torch.int32, device=dev)
        total = torch.full((1 + G,), 99, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        names = ("want",) if len(fd) == 1 else ("lo", "hi")
        getattr(hix, "search_exact_radius_%s_device" % self.name)(
            h, nq, rd.data_ptr(), cap, first.data_ptr(), 0 if null_arrays else ids.data_ptr(), 0 if null_arrays else d.data_ptr(),
            status.data_ptr(), total.data_ptr(), queries=qd, ldq=ld, qids=qi, exclude=ex,
            stream=0 if stream is None else stream.cuda_stream, **dict(zip(names, fd)))

        def fetch():
            torch.cuda.synchronize()
            assert (first[nq + 1:] == 77).all() and (ids[max(cap, 1):] == 7).all() and (d[max(cap, 1):] == -1.0).all()
            assert (status[nq:] == -1).all() and (total[1:] == 99).all()
            t = int(total.cpu().numpy()[0])
            i_all = ids[:max(cap, 1)].cpu().numpy().view(np.uint32).astype(np.uint64)
            d_all = d[:max(cap, 1)].cpu().numpy()
            n = t if t <= cap else 0
            del keep[:]
            return (first[:nq + 1].cpu().numpy().view(np.uint64), i_all[:n], d_all[:n]), status[:nq].cpu().numpy(), t, i_all, d_all
        return fetch() if sync else fetch


class ByLabel(By):
    name, slices_knob = "labeled", "PHNSW_LABEL_SLICES"

    def __init__(self, column):
        self.column = column

    def masks(self, filt, members=None):
        return lrr.label_masks(self.column, filt[0], members)

    def kw(self, h, filt):
        return dict(labels=h, want=filt[0])

    def u32(self, h, filt):
        return (ph.hnsw.pack_labels(filt[0], len(filt[0]), "want"),)


class ByRange(By):
    name, slices_knob = "ranged", "PHNSW_RANGE_SLICES"

    def __init__(self, keys):
        self.keys = keys

    def masks(self, filt, members=None):
        return lrr.range_masks(self.keys, filt[0], filt[1], members)

    def kw(self, h, filt):
        """the Python methods take no 0xFFFFFFFF as a value of a u32 column (an open end is None there): the largest value
        they take selects the same rows, no key being that large; the C calls (raw, device) get the words as they are"""
        top = lambda a: np.minimum(np.asarray(a, dtype=np.uint32), np.uint32(0xFFFFFFFE))
        assert self.keys[self.keys != 0xFFFFFFFF].max() < 0xFFFFFFFE
        return dict(attr=h, lo=top(filt[0]), hi=top(filt[1]))

    def u32(self, h, filt):
        return (np.ascontiguousarray(filt[0], dtype=np.uint32), np.ascontiguousarray(filt[1], dtype=np.uint32))


def forms(w, nq):
    return ((dict(queries=w["q"][:nq]), w["Dq"][:nq]), (dict(qids=w["qids"][:nq]), w["Ds"][:nq]))


def radii_at(D, masks, m):
    """f32 [nq]: the m[q]-th smallest finite distance among the rows query q may return, m[q] clipped to their number;
    a query with none takes it from all rows"""
    nq = D.shape[0]
    m = np.broadcast_to(np.asarray(m, dtype=np.int64), (nq,))
    out = np.zeros(nq, dtype=np.float32)
    for q in range(nq):
        row = D[q, masks[q]] if masks[q].any() else D[q]
        row = np.sort(row[np.isfinite(row)], kind="stable")
        out[q] = row[min(int(m[q]), len(row) - 1)]
    return out


def check(by, w, h, filt, radius, nq=NQX, exclude=None, members=None, hix=None, device=True, bitmap=True, topk=True, which=(0, 1),
          cap=None):
    """raw (0) and stored (1) queries, host form, count-only form and device form, against the three yardsticks:
    (1) the numpy restatement over the oracle's distances, (2) search_exact_radius once per distinct label or window with
    the equivalent bitmap, segment by segment (bitmap=False on a store that call refuses), (3) the top-k call at k = 1024
    cut at the radius.  radius(D, masks) -> [nq], or a value.  Returns the host results by form."""
    hix = hix or w["hix"]
    filt = by.take(filt, np.arange(nq))
    masks = by.masks(filt, members)
    out = {}
    for form in which:
        kw, D = forms(w, nq)[form]
        e = None if exclude is None else np.asarray(exclude[:nq], dtype=np.uint64)
        r = rr.radii(radius(D, masks) if callable(radius) else radius, nq)
        ref = lrr.by_masks(D, r, masks, e)                                       # yardstick 1
        got = by.search(hix, h, filt, radius=r, exclude=e, cap=cap, **kw)
        same(got, ref)
        np.testing.assert_array_equal(by.count(hix, h, filt, radius=r, exclude=e, **kw), ref[0])
        if bitmap:                                                               # yardstick 2
            for _, qs in by.distinct(filt).items():
                qs = np.array(qs)
                sub = {k: v[qs] for k, v in kw.items()}
                seg = hix.search_exact_radius(radius=r[qs], allow=masks[qs[0]], exclude=None if e is None else e[qs], **sub)
                for j, q in enumerate(qs):
                    a, b = rr.segment(got, q), rr.segment(seg, j)
                    np.testing.assert_array_equal(a[0], b[0])
                    np.testing.assert_array_equal(bits(a[1]), bits(b[1]))
        if topk:                                                                 # yardstick 3
            ti, td, tl = by.topk(hix, h, filt, 1024, exclude=e, **kw)
            for q in range(nq):
                si, sd = rr.segment(got, q)
                with np.errstate(invalid="ignore"):
                    cut = int(((td[q, :int(tl[q])] < r[q]) & (r[q] > 0)).sum())
                assert cut == min(1024, len(si))
                np.testing.assert_array_equal(si[:cut], ti[q, :cut])
                np.testing.assert_array_equal(bits(sd[:cut]), bits(td[q, :cut]))
        if device:
            dv, status, total, _, _ = by.device(hix, h, filt, r, max(len(ref[1]), 1), exclude=e, **kw)
            assert not status.any() and total == len(ref[1])
            same(dv, ref)
        out[form] = got
    return out
