"""The bitmaps a batch of label SETS stands for: query q of phnsw_search_exact_labelset may return the vectors whose
label is any of values[first[q]:first[q + 1]].  Built from labeled_reference.masks_of's rule per wanted label and OR-ed;
used with exact_filter_reference.exact_topk, which applies `members` (the index's vectors) and the exclude."""
import numpy as np

import labeled_reference as lr


def masks_of_sets(labels, first, values):
    """bool [nq, N]: row q = {v : labels[v] in S_q}; LABEL_NONE (or -1) lists nothing and wants nothing, a label twice
    counts once, an empty set gives an empty row"""
    first = np.asarray(first).astype(np.int64)
    values = np.asarray(values).astype(np.int64)
    nq = len(first) - 1
    m = np.zeros((nq, len(labels)), dtype=bool)
    if len(values):
        per = lr.masks_of(labels, values)  # one row per wanted label
        for q in range(nq):
            if first[q + 1] > first[q]:
                m[q] = per[first[q]:first[q + 1]].any(0)
    return m


def csr(sets):
    """a list of label lists -> (first i64 [nq + 1], values i64 [nwant])"""
    first = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sets], out=first[1:])
    values = np.array([v for s in sets for v in s], dtype=np.int64)
    return first, values
