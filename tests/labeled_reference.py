"""The bitmaps a label column stands for: query q of phnsw_search_exact_labeled may return the vectors whose label is
want[q].  Used with exact_filter_reference.exact_topk, which applies `members` (the index's vectors) and the exclude."""
import numpy as np

LABEL_NONE = 0xFFFFFFFF


def masks_of(labels, want):
    """bool [nq, N]: row q = {v : labels[v] == want[q]}; LABEL_NONE (or -1) lists nothing and wants nothing"""
    lab = np.asarray(labels).astype(np.int64)
    w = np.asarray(want).astype(np.int64)
    lab[lab == -1] = LABEL_NONE
    w[w == -1] = LABEL_NONE
    m = lab[None, :] == w[:, None]
    m[w == LABEL_NONE] = False
    m[:, lab == LABEL_NONE] = False
    return m
