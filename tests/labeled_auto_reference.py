"""phnsw_search_labeled_auto restated in numpy FROM THE LABEL COLUMN: list lengths by counting labels, "exclude[q] is a
candidate" by looking at its label -- no bitmap anywhere.  tests/test_labeled_auto_cpu.py holds it against
filter_auto_reference.compose over labeled_reference.masks_of.  As there, the strict graph rows and the exact rows come
from the caller."""
import numpy as np

import exact_filter_reference as xr
import filter_auto_reference as ar
from labeled_reference import LABEL_NONE

SCAN_BELOW_LABELED = 20000  # filter_route.h: the measured crossover (profiles/labeled_walk/README.md)


def listed_column(labels, members=None):
    """the handle's column: the label of every listed vector, LABEL_NONE elsewhere"""
    lab = np.asarray(labels).astype(np.int64).copy()
    lab[lab == -1] = LABEL_NONE
    if members is not None:
        lab[~np.asarray(members, dtype=bool)] = LABEL_NONE
    return lab


def counts_of(labels, want, members=None):
    """what phnsw_labels_count_device writes: the length of the list of want[q]"""
    lab = listed_column(labels, members)
    w = np.asarray(want).astype(np.int64).copy()
    w[w == -1] = LABEL_NONE
    return np.array([0 if x == LABEL_NONE else int(np.count_nonzero(lab == x)) for x in w], dtype=np.uint32)


def compose(walk, scan, labels, want, ef, k, n_nodes, exclude=None, members=None, scan_below=0):
    """walk: the strict rows of the label walk for every query, scan: the posting-list scan's rows -> ids[nq, k], d, len,
    route as phnsw.h composes them"""
    lab = listed_column(labels, members)
    w = np.asarray(want).astype(np.int64).copy()
    w[w == -1] = LABEL_NONE
    counts = counts_of(labels, want, members)
    nq, below = len(w), int(scan_below) if scan_below else SCAN_BELOW_LABELED
    ids = np.full((nq, k), xr.EMPTY, dtype=np.uint64)
    d = np.full((nq, k), xr.FMAX, dtype=np.float32)
    ln = np.zeros(nq, dtype=np.uint64)
    route = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        c = int(counts[q])
        ex = None if exclude is None else int(exclude[q])
        e = 1 if ex is not None and ex < len(lab) and w[q] != LABEL_NONE and lab[ex] == w[q] else 0
        r = ar.rule(c, below, ef, k, n_nodes)
        if r == ar.GRAPH:
            m = int(walk[2][q])
            keep = np.ones(m, dtype=bool) if ex is None else walk[0][q, :m] != np.uint64(ex)
            wi, wd = walk[0][q, :m][keep][:k], walk[1][q, :m][keep][:k]
            if len(wi) < min(k, c - e):
                r = ar.GRAPH_THEN_SCAN
            else:
                ids[q, :len(wi)], d[q, :len(wi)], ln[q] = wi, wd, len(wi)
        if r != ar.GRAPH:
            ids[q], d[q], ln[q] = scan[0][q], scan[1][q], scan[2][q]
        route[q] = r
    return ids, d, ln, route
