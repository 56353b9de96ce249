"""Pure-Python pieces of tests/test_gpu_ranged_scale.py, test_gpu_label_ranged_scale.py and
test_gpu_labelset_ranged_scale.py: what is particular to SPANS in range_plan.h, label_range_plan.h and
labelset_range_plan.h, restated (the span order of a column, the span of a range or of a (label, range) pair, the batch
order by span start, the rows a block reads in its second turn, the kept pairs of a set-range batch), so that a test can
assert the shape that makes a loop turn, and the makers of the key columns.  The rules of batches, slices and work items
are label_plan.h's, which ph_list_scan uses unchanged: they are tests/labeled_scale_reference.py's, imported, not copied.
Nothing here computes a distance.  Pinned by tests/test_ranged_scale_cpu.py on cases worked by hand from the headers."""
import numpy as np

from labeled_scale_reference import (BATCH, GRID_MAX, batches, both_turns, items, past_clamp, slice_count,  # noqa: F401
                                     slice_ranges)

NONE = 0xFFFFFFFF            # PHNSW_ATTR_NONE, PHNSW_LABEL_NONE, PH_RANGE_SORT_EMPTY
PAIR_NONE = 2 ** 64 - 1      # PH_LABEL_RANGE_PAIR_NONE
TOP = 0xFFFFFFFE             # the largest key and the largest label there is
STEP = 61356                 # key(r) = r * STEP + 7: spread over all four bytes, below 2^32 - 1 for r < 70 001


def u32(a):
    """labels or keys as i64 within u32 (-1 = NONE)"""
    a = np.asarray(a).astype(np.int64).copy()
    a[a == -1] = NONE
    assert ((a >= 0) & (a <= NONE)).all()
    return a


# ---------------------------------------------------------------- the rules
def span_order(keys, members=None):
    """the ids of the listed rows as the range handle keeps them, by (key, id), and their keys -> (ids i64, skeys i64)"""
    keys = u32(keys)
    listed = keys != NONE
    if members is not None:
        listed &= np.asarray(members, dtype=bool)
    ids = np.nonzero(listed)[0]
    ids = ids[np.argsort(keys[ids], kind="stable")]
    return ids, keys[ids]


def composites(labels, keys, members=None):
    """(label << 32) | key of every row as Python-sized unsigned integers (u64), PAIR_NONE where the row is not listed"""
    labels, keys = u32(labels), u32(keys)
    listed = (labels != NONE) & (keys != NONE)
    if members is not None:
        listed &= np.asarray(members, dtype=bool)
    pair = (labels.astype(np.uint64) << np.uint64(32)) | keys.astype(np.uint64)
    pair[~listed] = np.uint64(PAIR_NONE)
    return pair


def pair_order(labels, keys, members=None):
    """the ids of the listed rows as the label-range handle keeps them, by (composite, id) -> (ids i64, spairs u64)"""
    pair = composites(labels, keys, members)
    ids = np.nonzero(pair != np.uint64(PAIR_NONE))[0]
    ids = ids[np.argsort(pair[ids], kind="stable")]
    return ids, pair[ids]


def spans_of(skeys, lo, hi):
    """ph_range_span for every (lo, hi): [lower_bound(lo), upper_bound(hi)) -> (at, len) i64; an empty range has (0, 0)"""
    skeys = np.asarray(skeys)
    lo, hi = np.asarray(lo).astype(skeys.dtype), np.asarray(hi).astype(skeys.dtype)
    b = np.searchsorted(skeys, lo, side="left").astype(np.int64)
    e = np.searchsorted(skeys, hi, side="right").astype(np.int64)
    live = (lo <= hi) & (e > b)
    return np.where(live, b, 0), np.where(live, e - b, 0)


def pair_spans_of(spairs, want, lo, hi):
    """ph_label_range_span for every (want, lo, hi) -> (at, len) i64; want NONE (or -1), lo > hi, nobody with the label,
    no key inside: (0, 0)"""
    want, lo, hi = u32(want), u32(lo), u32(hi)
    w = want.astype(np.uint64) << np.uint64(32)
    at, ln = spans_of(np.asarray(spairs, dtype=np.uint64), w | lo.astype(np.uint64), w | hi.astype(np.uint64))
    live = (want != NONE) & (lo <= hi)
    return np.where(live, at, 0), np.where(live, ln, 0)


def batch_order(at, ln):
    """the per-call sort: stable, by ph_range_sort_key (the span's start, the empty spans last) -> sorted[] i64: the
    lookup position at every position of the sorted batch"""
    key = np.where(np.asarray(ln) > 0, np.asarray(at), NONE).astype(np.int64)
    return np.argsort(key, kind="stable")


def second_turn_rows(order, at, ln, slices):
    """per LOOKUP position p the (first, end) ranks of its span that only second-turn items read: work item = slice * nq
    + position of the sorted batch; the items at or past GRID_MAX are those a block takes in its second turn, and slice s
    of a span reads its batches slice_ranges(len, slices)[s].  (0, 0) where no item of p is past the clamp or the span
    has no batch there.  The slices of a position past the clamp are a suffix, so its second-turn rows are one range"""
    nq = len(order)
    past = past_clamp(nq, slices)
    out = np.zeros((nq, 2), dtype=np.int64)
    for pos in range(nq):
        late = np.nonzero(past[:, pos])[0]
        if not len(late):
            continue
        p = int(order[pos])
        assert late[-1] == slices - 1 and len(late) == slices - late[0]
        r = slice_ranges(int(ln[p]), slices)
        out[p] = min(r[late[0]][0] * BATCH, int(ln[p])), int(ln[p])
        if out[p, 0] >= out[p, 1]:
            out[p] = 0
    return out


def carrying_blocks(live, slices):
    """both_turns for live positions that are no prefix: live bool [nq] by position of the sorted batch (a position
    whose span is not empty and, in the PAIRS form, no duplicate) -> the blocks whose first AND second item scan rows"""
    live = np.asarray(live, dtype=bool)
    nq, total = len(live), items(len(live), slices)
    if total <= GRID_MAX:
        return np.zeros(0, dtype=np.int64)
    b = np.arange(min(GRID_MAX, total - GRID_MAX), dtype=np.int64)
    return b[live[b % nq] & live[(b + GRID_MAX) % nq]]


def pairs_of(first):
    """the owning query of every pair of a sound CSR batch"""
    first = np.asarray(first, dtype=np.int64)
    return np.repeat(np.arange(len(first) - 1), np.diff(first))


def kept_pairs(first, values, at, ln):
    """the set-range batch as labelset_range_plan.h cuts it: the pairs are sorted, stably, by span start; a position
    duplicates its predecessor iff both belong to one query and have the same non-empty span; a pair is KEPT iff it is
    no duplicate and its span is not empty -> (kept bool [nwant], order i64 [nwant])"""
    owner = pairs_of(first)
    at, ln = np.asarray(at, dtype=np.int64), np.asarray(ln, dtype=np.int64)
    order = batch_order(at, ln)
    dup = np.zeros(len(owner), dtype=bool)
    for pos in range(1, len(order)):
        i, j = order[pos], order[pos - 1]
        dup[i] = ln[i] != 0 and owner[i] == owner[j] and at[i] == at[j] and ln[i] == ln[j]
    return ~dup & (ln > 0), order


def distinct_pairs(first, values, ln):
    """brute force: per query the first pair of every distinct label whose span is not empty, bool [nwant]"""
    first, values = np.asarray(first, dtype=np.int64), u32(values)
    keep = np.zeros(len(values), dtype=bool)
    for q in range(len(first) - 1):
        seen = set()
        for i in range(first[q], first[q + 1]):
            if ln[i] and int(values[i]) not in seen:
                keep[i] = True
            seen.add(int(values[i]))
    return keep


def csr(sets):
    """(first i64 [nq + 1], values i64 [nwant]) of a list of label sets"""
    first = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sets], out=first[1:])
    values = u32(np.concatenate([np.asarray(s, dtype=np.int64) for s in sets])) if first[-1] else np.zeros(0, dtype=np.int64)
    return first, values


# ---------------------------------------------------------------- the columns
def key_of_rank(r, listed):
    """the key of rank r of a column of `listed` distinct keys: ascending in r, rank 0 has key 0, the top rank TOP"""
    r = np.asarray(r, dtype=np.int64)
    assert (r >= 0).all() and (r < listed).all() and (listed - 1) * STEP + 7 < TOP
    k = r * STEP + 7
    return np.where(r == 0, 0, np.where(r == listed - 1, TOP, k))


def span(r, c, listed):
    """(lo, hi) that hold exactly the c rows from rank r of a ranked column; c == 0: a range inside the gap behind r"""
    if c == 0:
        g = int(key_of_rank(r, listed))
        return g + 1, g + 5
    return int(key_of_rank(r, listed)), int(key_of_rank(r + c - 1, listed))


def ranked_column(n, seed, fixed=None, missing=()):
    """u32 keys [n] as i64: the rows but `missing` take the ranks 0 .. listed - 1 in a random order -- `fixed` {id: rank}
    first --, key = key_of_rank(rank); `missing` carry NONE -> (keys, rank_of i64 [n], -1 where missing)"""
    fixed = dict(fixed or {})
    missing = np.asarray(missing, dtype=np.int64)
    listed = n - len(missing)
    assert len(set(fixed.values())) == len(fixed) and not np.isin(list(fixed), missing).any()
    ids = np.setdiff1d(np.arange(n), np.concatenate([missing, np.array(list(fixed), dtype=np.int64)]))
    ranks = np.setdiff1d(np.arange(listed), np.array(list(fixed.values()), dtype=np.int64))
    rank_of = np.full(n, -1, dtype=np.int64)
    rank_of[np.random.default_rng(seed).permutation(ids)] = ranks
    for v, r in fixed.items():
        rank_of[v] = r
    keys = np.full(n, NONE, dtype=np.int64)
    at = rank_of >= 0
    keys[at] = key_of_rank(rank_of[at], listed)
    assert sorted(rank_of[at].tolist()) == list(range(listed))
    return keys, rank_of


def plateau_column(n, seed, on, first, count, missing=()):
    """a ranked column whose ranks first .. first + count - 1 carry ONE key, key_of_rank(first): the rows `on` among
    them -> (keys, the plateau's key)"""
    listed = n - len(missing)
    assert len(on) <= count and 0 < first and first + count < listed - 1
    slots = np.linspace(first, first + count - 1, len(on)).astype(np.int64)
    keys, rank_of = ranked_column(n, seed, dict(zip(np.asarray(on).tolist(), slots.tolist())), missing)
    flat = (rank_of >= first) & (rank_of < first + count)
    keys[flat] = int(key_of_rank(first, listed))
    return keys, int(key_of_rank(first, listed))


def within_label_keys(labels, seed, base=1000, step=10):
    """u32 keys [n] as i64: the rows of every label take the ranks 0 .. (rows of the label) - 1 in a random order, key =
    base + step * rank; rows without a label carry a key all the same (they are not listed).  A range of ranks [a, b)
    then holds exactly min(b, rows) - a rows of every label that has more than a rows"""
    labels = u32(labels)
    perm = np.random.default_rng(seed).permutation(len(labels))
    o = perm[np.argsort(labels[perm], kind="stable")]
    sl = labels[o]
    start = np.searchsorted(sl, sl, side="left")
    keys = np.empty(len(labels), dtype=np.int64)
    keys[o] = base + step * (np.arange(len(labels)) - start)
    return keys


def ranks(a, b, base=1000, step=10):
    """(lo, hi) that hold the ranks [a, b) of within_label_keys; a == b: an empty range in the gap behind rank a"""
    return (base + step * a + 3, base + step * a + 7) if a == b else (base + step * a, base + step * (b - 1))
