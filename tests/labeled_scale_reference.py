"""Pure-Python pieces of tests/test_gpu_labeled_scale.py: label_plan.h's integer rules restated (batches of a list, slice
ranges after the clamp, the tile cut over sorted slots, the work items of the scan and which of them a block meets in its
second turn), so that a test can assert the shape that makes a loop turn, and the makers of the label columns.  Nothing
here computes a distance.  Pinned by tests/test_labeled_scale_cpu.py on cases worked by hand from the header."""
import numpy as np

LABEL_NONE = 0xFFFFFFFF
SLOT_NONE = 0xFFFFFFFF       # PH_LABEL_SLOT_NONE
BATCH = 64                   # PH_LABEL_BATCH: ids of a list read at a time
GRID_MAX = 1 << 20           # filter_labeled.hip: blocks of the scan and of the tile kernel at the most
LDS_BYTES = 160 * 1024       # PH_LABEL_LDS_BYTES
TILE_CAP, TILE_WAVES = 16, 4
KMAX = 1024                  # PH_EXACT_KMAX
MULT = 2654435761            # odd: v -> v * MULT mod 2^32 is a bijection on u32


# ---------------------------------------------------------------- the rules
def batches(length):
    return (int(length) + BATCH - 1) // BATCH


def last_batch_ids(length):
    """ids in the last batch of a list (0 for an empty list)"""
    return int(length) - (batches(length) - 1) * BATCH if length else 0


def slice_count(forced, longest):
    """ph_label_slice_count under PHNSW_LABEL_SLICES=forced (> 0): clamped to the batches of the LONGEST list, never 0"""
    assert forced > 0
    nb = batches(longest)
    return 1 if nb == 0 else max(1, min(int(forced), nb))


def slice_ranges(length, slices):
    """ph_label_slice_range of a list of `length` ids for every slice of a call with `slices` slices (after the clamp,
    which looked at the longest list: a shorter one may have fewer batches than slices, and empty ranges)"""
    nb = batches(length)
    return [(s * nb // slices, (s + 1) * nb // slices) for s in range(int(slices))]


def tile_query_lds(k, ld):
    return ld * 4 + (2 * k * 8 + 64 * 8) + 64 * 4 + 16


def tile_of(k, ld, knob=0):
    """ph_label_tile: queries of one label per wave of the tile kernel; 1 = the per-query scan"""
    cap = knob if knob > 0 else TILE_CAP
    return max(1, min((LDS_BYTES // TILE_WAVES) // tile_query_lds(k, ld), cap, 0xFFFF))


def slots_of(values, want):
    """ph_label_slot for every wanted label: the index in `values` (ascending, distinct) or SLOT_NONE"""
    values = np.asarray(values, dtype=np.int64)
    w = np.asarray(want).astype(np.int64)
    w[w == -1] = LABEL_NONE
    at = np.searchsorted(values, w, side="left")
    hit = (w != LABEL_NONE) & (at < len(values))
    hit[hit] = values[at[hit]] == w[hit]
    return np.where(hit, at, SLOT_NONE).astype(np.int64)


def sorted_slots(slot):
    """the per-call sort of (slot, query): stable, so the queries of one slot keep their order -> (sslot, order)"""
    order = np.argsort(np.asarray(slot, dtype=np.int64), kind="stable")
    return np.asarray(slot, dtype=np.int64)[order], order


def tiles(sslot, T):
    """the tile cut over sorted slots: [(head position, size)]; every T-th position of a slot's group heads a tile"""
    out, p, nq = [], 0, len(sslot)
    while p < nq:
        c = 1
        while c < T and p + c < nq and sslot[p + c] == sslot[p]:
            c += 1
        out.append((p, c))
        p += c
    return out


def items(nq, slices):
    return int(nq) * int(slices)


def item_of(pos, slc, nq):
    """work item of (position or tile, slice): slice-major"""
    return int(slc) * int(nq) + int(pos)


def past_clamp(nq, slices):
    """bool [slices, nq]: the (slice, position) pairs whose item lies at or past GRID_MAX -- the items a block takes in
    its second turn (a third needs items > 2 * GRID_MAX)"""
    it = np.arange(int(slices), dtype=np.int64)[:, None] * int(nq) + np.arange(int(nq), dtype=np.int64)[None, :]
    return it >= GRID_MAX


def second_turn_first_row(nq, slices, length):
    """the smallest list position any second-turn item of a list of `length` ids reads, and the smallest read in a second
    turn for EVERY position (None, None if no item is past the clamp)"""
    past = past_clamp(nq, slices)
    if not past.any():
        return None, None
    r = slice_ranges(length, slices)
    some = min(s for s in range(slices) if past[s].any())
    every = min(s for s in range(slices) if past[s].all())
    return r[some][0] * BATCH, r[every][0] * BATCH


def both_turns(nq, slices, live):
    """blocks whose first AND second item are live: item % nq < live (live = nq for the scan kernel, the tile count for
    the tile kernel, whose other items are skipped).  Only these carry LDS from one item to the next."""
    total = items(nq, slices)
    if total <= GRID_MAX:
        return np.zeros(0, dtype=np.int64)
    b = np.arange(min(GRID_MAX, total - GRID_MAX), dtype=np.int64)
    return b[(b % nq < live) & ((b + GRID_MAX) % nq < live)]


# ---------------------------------------------------------------- the columns
def own_label(v):
    return (np.asarray(v, dtype=np.uint64) * np.uint64(MULT) % np.uint64(2 ** 32)).astype(np.int64)


def none_rows(n, count, keep_out, below, seed):
    """`count` ids below `below`, none of `keep_out`, drawn once"""
    pool = np.setdiff1d(np.arange(min(n, below)), np.asarray(keep_out, dtype=np.int64))
    return np.sort(np.random.default_rng(seed).permutation(pool)[:count])


def column_one(n, value, none=()):
    lab = np.full(n, value, dtype=np.int64)
    lab[np.asarray(none, dtype=np.int64)] = LABEL_NONE
    return lab


def column_own(n, none=()):
    lab = own_label(np.arange(n))
    assert not (lab == LABEL_NONE).any() and len(np.unique(lab)) == n
    lab[np.asarray(none, dtype=np.int64)] = LABEL_NONE
    return lab


SMALL_SIZES = (1, 2, 63, 64, 65, 128, 129)


def column_mix(n, big_first, big_others, none, seed, rounds=10):
    """-> (column i64 [n], info): BIG on `big_first` and big_others more rows; `rounds` times a label of each of
    SMALL_SIZES rows; the rest in labels of 20 .. 40 rows (the very last one may be shorter); `none` unlabelled.  Label
    values are scrambled over all four bytes; one is 0xFFFFFFFE, two are adjacent (x, x + 1).  info: big, top, adjacent
    (x, x + 1), between (absent, between two present values), below (absent, under the smallest), sizes {value: rows}"""
    rng = np.random.default_rng(seed)
    lab = np.full(n, LABEL_NONE, dtype=np.int64)
    free = rng.permutation(np.setdiff1d(np.arange(n), np.concatenate([np.asarray(big_first), np.asarray(none)])))
    sizes = [big_others] + list(SMALL_SIZES) * rounds
    left = len(free) - sum(sizes)
    assert left > 40
    t = 0
    while left > 0:
        c = min(20 + t % 21, left)
        sizes.append(c)
        left, t = left - c, t + 1
    values = own_label(np.arange(len(sizes)) + 17)  # distinct: the multiplier is odd
    values[1] = 0xFFFFFFFE
    values[3] = values[2] + 1
    assert len(np.unique(values)) == len(values) and values.min() > 0 and values.max() == 0xFFFFFFFE
    at = 0
    for v, c in zip(values, sizes):
        lab[free[at:at + c]] = v
        at += c
    assert at == len(free)
    lab[np.asarray(big_first)] = values[0]
    sv = np.sort(values)
    gap = int(np.nonzero(np.diff(sv) > 1)[0][len(sv) // 2])
    info = dict(big=int(values[0]), top=0xFFFFFFFE, adjacent=(int(values[2]), int(values[3])), between=int(sv[gap]) + 1,
                below=int(sv[0]) - 1, sizes={int(v): int(c) for v, c in zip(values, sizes)})
    info["sizes"][info["big"]] += len(big_first)
    return lab, info


def sized_column(n, sizes, seed, first=1):
    """label first + j on exactly sizes[j] rows drawn at random, the others unlabelled"""
    perm = np.random.default_rng(seed).permutation(n)
    lab = np.full(n, LABEL_NONE, dtype=np.int64)
    at = 0
    for j, c in enumerate(sizes):
        lab[perm[at:at + c]] = first + j
        at += c
    assert at <= n
    return lab


def counts_of(lab, want, members=None):
    """numpy's count of every wanted label among the listed rows"""
    lab = np.asarray(lab).astype(np.int64).copy()
    lab[lab == -1] = LABEL_NONE
    if members is not None:
        lab[~np.asarray(members, dtype=bool)] = LABEL_NONE
    values, counts = np.unique(lab[lab != LABEL_NONE], return_counts=True)
    s = slots_of(values, want)
    return np.where(s == SLOT_NONE, 0, counts[np.minimum(s, len(counts) - 1)]).astype(np.int64)


def info_of(lab, n, members=None):
    """(n, nlabels, listed, longest) as phnsw_labels_info reports them"""
    lab = np.asarray(lab).astype(np.int64).copy()
    lab[lab == -1] = LABEL_NONE
    if members is not None:
        lab[~np.asarray(members, dtype=bool)] = LABEL_NONE
    values, counts = np.unique(lab[lab != LABEL_NONE], return_counts=True)
    return n, len(values), int(counts.sum()), int(counts.max()) if len(counts) else 0


def spread_groups(nq, groups, fill, seed):
    """want [nq]: label g on c queries for (g, c) in `groups`, at positions drawn at random (members of a group are not
    adjacent but spread over the batch), `fill` elsewhere"""
    want = np.full(nq, fill, dtype=np.int64)
    spots = np.random.default_rng(seed).permutation(nq)
    at = 0
    for g, c in groups:
        want[spots[at:at + c]] = g
        at += c
    assert at <= nq
    return want
