"""Pure-Python pieces of tests/test_gpu_filter_scale.py: where the library's integer rules cut a bitmap or a batch
(restated, so that a test can say which loop its shape turns), the numpy popcount that filter_count is held against,
and the makers of masks and batches.  Nothing here computes a distance.  Pinned by tests/test_filter_scale_cpu.py."""
import numpy as np

PASS_WORDS, PASS_IDS = 64, 2048  # exact_slices.h: bitmap words and ids of one pass of the scan
COUNT_THREADS = 256              # ph_filter_count_kernel: words per trip of its loop
PREFIX_WORDS = 1024              # ph_dense_prefix_kernel: words per trip
ROUTE_QUERIES = 256              # ph_auto_route_kernel: queries per trip
DENSE_NODES, DENSE_NODES_MAX = 8192, 65536  # dense_plan.h: ids per node chunk, default and clamp


def words_of(n):
    return (int(n) + 31) // 32


def passes_of(n):
    return (words_of(n) + PASS_WORDS - 1) // PASS_WORDS


def trips(count, per_trip):
    """turns of a loop that takes per_trip items a time over count items"""
    return (int(count) + per_trip - 1) // per_trip


def slice_ranges(passes, slices):
    """ph_exact_slice_range for every slice after ph_exact_slice_count's clamp: [(p0, p1)], tiling [0, passes)"""
    s = max(1, min(int(slices), int(passes)))
    return [(i * passes // s, (i + 1) * passes // s) for i in range(s)]


def node_chunks(c, knob=0):
    """ids per node chunk of the shared table for c candidates under PHNSW_DENSE_NODES=knob (0: unset): dense_plan.h"""
    nodes = DENSE_NODES if knob <= 0 else min((int(knob) + 63) // 64 * 64, DENSE_NODES_MAX)
    return [min(nodes, c - at) for at in range(0, int(c), nodes)]


def host_chunk_bounds(nq, pipe_min, first, piece):
    """plan_chunks of the host path under PHNSW_HOST_CHUNKS="pipe_min,first,piece": the chunk borders in the list"""
    if nq < pipe_min:
        return [0, nq]
    at = min(first, nq)
    rest = nq - at
    pieces = max(1, (rest + piece - 1) // piece)
    return [0, at] + [at + rest * p // pieces for p in range(1, pieces + 1)]


def popcount_candidates(words, n, members=None):
    """candidates of packed bitmaps, counted without the library: u32 words [>= ceil(n/32)] or [nb, stride] -> int64
    [nb].  Bit v % 32 of word v // 32 is VectorId v; bits at and past n, and words past ceil(n/32), do not count, nor do
    vectors outside `members` (bool [n], None = all)"""
    w = np.ascontiguousarray(np.atleast_2d(np.asarray(words, dtype=np.uint32))[:, :words_of(n)]).astype("<u4")
    set_bits = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(np.bool_)
    if members is not None:
        set_bits &= np.asarray(members, dtype=np.bool_)[None, :]
    return set_bits.sum(axis=1, dtype=np.int64)


def words_mask(n, words):
    """bool [n]: every id of the listed bitmap words (those below n)"""
    m = np.zeros(words_of(n) * 32, dtype=np.bool_)
    for w in words:
        m[int(w) * 32:int(w) * 32 + 32] = True
    return m[:n].copy()


def exactly_of(n, count, seed, first=()):
    """bool [n] with exactly `count` ids set: those of `first` (as many as fit), the rest drawn at random"""
    m = np.zeros(n, dtype=np.bool_)
    take = np.asarray(first, dtype=np.int64)[:count]
    m[take] = True
    perm = np.random.default_rng(seed).permutation(n)
    m[perm[~np.isin(perm, take)][:count - len(take)]] = True
    assert m.sum() == count
    return m


def cycle_counts(nq, cycle):
    """query q gets cycle[q % len(cycle)]"""
    return [int(cycle[i % len(cycle)]) for i in range(nq)]


def arranged_counts(nq, split, head, tail):
    """queries below `split` cycle through `head`, the others through `tail`"""
    return cycle_counts(split, head) + cycle_counts(nq - split, tail)


def bitmaps_of(n, counts, seed, pool=None):
    """bool [len(counts), n]: query q allows counts[q] ids drawn at random from `pool` (ids, None = all below n)"""
    rng = np.random.default_rng(seed)
    pool = np.arange(n) if pool is None else np.asarray(pool, dtype=np.int64)
    allow = np.zeros((len(counts), n), dtype=np.bool_)
    for i, c in enumerate(counts):
        assert 0 <= c <= len(pool)
        if c == len(pool):
            allow[i, pool] = True
        elif c:
            allow[i, pool[np.argpartition(rng.random(len(pool)), c - 1)[:c]]] = True
    return allow
