// How the exact top-k for a TABLE of allow-lists (filter_grouped.hip) groups a batch and bounds its scratch: pure
// integer rules, shared by the launcher, its kernels and tests/cpp/test_group_plan.cpp (which runs them under the host
// sanitizers, no GPU).
//
// Every query gets a 32-bit KEY from its selector: the bitmap's number, nfilters for PHNSW_FILTER_ALL, 0xFFFFFFFF for a
// query that is refused (a selector outside the table, a Stored query id at or past n).  The queries sorted by key
// (stably, so by query index inside a key) are the POSITIONS; the positions of one key are a GROUP, and the groups in
// position order are in ascending bitmap order, then the ALL group, then the reject group.  A group with c candidates
// costs (c + nwords + 1) 4-byte words of list scratch: its ascending id list and the per-word offsets the list is
// built from.  Groups are taken in ROUNDS, in order: a round takes groups while their cost fits the byte budget and
// their number the grid, and always at least one.  All products in 64 bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PH_GROUP_HD __host__ __device__
#else
#define PH_GROUP_HD
#endif

#define PH_GROUP_LIST_BYTES_DEFAULT (256ull << 20)  // PHNSW_GROUP_LIST_BYTES
#define PH_GROUP_LIST_BYTES_MAX (16ull << 30)       // ... clamped to this
#define PH_GROUP_ROUND_GROUPS_MAX 32768u            // groups of one round: the y extent of the list kernels' grids
#define PH_GROUP_HEAD_WORDS 4u                      // [0] the number of groups
#define PH_GROUP_KEY_REJECT 0xFFFFFFFFu
#define PH_GROUP_SELECT_ALL 0xFFFFFFFFu             // PHNSW_FILTER_ALL
#define PH_GROUP_NFILTERS_MAX 0xFFFFFFFEull
#define PH_GROUP_NQ_MAX 0x7FFFFFFEull  // the grouping pass sorts and scans nq + 1 entries with 32-bit signed counts
// why a query is in the reject group, as its status word: phnsw.h
#define PH_GROUP_ST_OK 0u
#define PH_GROUP_ST_MISSING 4u   // a Stored query id at or past n
#define PH_GROUP_ST_SELECTOR 6u  // a selector outside the table
#define PH_GROUP_ST_CHANGED 7u   // the query's bitmap changed while the call read it

// the knob as the launcher takes it: 0 or negative = the default, anything else clamped
static inline uint64_t ph_group_bytes_knob(long long v) {
  if (v <= 0) return PH_GROUP_LIST_BYTES_DEFAULT;
  return (uint64_t)v > PH_GROUP_LIST_BYTES_MAX ? PH_GROUP_LIST_BYTES_MAX : (uint64_t)v;
}

// the key of a selector (nfilters <= PH_GROUP_NFILTERS_MAX, so nfilters itself is a key no bitmap has)
PH_GROUP_HD static inline uint32_t ph_group_key(uint32_t selector, uint64_t nfilters) {
  if (selector == PH_GROUP_SELECT_ALL) return (uint32_t)nfilters;
  return selector < nfilters ? selector : PH_GROUP_KEY_REJECT;
}
// ... and the bitmap a key names: word offset into the table, or no bitmap (ALL: every vector; reject: none is read)
PH_GROUP_HD static inline bool ph_group_key_has_bitmap(uint32_t key, uint64_t nfilters) { return key < nfilters; }
PH_GROUP_HD static inline uint64_t ph_group_bitmap_at(uint32_t key, uint32_t stride_words) {
  return (uint64_t)key * stride_words;
}

// groups a batch can have at most: one per bitmap, ALL, reject -- and never more than queries
static inline uint64_t ph_group_max(uint64_t nq, uint64_t nfilters) {
  const uint64_t g = nfilters + 2u;
  return nq < g ? nq : g;
}

// list scratch of one group, in words and for a round in bytes
PH_GROUP_HD static inline uint64_t ph_group_off_words(uint64_t nwords) { return nwords + 1u; }
static inline uint64_t ph_group_cost_words(uint64_t c, uint64_t nwords) { return c + ph_group_off_words(nwords); }

// the round that starts at group g0 (g0 < ngroups): groups [g0, return value); counts[g] <= 2^31 - 1
static inline uint64_t ph_group_round_end(const uint32_t *counts, uint64_t ngroups, uint64_t g0, uint64_t nwords,
                                          uint64_t budget_bytes) {
  uint64_t words = ph_group_cost_words(counts[g0], nwords), g = g0 + 1u;
  while (g < ngroups && g - g0 < PH_GROUP_ROUND_GROUPS_MAX) {
    const uint64_t next = words + ph_group_cost_words(counts[g], nwords);
    if (next * 4u > budget_bytes) break;
    words = next, g++;
  }
  return g;
}
// inside the round [g0, g1): the offsets of group g are word (g - g0) * (nwords + 1) of the offset area, which holds
// (g1 - g0) * (nwords + 1) words; its list starts at entry sum(counts[g0 .. g)) of the list area
static inline uint64_t ph_group_round_off_words(uint64_t g0, uint64_t g1, uint64_t nwords) {
  return (g1 - g0) * ph_group_off_words(nwords);
}
static inline uint64_t ph_group_round_list_words(const uint32_t *counts, uint64_t g0, uint64_t g1) {
  uint64_t s = 0;
  for (uint64_t g = g0; g < g1; g++) s += counts[g];
  return s;
}
// the list block: the largest round's offsets and lists, in bytes
static inline uint64_t ph_group_list_bytes(const uint32_t *counts, uint64_t ngroups, uint64_t nwords, uint64_t budget_bytes,
                                           uint64_t *rounds) {
  uint64_t most = 0, r = 0;
  for (uint64_t g0 = 0; g0 < ngroups; r++) {
    const uint64_t g1 = ph_group_round_end(counts, ngroups, g0, nwords, budget_bytes);
    const uint64_t w = ph_group_round_off_words(g0, g1, nwords) + ph_group_round_list_words(counts, g0, g1);
    if (w > most) most = w;
    g0 = g1;
  }
  if (rounds) *rounds = r;
  return most * 4u;
}

// The scratch sized BEFORE anything is known, in 4-byte words (the 8-byte cumulative counts start at an even word, so
// they are aligned when the block is):
//   head | gfirst [G + 1] | gkey [G] | gcount [G] | gcum [G + 1] as 64-bit | gerr [G] | keys [nq] | sorted keys [nq] |
//   iota [nq] | order [nq] | flags [nq + 1] | slots [nq + 1] | safe qids [nq] | why [nq]
// head .. gcount are contiguous from word 0: the one read of the call fetches exactly them.
static inline uint64_t ph_group_even(uint64_t w) { return (w + 1u) & ~1ull; }
struct PhGroupPre {
  uint64_t head, gfirst, gkey, gcount, gcum, gerr, keys, skeys, iota, order, flags, slots, safe, why;  // first words
  uint64_t read_words;  // words [0, read_words) are head .. gcount
  uint64_t words;       // the block
};
static inline PhGroupPre ph_group_pre(uint64_t nq, uint64_t G) {
  PhGroupPre p;
  uint64_t at = 0;
  p.head = at, at += PH_GROUP_HEAD_WORDS;
  p.gfirst = at, at += G + 1u;
  p.gkey = at, at += G;
  p.gcount = at, at += G;
  p.read_words = at;
  at = ph_group_even(at);
  p.gcum = at, at += 2u * (G + 1u);
  p.gerr = at, at += ph_group_even(G);
  p.keys = at, at += ph_group_even(nq);
  p.skeys = at, at += ph_group_even(nq);
  p.iota = at, at += ph_group_even(nq);
  p.order = at, at += ph_group_even(nq);
  p.flags = at, at += ph_group_even(nq + 1u);
  p.slots = at, at += ph_group_even(nq + 1u);
  p.safe = at, at += ph_group_even(nq);
  p.why = at, at += ph_group_even(nq);
  p.words = at;
  return p;
}
// the [nq][k] key scratch of the select, indexed by the QUERY (8-byte keys), then the largest table of any group
static inline uint64_t ph_group_key_bytes(uint64_t nq, uint64_t k) { return nq * k * 8u; }
static inline uint64_t ph_group_post_bytes(uint64_t nq, uint64_t k, uint64_t table_floats_max) {
  return ph_group_key_bytes(nq, k) + table_floats_max * 4u;
}
