// How the exact search by a SET of row labels (phnsw_search_exact_labelset, filter_labeled.hip) is cut: pure integer
// rules, shared by the launcher, the kernels and tests/cpp/test_labelset_plan.cpp (host sanitizers, no GPU).
//
// A batch carries its sets in CSR form: want_first[nq + 1], want_values[nwant].  PAIR i < nwant is (the query whose
// range holds i, want_values[i]).  The machinery of label_plan.h runs over pairs: a POSITION of the sorted batch is a
// pair, not a query; positions of one slot form the tiles.  Equal (slot, query) pairs are adjacent after the stable
// sort; the second and later ones are DUPLICATES and contribute nothing.  A wave per query then merges the lists of
// its positions.
//
// The device form does not trust the offsets.  A query CLAIMS the pairs of its range only if the range passes
// ph_labelset_range_ok; a pair claimed by several queries belongs to the lowest (ranges of honest offsets are disjoint),
// and a query that does not own every pair of its range is refused like one whose range is bad.  A binary search of i
// in want_first would be cheaper, but one offset out of order sends the pairs of OTHER queries the wrong way.
#pragma once
#include <stdint.h>

#include "label_plan.h"

#define PH_LABELSET_OWNER_NONE 0xFFFFFFFFu  // a pair no query claimed
#define PH_LABELSET_NWANT_MAX PH_LABEL_NQ_MAX  // pairs of one call (the sort counts in int)

// the range [b, e) of a query (b = want_first[q], e = want_first[q + 1]) lies inside [0, nwant] and does not run backwards
PH_EXACT_HD static inline bool ph_labelset_range_ok(uint64_t b, uint64_t e, uint64_t nwant) { return b <= e && e <= nwant; }

// One claim: query q takes pair i unless a lower query holds it.  Returns whether q may go on claiming -- a pair of its
// range that a lower query holds already makes q a refused query.  The kernel's form is atomicMin on the same word.
PH_EXACT_HD static inline bool ph_labelset_claim_goes_on(uint32_t held_before, uint32_t q) { return held_before >= q; }
static inline bool ph_labelset_claim(uint32_t *owner, uint64_t i, uint32_t q) {
  const uint32_t before = owner[i];
  if (q < before) owner[i] = q;
  return ph_labelset_claim_goes_on(before, q);
}

// the first query whose offsets are unsound, nq if none: want_first[0] != 0 is query 0's, a range that runs backwards
// its own.  What the host form refuses before any device work.
static inline uint64_t ph_labelset_first_bad(const uint32_t *want_first, uint64_t nq) {
  if (nq && want_first[0] != 0u) return 0;
  for (uint64_t q = 0; q < nq; q++)
    if (want_first[q] > want_first[q + 1u]) return q;
  return nq;
}

// position p > 0 repeats the (slot, query) pair of the position before it
PH_EXACT_HD static inline bool ph_labelset_dup(uint32_t slot, uint32_t query, uint32_t slot_before, uint32_t query_before) {
  return slot == slot_before && query == query_before;
}

// ---- scratch of one call; every figure in 64 bits
// words of the grouping block: label_plan.h's block for nwant positions (its `order` holds the QUERY of a position),
// then owner [nwant] by pair, spair [nwant] by position (its pair), inv [nwant] by pair (its position), dup [nwant] by
// position
struct PhLabelsetPre {
  PhLabelPre pos;
  uint64_t owner, spair, inv, dup, words;
};
static inline PhLabelsetPre ph_labelset_pre(uint64_t nwant) {
  PhLabelsetPre l;
  l.pos = ph_label_pre(nwant);
  uint64_t at = l.pos.words;
  l.owner = at, at += nwant;
  l.spair = at, at += nwant;
  l.inv = at, at += nwant;
  l.dup = at, at += nwant;
  l.words = at;
  return l;
}
// bytes of the per-slice key lists [nwant positions][slices][k]: written at every slice count, one slice included
static inline bool ph_labelset_key_bytes(uint64_t nwant, uint64_t slices, uint64_t k, uint64_t *bytes) {
  return ph_label_key_bytes(nwant, slices, k, bytes);
}
