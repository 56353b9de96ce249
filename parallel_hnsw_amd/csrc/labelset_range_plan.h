// How the exact search by a SET of row labels AND a numeric range (phnsw_search_exact_labelset_ranged,
// filter_label_ranged.hip) is cut: pure integer rules on top of labelset_plan.h and label_range_plan.h, shared by the
// launcher, the kernels and tests/cpp/test_labelset_range_plan.cpp (host sanitizers, no GPU).
//
// A batch carries its sets in CSR form, want_first[nq + 1] and want_values[nwant], and ONE range lo[q] .. hi[q] per
// query, shared by every label of the query's set.  PAIR i < nwant is (its owning query, want_values[i]); which query
// owns a pair is labelset_plan.h's claim, unchanged.  The list of a pair is a SPAN of the column sorted by
// (label << 32) | key, not a posting list: ph_label_range_span(spairs, listed, want_values[i], lo[owner], hi[owner]).
// The pairs are sorted, stably, by ph_label_range_sort_key of their span, as the label-range scan sorts queries; a
// POSITION is a pair in that order.  A wave per query then merges the lists of its positions.
//
// DUPLICATES (SHIPPED: this rule, on the span-start order; not the (label, query) order of labelset_plan.h).  A
// position duplicates its predecessor iff both belong to the same query and have the same non-empty span.  Why that
// finds every repeated label of a query that owns its whole range (a refused query's row is empty whatever is scanned):
//   1. Two pairs of one query have the same non-empty span iff they want the same label: the bounds are the query's, so
//      equal labels give equal spans; a non-empty span starts at a row of spairs that carries the span's label, so equal
//      starts give equal labels (spans of different labels are disjoint).
//   2. Non-empty spans sort by their start, empty ones by PH_RANGE_SORT_EMPTY, which is no start (a start is below
//      listed <= n < 2^32 - 1): the positions with one start are one run of the sorted order, all non-empty.
//   3. The sort is stable, so a run keeps pair order.  The pairs of a query that owns its range are contiguous in pair
//      order, so between two of them in a run lie only pairs of that query, which by 1. want the same label.  The pairs
//      of one (query, label) with a non-empty span are therefore ADJACENT positions, and every one but the first sees
//      its duplicate directly before it.
// Empty spans need no test: they contribute nothing, once or ten times.  A run may hold pairs of several queries that
// want the same label from the same start; they differ in the query and are no duplicates.
// tests/cpp/test_labelset_range_plan.cpp checks the consequence against brute force: the kept positions of a query are
// exactly its distinct labels with non-empty spans.
#pragma once
#include <stdint.h>

#include "label_range_plan.h"
#include "labelset_plan.h"

// position p > 0 with span (at, len) of query `query` repeats the position before it
PH_EXACT_HD static inline bool ph_labelset_range_dup(uint32_t at, uint32_t len, uint32_t query, uint32_t at_before, uint32_t len_before,
                                                     uint32_t query_before) {
  return len != 0u && query == query_before && at == at_before && len == len_before;
}

// what pair i of the range [b, e) of a query adds to the query's count: the length of its span, and nothing when an
// earlier pair of the range wants the same label (sets are short; no sort, no scratch).  b <= i < e <= nwant.
PH_EXACT_HD static inline uint32_t ph_labelset_range_count_pair(const uint64_t *spairs, uint64_t listed, const uint32_t *want_values,
                                                                uint32_t b, uint32_t i, uint32_t lo, uint32_t hi) {
  const uint32_t w = want_values[i];
  for (uint32_t j = b; j < i; j++)
    if (want_values[j] == w) return 0u;
  return ph_label_range_count(spairs, listed, w, lo, hi);
}
// the candidates of a query: the spans of the DISTINCT labels of its range; a range that is not sound counts 0
PH_EXACT_HD static inline uint32_t ph_labelset_range_count(const uint64_t *spairs, uint64_t listed, const uint32_t *want_values,
                                                           uint64_t b, uint64_t e, uint64_t nwant, uint32_t lo, uint32_t hi) {
  if (!ph_labelset_range_ok(b, e, nwant)) return 0u;
  uint32_t c = 0;
  for (uint32_t i = (uint32_t)b; i < (uint32_t)e; i++) c += ph_labelset_range_count_pair(spairs, listed, want_values, (uint32_t)b, i, lo, hi);
  return c;
}

// ---- scratch of one call.  The grouping block is ph_labelset_pre(nwant)'s, its arrays read as follows -- by pair:
// pos.slot = the sort key, pos.iota = the pair itself (the sort's value), pos.tile_first = the span's start,
// pos.flags = its length, owner, inv; by position: pos.sslot = the sorted key, spair, pos.order = the query, dup.
// The per-slice key lists [nwant positions][slices][k] are ph_labelset_key_bytes'.
