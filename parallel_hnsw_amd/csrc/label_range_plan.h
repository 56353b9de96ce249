// How the exact search by a row label AND a numeric range of a row attribute (filter_label_ranged.hip) is cut: pure
// integer rules, shared by the launcher, the kernels and tests/cpp/test_label_range_plan.cpp (which runs them under the
// host sanitizers, no GPU).
//
// Every vector carries one u32 label and one u32 key; the handle keeps the listed rows sorted by the 64-bit COMPOSITE
// (label << 32) | key, compared as an unsigned integer, then by id: spairs[listed] ascending, ids[listed] ascending
// within equal composites.  A query wants label == want and lo <= key <= hi, both ends inclusive: ONE contiguous SPAN of
// that order, [lower_bound(want << 32 | lo), upper_bound(want << 32 | hi)), found with two binary searches.  The span is
// empty when want is PH_LABEL_RANGE_NONE, when lo > hi, or when nobody carries the label.  The key PH_LABEL_RANGE_NONE
// (PHNSW_ATTR_NONE) is never in spairs, so hi = 0xFFFFFFFF is "no upper end within this label": the upper bound lands on
// the first row of the next label.  A listed composite never equals PH_LABEL_RANGE_PAIR_NONE: its top word is a label,
// at most 0xFFFFFFFE.
//
// A span of `len` ids is read in batches of 64 and dealt to slices as label_plan.h deals a posting list; the batch is
// sorted by span start, so that waves resident together read neighbouring rows.
#pragma once
#include <stdint.h>

#include "range_plan.h"

#define PH_LABEL_RANGE_NONE 0xFFFFFFFFu                 // the label of a row without one, the key of a row without a value
#define PH_LABEL_RANGE_PAIR_NONE 0xFFFFFFFFFFFFFFFFull  // the composite of a row that is not listed

// the composite of (label, key); the u64 bounds of a query are ph_label_range_pair(want, lo) and (want, hi)
PH_EXACT_HD static inline uint64_t ph_label_range_pair(uint32_t label, uint32_t key) { return ((uint64_t)label << 32) | (uint64_t)key; }

// the first index whose composite is not below lo64
PH_EXACT_HD static inline uint64_t ph_label_range_lower_bound(const uint64_t *spairs, uint64_t listed, uint64_t lo64) {
  uint64_t a = 0, b = listed;
  while (a < b) {
    const uint64_t mid = a + (b - a) / 2u;
    if (spairs[mid] < lo64)
      a = mid + 1u;
    else
      b = mid;
  }
  return a;
}
// the first index whose composite is above hi64
PH_EXACT_HD static inline uint64_t ph_label_range_upper_bound(const uint64_t *spairs, uint64_t listed, uint64_t hi64) {
  uint64_t a = 0, b = listed;
  while (a < b) {
    const uint64_t mid = a + (b - a) / 2u;
    if (spairs[mid] <= hi64)
      a = mid + 1u;
    else
      b = mid;
  }
  return a;
}

// the span of (want, [lo, hi]) in spairs[0 .. listed): *at + *len <= listed; an empty one (want NONE, lo > hi, nobody
// with the label, no key inside) has *len == 0 and *at == 0
PH_EXACT_HD static inline void ph_label_range_span(const uint64_t *spairs, uint64_t listed, uint32_t want, uint32_t lo, uint32_t hi,
                                                   uint32_t *at, uint32_t *len) {
  *at = 0u, *len = 0u;
  if (want == PH_LABEL_RANGE_NONE || lo > hi) return;
  const uint64_t b = ph_label_range_lower_bound(spairs, listed, ph_label_range_pair(want, lo));
  const uint64_t e = ph_label_range_upper_bound(spairs, listed, ph_label_range_pair(want, hi));
  if (e <= b) return;  // (e >= b always: every composite below the lower bound is at most the upper one)
  *at = (uint32_t)b, *len = (uint32_t)(e - b);
}
PH_EXACT_HD static inline uint32_t ph_label_range_count(const uint64_t *spairs, uint64_t listed, uint32_t want, uint32_t lo,
                                                        uint32_t hi) {
  uint32_t at, len;
  ph_label_range_span(spairs, listed, want, lo, hi, &at, &len);
  return len;
}

// what the batch is sorted by: the span's start; the empty spans sit together at the end (range_plan.h's rule)
PH_EXACT_HD static inline uint32_t ph_label_range_sort_key(uint32_t at, uint32_t len) { return ph_range_sort_key(at, len); }

// ---- scratch of one call: the grouping block is range_plan.h's (PhRangePre, ph_range_pre), the per-slice key lists
// [nq][slices][k] are label_plan.h's (ph_label_key_bytes), both addressed by lookup position.
