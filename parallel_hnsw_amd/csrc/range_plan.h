// How the exact search by a numeric range of a row attribute (filter_ranged.hip) is cut: pure integer rules, shared by
// the launcher, the kernels and tests/cpp/test_range_plan.cpp (which runs them under the host sanitizers, no GPU).
//
// Every vector carries one u32 key, compared as an unsigned integer; the handle keeps the listed rows sorted by
// (key, id): skeys[listed] ascending, ids[listed] ascending within equal keys.  A query wants lo <= key <= hi, both ends
// inclusive: ONE contiguous SPAN of that order, [lower_bound(lo), upper_bound(hi)), found with two binary searches;
// lo > hi is the empty range.  The key PH_RANGE_KEY_NONE (PHNSW_ATTR_NONE) is never in skeys, so hi = 0xFFFFFFFF is
// "no upper bound" and no row without a value ever passes.
//
// A span of `len` ids is read in batches of 64 and dealt to slices as label_plan.h deals a posting list; the batch is
// sorted by span start, so that waves resident together read neighbouring rows.
#pragma once
#include <stdint.h>

#include "label_plan.h"

#define PH_RANGE_KEY_NONE 0xFFFFFFFFu   // the key of a row without a value
#define PH_RANGE_SORT_EMPTY 0xFFFFFFFFu  // the sort key of an empty span: behind every start (a start is < listed <= n < 2^32 - 1)

// the first index whose key is not below lo: ph_label_lower_bound; the first index whose key is above hi:
PH_EXACT_HD static inline uint64_t ph_range_upper_bound(const uint32_t *skeys, uint64_t listed, uint32_t hi) {
  uint64_t a = 0, b = listed;
  while (a < b) {
    const uint64_t mid = a + (b - a) / 2u;
    if (skeys[mid] <= hi)
      a = mid + 1u;
    else
      b = mid;
  }
  return a;
}

// the span of [lo, hi] in skeys[0 .. listed): *at + *len <= listed; an empty range (lo > hi, or no key inside) has
// *len == 0 and *at == 0
PH_EXACT_HD static inline void ph_range_span(const uint32_t *skeys, uint64_t listed, uint32_t lo, uint32_t hi, uint32_t *at,
                                             uint32_t *len) {
  *at = 0u, *len = 0u;
  if (lo > hi) return;
  const uint64_t b = ph_label_lower_bound(skeys, listed, lo), e = ph_range_upper_bound(skeys, listed, hi);
  if (e <= b) return;  // (e >= b always: every key below lo is at most hi)
  *at = (uint32_t)b, *len = (uint32_t)(e - b);
}
PH_EXACT_HD static inline uint32_t ph_range_count(const uint32_t *skeys, uint64_t listed, uint32_t lo, uint32_t hi) {
  uint32_t at, len;
  ph_range_span(skeys, listed, lo, hi, &at, &len);
  return len;
}

// what the batch is sorted by: the span's start; the empty spans sit together at the end
PH_EXACT_HD static inline uint32_t ph_range_sort_key(uint32_t at, uint32_t len) { return len ? at : PH_RANGE_SORT_EMPTY; }

// ---- scratch of one call; every figure in 64 bits
// words of the grouping block, [nq] each, by LOOKUP position p unless said: key (the sort key), iota (p itself, the
// sort's value), query (the query p stands for: ph_label_seed), at and len (the span), skey and sorted (by position of
// the sorted batch: its key, its lookup position).  The per-slice key lists [nq][slices][k] are label_plan.h's
// (ph_label_key_bytes), addressed by lookup position.
struct PhRangePre {
  uint64_t key, iota, query, at, len, skey, sorted, words;
};
static inline PhRangePre ph_range_pre(uint64_t nq) {
  PhRangePre l;
  uint64_t w = 0;
  l.key = w, w += nq;
  l.iota = w, w += nq;
  l.query = w, w += nq;
  l.at = w, w += nq;
  l.len = w, w += nq;
  l.skey = w, w += nq;
  l.sorted = w, w += nq;
  l.words = w;
  return l;
}
