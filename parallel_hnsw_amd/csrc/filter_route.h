// How the routed filtered search (filter_auto.hip, phnsw_search_filtered_auto) decides: pure integer rules without a
// pointer, shared by the entry points, the kernels and tests/cpp/test_filter_route.cpp (which runs them under the host
// sanitizers, no GPU).
//
// Per query, with c = its candidates as phnsw_filter_count_device counts them, N = nodes of the bottom layer,
// ef = number_of_candidates:
//   scan   iff  c <= scan_below  or  c * ef < k * N   (the walk's post-filter keeps about ef * c / N of its queue:
//               fewer than k of them are expected to survive)
//   graph  otherwise; a graph row that comes back with fewer than min(k, c - e) entries is scanned after all
//               (e = 1 iff exclude[q] is itself among the c)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PH_ROUTE_HD __host__ __device__
#else
#define PH_ROUTE_HD
#endif

// the values of phnsw.h's PHNSW_ROUTE_* (filter_auto.hip asserts that they agree)
#define PH_ROUTE_GRAPH 0u
#define PH_ROUTE_SCAN 1u
#define PH_ROUTE_GRAPH_THEN_SCAN 2u

#define PH_AUTO_EF_MAX 1024u  // largest number_of_candidates of a search, hence the largest k
// scan_below == 0: the measured crossover of the two calls (profiles/filter_exact/README.md: 1M x 768 f32 rows, k = 10,
// batches of 10 000 queries; other store kinds and shapes are unmeasured)
#define PH_AUTO_SCAN_BELOW_SHARED 13000u     // one bitmap for the batch
#define PH_AUTO_SCAN_BELOW_PER_QUERY 10000u  // a bitmap per query
// a label per query (phnsw_search_labeled_auto): the measured crossover of phnsw_search_exact_labeled and the label walk
// (profiles/labeled_walk/README.md, "Crossover": at 20 000 rows per label the scan took 17.8 ms against the walk's 22.0,
// at 25 000 rows 22.0 against 21.5 -- 1M x 768 f32 rows, ef 256 / probe_depth 8, k = 10, 10 000 queries; other shapes
// are unmeasured)
#define PH_AUTO_SCAN_BELOW_LABELED 20000u

// the threshold a call runs with.  UINT64_MAX stays what it is: no count exceeds it, every query is scanned
PH_ROUTE_HD static inline uint64_t ph_auto_scan_below(uint64_t scan_below, bool per_query) {
  if (scan_below != 0u) return scan_below;
  return per_query ? PH_AUTO_SCAN_BELOW_PER_QUERY : PH_AUTO_SCAN_BELOW_SHARED;
}
// ... of a call by label
PH_ROUTE_HD static inline uint64_t ph_auto_scan_below_labeled(uint64_t scan_below) {
  return scan_below != 0u ? scan_below : PH_AUTO_SCAN_BELOW_LABELED;
}
// e of ph_auto_full_len for a call by label: exclude[q] is a candidate iff it is listed under want[q].  label_of [n]
// holds none_label for a vector that is not listed, and a query that wants none_label has no candidates
PH_ROUTE_HD static inline bool ph_auto_label_candidate(const uint32_t *label_of, uint32_t n, uint32_t want, uint32_t v,
                                                       uint32_t none_label) {
  return v < n && want != none_label && label_of[v] == want;
}

// ---- a numeric range per query (phnsw_search_batch_ranged, phnsw_search_ranged_auto): attr_of [n] holds the key of a
// listed vector and none_key elsewhere; a vector passes iff lo <= key <= hi and the key is a value.  Used by the search
// kernels' range mode (search_kernels.h), by filter_auto.hip and by tests/cpp/test_range_plan.cpp.
// scan_below == 0 of the routed call by range: UNMEASURED.  This is the one-label figure above; the range scan has no
// tile path (the label tile path measured 2.2-3.6x faster than the per-query scan), so its crossover with the range walk
// is expected BELOW this number.  scripts/bench_ranged.py --crossover measures it (profiles/ranged/README.md)
#define PH_AUTO_SCAN_BELOW_RANGED 20000u
PH_ROUTE_HD static inline uint64_t ph_auto_scan_below_ranged(uint64_t scan_below) {
  return scan_below != 0u ? scan_below : PH_AUTO_SCAN_BELOW_RANGED;
}
// the range test of one key, the form the walk's lanes run
PH_ROUTE_HD static inline bool ph_range_holds(uint32_t key, uint32_t lo, uint32_t hi, uint32_t none_key) {
  return key >= lo && key <= hi && key != none_key;
}
// e of ph_auto_full_len for a call by range: exclude[q] is a candidate iff it is listed with a key inside [lo, hi]
PH_ROUTE_HD static inline bool ph_auto_range_candidate(const uint32_t *attr_of, uint32_t n, uint32_t lo, uint32_t hi, uint32_t v,
                                                       uint32_t none_key) {
  return v < n && ph_range_holds(attr_of[v], lo, hi, none_key);
}

// ---- a label AND a numeric range per query (phnsw_search_batch_label_ranged, phnsw_search_label_ranged_auto): pair_of
// [n] holds the composite (label << 32) | key of a listed vector and none_pair (UINT64_MAX) elsewhere; a vector passes
// iff lo64 <= pair <= hi64 and the pair is a listed one, with lo64 = want << 32 | lo and hi64 = want << 32 | hi.  An
// empty range (lo > hi) gives lo64 > hi64, and a query that wants the NONE label can only be met by none_pair, which the
// third term refuses: both pass nothing without a test of want or of the bounds.  Used by the search kernels'
// label-range mode (search_kernels.h), by filter_auto.hip and by tests/cpp/test_label_range_plan.cpp.
// scan_below == 0 of the routed call by label and range: UNMEASURED.  This is the ranged figure above, itself
// unmeasured; scripts/bench_label_ranged.py --crossover measures it (profiles/label_ranged/README.md)
#define PH_AUTO_SCAN_BELOW_LABEL_RANGED PH_AUTO_SCAN_BELOW_RANGED
PH_ROUTE_HD static inline uint64_t ph_auto_scan_below_label_ranged(uint64_t scan_below) {
  return scan_below != 0u ? scan_below : PH_AUTO_SCAN_BELOW_LABEL_RANGED;
}
// the test of one composite, the form the walk's lanes run
PH_ROUTE_HD static inline bool ph_pair_holds(uint64_t pair, uint64_t lo64, uint64_t hi64, uint64_t none_pair) {
  return pair >= lo64 && pair <= hi64 && pair != none_pair;
}
PH_ROUTE_HD static inline uint64_t ph_pair_bound(uint32_t want, uint32_t key) { return ((uint64_t)want << 32) | (uint64_t)key; }
// ph_pair_holds(pair, ph_pair_bound(want, lo), ph_pair_bound(want, hi), none_pair) word by word, equal to it for every
// input: the composites order by the label first, so both 64-bit compares hold iff the label word IS want and the key
// word lies inside [lo, hi].  The form the search kernels run: three wave-uniform words per query, no 64-bit bound to
// put together per lane (profiles/label_ranged)
PH_ROUTE_HD static inline bool ph_pair_holds_words(uint64_t pair, uint32_t want, uint32_t lo, uint32_t hi, uint64_t none_pair) {
  const uint32_t lbl = (uint32_t)(pair >> 32), key = (uint32_t)pair;
  return lbl == want && key >= lo && key <= hi && pair != none_pair;
}
// e of ph_auto_full_len for a call by label and range: exclude[q] is a candidate iff it is listed under want with a key
// inside [lo, hi]
PH_ROUTE_HD static inline bool ph_auto_pair_candidate(const uint64_t *pair_of, uint32_t n, uint32_t want, uint32_t lo, uint32_t hi,
                                                      uint32_t v, uint64_t none_pair) {
  return v < n && ph_pair_holds(pair_of[v], ph_pair_bound(want, lo), ph_pair_bound(want, hi), none_pair);
}

// ---- a SET of labels per query (phnsw_search_batch_labelset, phnsw_search_labelset_auto): want_first [nq + 1] offsets
// into want_values [nwant].  Used by the search kernels' set mode (search_kernels.h), by filter_auto.hip and by
// tests/cpp/test_labelset_route.cpp.
// scan_below == 0 of the routed call by set: the measured crossover of phnsw_search_exact_labelset and the walk by set in
// candidates of the UNION (profiles/labelset_walk/README.md, "Crossover": sets of 4 labels; at a union of 20 000 rows the
// scan took 17.6 ms against the walk's 22.0, at 40 000 rows 34.2 against 20.3, the lines cross near 25 000 -- 1M x 768 f32
// rows, ef 256 / probe_depth 8, k = 10, 10 000 queries; other set sizes and shapes are unmeasured).  The last measured
// count at which the scan still won, which happens to be the one-label figure
#define PH_AUTO_SCAN_BELOW_LABELSET 20000u
PH_ROUTE_HD static inline uint64_t ph_auto_scan_below_labelset(uint64_t scan_below) {
  return scan_below != 0u ? scan_below : PH_AUTO_SCAN_BELOW_LABELSET;
}
// the range [first, last) of a query is sound: inside [0, nwant] and not backwards.  The offsets of a device call are
// not trusted: a query whose range is not sound reads nothing of want_values (status 8, an empty row)
PH_ROUTE_HD static inline bool ph_set_range_sound(uint64_t first, uint64_t last, uint64_t nwant) {
  return first <= last && last <= nwant;
}
// the membership test of the set mode, written for one id: v passes iff its label is a label (not none_label) and one of
// values[first .. last).  Duplicates and none_label in the set need no handling: a duplicate matches what its first copy
// matches, and none_label is never the label of a passing vector.  The caller has found the range sound.
PH_ROUTE_HD static inline bool ph_set_holds(uint32_t lbl, uint32_t first, uint32_t last, const uint32_t *values,
                                            uint32_t none_label) {
  bool hit = false;
  for (uint32_t i = first; i < last; i++) hit |= values[i] == lbl;
  return hit && lbl != none_label;
}
// e of ph_auto_full_len for a call by set: exclude[q] is a candidate iff it is listed under a label of the set
PH_ROUTE_HD static inline bool ph_auto_set_candidate(const uint32_t *label_of, uint32_t n, uint32_t first, uint32_t last,
                                                     const uint32_t *values, uint32_t v, uint32_t none_label) {
  return v < n && ph_set_holds(label_of[v], first, last, values, none_label);
}

// ---- a SET of labels AND a numeric range per query (phnsw_search_batch_labelset_ranged,
// phnsw_search_labelset_ranged_auto): pair_of as in the label-range calls, the set as in the calls by set, and ONE range
// lo .. hi per query, shared by every label of its set.  Used by the search kernels' set-range mode (search_kernels.h),
// by filter_auto.hip and by tests/cpp/test_labelset_range_plan.cpp.
// scan_below == 0 of the routed call by set and range: the measured crossover of phnsw_search_exact_labelset_ranged and
// the walk by set and range in candidates of the UNION (profiles/labelset_ranged/README.md, "Crossover": sets of 4 labels;
// at a union of 5 000 rows the scan took 20.8 ms against the walk's 23.6, at 10 000 rows 40.2 against 22.3 -- 1M x 768 f32
// rows, ef 256 / probe_depth 8, k = 10, 10 000 queries; other set sizes and shapes are unmeasured).  The last measured
// count at which the scan still won: this scan has no tile path, so it lies below the figure of the scan by set
#define PH_AUTO_SCAN_BELOW_LABELSET_RANGED 5000u
PH_ROUTE_HD static inline uint64_t ph_auto_scan_below_labelset_ranged(uint64_t scan_below) {
  return scan_below != 0u ? scan_below : PH_AUTO_SCAN_BELOW_LABELSET_RANGED;
}
// the test of one composite: its label word is one of values[first .. last) and its key word lies inside [lo, hi].  A
// NONE label in the set can only match none_pair's top word, which the last term refuses (a listed composite's label is
// at most 0xFFFFFFFE); lo > hi passes nothing without a scalar test; a duplicate matches what its first copy matches.
// The caller has found the range [first, last) sound.
PH_ROUTE_HD static inline bool ph_pairset_holds(uint64_t pair, uint32_t first, uint32_t last, const uint32_t *values, uint32_t lo,
                                                uint32_t hi, uint64_t none_pair) {
  const uint32_t lbl = (uint32_t)(pair >> 32), key = (uint32_t)pair;
  bool hit = false;
  for (uint32_t i = first; i < last; i++) hit |= values[i] == lbl;
  return hit && key >= lo && key <= hi && pair != none_pair;
}
// e of ph_auto_full_len for a call by set and range: exclude[q] is a candidate iff it passes the walk's predicate
PH_ROUTE_HD static inline bool ph_auto_pairset_candidate(const uint64_t *pair_of, uint32_t n, uint32_t first, uint32_t last,
                                                         const uint32_t *values, uint32_t lo, uint32_t hi, uint32_t v,
                                                         uint64_t none_pair) {
  return v < n && ph_pairset_holds(pair_of[v], first, last, values, lo, hi, none_pair);
}

// the route of a query with c candidates.  c and n_nodes are 32-bit counts, ef and k at most 1024: the two products
// stay below 2^42 and cannot wrap
PH_ROUTE_HD static inline uint32_t ph_auto_route(uint32_t c, uint64_t scan_below, uint32_t ef, uint32_t k, uint32_t n_nodes) {
  if ((uint64_t)c <= scan_below) return PH_ROUTE_SCAN;
  return (uint64_t)c * (uint64_t)ef < (uint64_t)k * (uint64_t)n_nodes ? PH_ROUTE_SCAN : PH_ROUTE_GRAPH;
}

// entries a complete row of a query holds: min(k, c - e); excluded is 1 only when exclude[q] is one of the c
PH_ROUTE_HD static inline uint32_t ph_auto_full_len(uint32_t c, uint32_t excluded, uint32_t k) {
  const uint32_t left = c - (excluded && c ? 1u : 0u);
  return left < k ? left : k;
}

// ---- argument checks
static inline bool ph_auto_ef_valid(uint64_t ef) { return ef >= 1u && ef <= PH_AUTO_EF_MAX; }
static inline bool ph_auto_k_valid(uint64_t k, uint64_t ef) { return ph_auto_ef_valid(ef) && k >= 1u && k <= ef; }
// exactly one of queries / qids
static inline bool ph_auto_queries_valid(bool has_queries, bool has_qids) { return has_queries != has_qids; }
// 0 = one shared bitmap, else at least the ceil(n / 32) words of one bitmap
static inline bool ph_auto_stride_valid(uint64_t stride_words, uint64_t n) { return stride_words == 0u || stride_words >= (n + 31u) / 32u; }
static inline bool ph_auto_nq_valid(uint64_t nq) { return nq <= 0xFFFFFFFFull; }

// ---- capacities of a call's device scratch, in 32-bit words.  One block:
//   head[PH_AUTO_HEAD_WORDS] | counts[bitmaps] | graph list[nq] | scan list[nq] | route[nq] | walk len[nq] |
//   walk ids[nq][ef] | walk distances[nq][ef]
// Every query is in at most one of the two lists at a time (a short graph row moves over), so nq entries hold either.
#define PH_AUTO_HEAD_WORDS 4u  // [0] length of the graph list, [1] of the scan list
static inline uint64_t ph_auto_bitmaps(uint64_t nq, bool per_query) { return per_query ? nq : 1u; }
static inline uint64_t ph_auto_list_words(uint64_t nq) { return nq; }
static inline uint64_t ph_auto_scratch_words(uint64_t nq, bool per_query, uint64_t ef) {
  return PH_AUTO_HEAD_WORDS + ph_auto_bitmaps(nq, per_query) + 2u * ph_auto_list_words(nq) + 2u * nq + 2u * nq * ef;
}
