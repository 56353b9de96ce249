// Stand-alone host check of the integer rules behind the search by a numeric range (parallel_hnsw_amd/csrc/range_plan.h,
// the header the launcher and the kernels include, and the range candidate test of filter_route.h): compiled with
// -fsanitize=address,undefined and run without a GPU (tests/test_range_plan_cpp.py).  The span of a range against a
// brute-force count, the sort key of empty spans, the scratch layout in 64 bits, the candidate test of the routed call.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/filter_route.h"
#include "../../parallel_hnsw_amd/csrc/range_plan.h"

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

static const uint32_t NONE = 0xFFFFFFFFu;

// the span of [lo, hi] against what a walk over the whole array counts; the vector is copied to its exact size, so a
// read past either end is the sanitizer's
static void check_span(const std::vector<uint32_t> &keys, uint32_t lo, uint32_t hi) {
  std::vector<uint32_t> exact(keys);
  exact.shrink_to_fit();
  const uint32_t *p = exact.empty() ? nullptr : exact.data();
  uint32_t at = 77u, len = 77u;
  ph_range_span(p, exact.size(), lo, hi, &at, &len);
  uint64_t count = 0, first = 0;
  bool any = false;
  for (uint64_t i = 0; i < exact.size(); i++)
    if (exact[i] >= lo && exact[i] <= hi) {
      if (!any) first = i, any = true;
      count++;
    }
  CHECK(len == count && ph_range_count(p, exact.size(), lo, hi) == count);
  CHECK((uint64_t)at + len <= exact.size());
  if (count) {
    CHECK(at == first);
    for (uint32_t i = 0; i < len; i++) CHECK(exact[at + i] >= lo && exact[at + i] <= hi);  // contiguous
    CHECK(ph_range_sort_key(at, len) == at);
  } else {
    CHECK(at == 0u && ph_range_sort_key(at, len) == PH_RANGE_SORT_EMPTY);
  }
}

static void test_spans() {
  const std::vector<std::vector<uint32_t>> arrays = {
      {},                                         // empty
      {40},                                       // one key
      {7, 7, 7, 7, 7},                            // all keys equal
      {3, 3, 3, 10, 20, 30, 90, 90, 90, 90},      // plateaus at both ends
      {0, 0, 5, 6, 7, 100, 0xFFFFFFFEu},          // the smallest and the largest value there is
      {1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096},
  };
  for (const auto &keys : arrays) {
    std::vector<uint32_t> bounds = {0u, 1u, NONE, NONE - 1u, 0x80000000u};
    for (uint32_t k : keys)
      for (uint32_t d : {0u, 1u}) bounds.push_back(k - d), bounds.push_back(k + d);  // on a key, in the gaps beside it
    if (!keys.empty()) bounds.push_back(keys.front() / 2u), bounds.push_back(keys.back() + (NONE - keys.back()) / 2u);
    for (uint32_t lo : bounds)
      for (uint32_t hi : bounds) check_span(keys, lo, hi);  // lo > hi among them: empty, whatever lies between
  }
  // hi = 0xFFFFFFFF is "no upper bound"; lo > hi is empty although keys lie between
  const std::vector<uint32_t> k = {3, 3, 3, 10, 20, 30, 90, 90, 90, 90};
  CHECK(ph_range_count(k.data(), k.size(), 0u, NONE) == 10u && ph_range_count(k.data(), k.size(), 11u, NONE) == 6u);
  CHECK(ph_range_count(k.data(), k.size(), 90u, 3u) == 0u && ph_range_count(k.data(), k.size(), 91u, NONE) == 0u);
  CHECK(ph_range_count(k.data(), k.size(), 4u, 9u) == 0u && ph_range_count(k.data(), k.size(), 0u, 2u) == 0u);
  CHECK(ph_range_upper_bound(k.data(), k.size(), NONE) == 10u && ph_range_upper_bound(k.data(), 0, 5u) == 0u);
  // the empty spans sort behind every start a column below 2^32 - 1 rows can have
  CHECK(ph_range_sort_key(0u, 0u) == PH_RANGE_SORT_EMPTY && ph_range_sort_key(123u, 0u) == PH_RANGE_SORT_EMPTY);
  CHECK(ph_range_sort_key(0u, 1u) == 0u && ph_range_sort_key(0xFFFFFFFDu, 1u) < PH_RANGE_SORT_EMPTY);
}

static void test_scratch() {
  const uint64_t nq = PH_LABEL_NQ_MAX;
  const PhRangePre l = ph_range_pre(nq);
  CHECK(l.key == 0 && l.iota == nq && l.query == 2u * nq && l.at == 3u * nq && l.len == 4u * nq && l.skey == 5u * nq);
  CHECK(l.sorted == 6u * nq && l.words == 7u * nq && l.words > 0xFFFFFFFFull);  // counted in 64 bits
  CHECK(l.words * 4u / 4u == l.words);
  CHECK(ph_range_pre(1).words == 7u && ph_range_pre(0).words == 0u);
  uint64_t bytes = 0;  // the per-slice key lists are label_plan.h's
  CHECK(ph_label_key_bytes(nq, 7, 1024, &bytes) && bytes == nq * 7u * 8192u);
  CHECK(ph_label_slice_count(10, 1000, 5000, 0) == ph_exact_slice_count(10, 1000, ph_label_batches(5000), 0));
  CHECK(ph_label_slice_count(10, 1000, 0, 7) == 1u && ph_label_slice_count(10, 1000, 65, 7) == 2u);
}

static void test_route() {
  const uint32_t attr_of[] = {5u, NONE, 0u, 0xFFFFFFFEu, 9u};
  CHECK(ph_auto_range_candidate(attr_of, 5, 5u, 5u, 0u, NONE) && ph_auto_range_candidate(attr_of, 5, 0u, NONE, 3u, NONE));
  CHECK(!ph_auto_range_candidate(attr_of, 5, 0u, NONE, 1u, NONE));   // no value: in no range, not even the open one
  CHECK(!ph_auto_range_candidate(attr_of, 5, NONE, NONE, 1u, NONE));
  CHECK(!ph_auto_range_candidate(attr_of, 5, 6u, 8u, 0u, NONE) && !ph_auto_range_candidate(attr_of, 5, 9u, 5u, 0u, NONE));
  CHECK(!ph_auto_range_candidate(attr_of, 5, 0u, NONE, 5u, NONE));   // v >= n: nothing is read
  CHECK(!ph_auto_range_candidate(attr_of, 4, 0u, NONE, 4u, NONE) && !ph_auto_range_candidate(attr_of, 5, 0u, NONE, NONE, NONE));
  CHECK(ph_range_holds(0u, 0u, 0u, NONE) && !ph_range_holds(1u, 2u, 1u, NONE) && ph_range_holds(0xFFFFFFFEu, 0u, NONE, NONE));
  CHECK(ph_auto_scan_below_ranged(0) == PH_AUTO_SCAN_BELOW_RANGED && ph_auto_scan_below_ranged(5) == 5u);
  CHECK(ph_auto_scan_below_ranged(UINT64_MAX) == UINT64_MAX);
}

int main() {
  test_spans();
  test_scratch();
  test_route();
  std::printf("ALL OK\n");
  return 0;
}
