// Stand-alone host check of the integer rules behind the search by a row label and a numeric range
// (parallel_hnsw_amd/csrc/label_range_plan.h, the header the launcher and the kernels include, and ph_pair_holds of
// filter_route.h): compiled with -fsanitize=address,undefined and run without a GPU (tests/test_label_range_plan_cpp.py).
// The span of a (label, range) pair against a brute-force count over constructed columns, the sort key of empty spans,
// the walk's test of one composite in its two forms, the candidate test of the routed call.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/filter_route.h"
#include "../../parallel_hnsw_amd/csrc/label_range_plan.h"

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

static const uint32_t NONE = 0xFFFFFFFFu;
static const uint64_t NONE64 = 0xFFFFFFFFFFFFFFFFull;
typedef std::vector<std::pair<uint32_t, uint32_t>> Rows;  // (label, key) of the listed rows, in any order

// the sorted column of composites, written here and not with the header's function: label in the top word
static std::vector<uint64_t> column_of(const Rows &rows) {
  std::vector<uint64_t> c;
  for (const auto &r : rows) c.push_back((uint64_t)r.first * 4294967296ull + r.second);
  std::sort(c.begin(), c.end());
  c.shrink_to_fit();  // a read past either end is the sanitizer's
  return c;
}

// the span of (want, [lo, hi]) against what a walk over the rows counts, label and key compared as separate u32 words
static void check_span(const Rows &rows, uint32_t want, uint32_t lo, uint32_t hi) {
  const std::vector<uint64_t> c = column_of(rows);
  const uint64_t *p = c.empty() ? nullptr : c.data();
  uint32_t at = 77u, len = 77u;
  ph_label_range_span(p, c.size(), want, lo, hi, &at, &len);
  uint64_t count = 0, first = 0;
  bool any = false;
  for (uint64_t i = 0; i < c.size(); i++) {
    const uint32_t lbl = (uint32_t)(c[i] / 4294967296ull), key = (uint32_t)(c[i] % 4294967296ull);
    const bool in = want != NONE && lbl == want && key >= lo && key <= hi;
    if (in && !any) first = i, any = true;
    count += in ? 1u : 0u;
    // the walk's test of this composite, in both forms, says the same
    CHECK(ph_pair_holds(c[i], ph_pair_bound(want, lo), ph_pair_bound(want, hi), NONE64) == in);
    CHECK(ph_pair_holds_words(c[i], want, lo, hi, NONE64) == in);
  }
  CHECK(len == count && ph_label_range_count(p, c.size(), want, lo, hi) == count);
  CHECK((uint64_t)at + len <= c.size());
  if (count) {
    CHECK(at == first);
    for (uint32_t i = 0; i < len; i++) CHECK((uint32_t)(c[at + i] >> 32) == want);  // contiguous, one label
    CHECK(ph_label_range_sort_key(at, len) == at);
  } else {
    CHECK(at == 0u && ph_label_range_sort_key(at, len) == PH_RANGE_SORT_EMPTY);
  }
  // a row that is not listed never passes, whatever is wanted
  CHECK(!ph_pair_holds(NONE64, ph_pair_bound(want, lo), ph_pair_bound(want, hi), NONE64));
  CHECK(!ph_pair_holds_words(NONE64, want, lo, hi, NONE64));
}

static void test_spans() {
  const uint32_t TOP = 0xFFFFFFFEu;
  const std::vector<Rows> worlds = {
      {},            // listed == 0
      {{7u, 40u}},   // listed == 1
      {{TOP, TOP}},  // ... the largest composite there is
      {{0u, 0u}},    // ... the smallest
      // label 0, a label in the middle, two neighbouring labels at and above 2^31 (bit 63 of the composite), the last
      // label; the lower neighbour's largest key is 0xFFFFFFFE and the upper neighbour's smallest is 0: a 32-bit
      // truncation or a signed compare joins or swaps them
      {{0u, 0u}, {0u, 5u}, {0u, 5u}, {0u, TOP},
       {9u, 100u}, {9u, 100u}, {9u, 100u}, {9u, 200u},
       {0x80000000u, 1u}, {0x80000000u, 0x80000000u}, {0x80000000u, TOP},
       {0x80000001u, 0u}, {0x80000001u, 0u}, {0x80000001u, 7u},
       {TOP, 0u}, {TOP, 3u}, {TOP, TOP}},
      // the same keys under two labels: the range alone cannot tell them apart
      {{3u, 10u}, {3u, 20u}, {3u, 30u}, {4u, 10u}, {4u, 20u}, {4u, 30u}},
  };
  for (const Rows &rows : worlds) {
    std::vector<uint32_t> labels = {0u, 1u, NONE, TOP, 0x7FFFFFFFu, 0x80000000u}, bounds = {0u, 1u, NONE, TOP, 0x80000000u};
    for (const auto &r : rows) {
      for (uint32_t d : {0u, 1u}) labels.push_back(r.first - d), labels.push_back(r.first + d);  // carried, and beside
      for (uint32_t d : {0u, 1u}) bounds.push_back(r.second - d), bounds.push_back(r.second + d);
    }
    std::sort(labels.begin(), labels.end()), labels.erase(std::unique(labels.begin(), labels.end()), labels.end());
    std::sort(bounds.begin(), bounds.end()), bounds.erase(std::unique(bounds.begin(), bounds.end()), bounds.end());
    for (uint32_t want : labels)  // want == NONE, labels nobody carries below, between and above those present
      for (uint32_t lo : bounds)
        for (uint32_t hi : bounds) check_span(rows, want, lo, hi);  // lo > hi among them: empty, whatever lies between
  }
  const std::vector<uint64_t> c = column_of(worlds[4]);
  const auto count = [&](uint32_t want, uint32_t lo, uint32_t hi) { return ph_label_range_count(c.data(), c.size(), want, lo, hi); };
  // hi == 0xFFFFFFFF is "no upper end within this label", at a middle label and at the last one
  CHECK(count(9u, 0u, NONE) == 4u && count(9u, 101u, NONE) == 1u && count(0x80000000u, 0u, NONE) == 3u);
  CHECK(count(TOP, 0u, NONE) == 3u && count(TOP, 1u, NONE) == 2u && count(TOP, TOP, NONE) == 1u);
  CHECK(count(0u, 0u, NONE) == 4u && count(0u, 5u, 5u) == 2u);
  // the neighbours: the span of one never reaches into the other
  CHECK(count(0x80000000u, TOP, NONE) == 1u && count(0x80000001u, 0u, 0u) == 2u && count(0x80000001u, 0u, NONE) == 3u);
  // lo > hi although keys lie between; the NONE label; labels nobody carries
  CHECK(count(9u, 200u, 100u) == 0u && count(NONE, 0u, NONE) == 0u);
  CHECK(count(5u, 0u, NONE) == 0u && count(0x7FFFFFFFu, 0u, NONE) == 0u && count(0xFFFFFFFDu, 0u, NONE) == 0u);
  CHECK(ph_label_range_count(nullptr, 0, 9u, 0u, NONE) == 0u);
  CHECK(ph_label_range_upper_bound(c.data(), c.size(), NONE64) == c.size());
  CHECK(ph_label_range_lower_bound(c.data(), c.size(), 0u) == 0u && ph_label_range_lower_bound(c.data(), 0, 5u) == 0u);
  CHECK(ph_label_range_pair(0x80000001u, 7u) == 0x8000000100000007ull && ph_label_range_pair(NONE, NONE) == PH_LABEL_RANGE_PAIR_NONE);
  CHECK(ph_label_range_pair(TOP, NONE) < PH_LABEL_RANGE_PAIR_NONE);  // a listed composite and every bound of a label stay below it
  // the empty spans sort behind every start a column below 2^32 - 1 rows can have
  CHECK(ph_label_range_sort_key(0u, 0u) == PH_RANGE_SORT_EMPTY && ph_label_range_sort_key(123u, 0u) == PH_RANGE_SORT_EMPTY);
  CHECK(ph_label_range_sort_key(0u, 1u) == 0u && ph_label_range_sort_key(0xFFFFFFFDu, 1u) < PH_RANGE_SORT_EMPTY);
}

static void test_route() {
  const uint64_t pair_of[] = {ph_pair_bound(5u, 50u), NONE64, ph_pair_bound(0u, 0u), ph_pair_bound(0xFFFFFFFEu, 0xFFFFFFFEu),
                              ph_pair_bound(0x80000000u, 9u)};
  CHECK(ph_auto_pair_candidate(pair_of, 5, 5u, 50u, 50u, 0u, NONE64) && ph_auto_pair_candidate(pair_of, 5, 5u, 0u, NONE, 0u, NONE64));
  CHECK(ph_auto_pair_candidate(pair_of, 5, 0xFFFFFFFEu, 0u, NONE, 3u, NONE64) && ph_auto_pair_candidate(pair_of, 5, 0u, 0u, 0u, 2u, NONE64));
  CHECK(ph_auto_pair_candidate(pair_of, 5, 0x80000000u, 9u, 9u, 4u, NONE64));
  CHECK(!ph_auto_pair_candidate(pair_of, 5, 0x80000000u, 10u, NONE, 4u, NONE64));
  CHECK(!ph_auto_pair_candidate(pair_of, 5, 6u, 0u, NONE, 0u, NONE64) && !ph_auto_pair_candidate(pair_of, 5, 4u, 0u, NONE, 0u, NONE64));
  CHECK(!ph_auto_pair_candidate(pair_of, 5, 5u, 51u, 50u, 0u, NONE64));     // lo > hi
  CHECK(!ph_auto_pair_candidate(pair_of, 5, NONE, 0u, NONE, 1u, NONE64));   // not listed: in no span, not even NONE's open one
  CHECK(!ph_auto_pair_candidate(pair_of, 5, NONE, NONE, NONE, 1u, NONE64));
  CHECK(!ph_auto_pair_candidate(pair_of, 5, 5u, 0u, NONE, 5u, NONE64));     // v >= n: nothing is read
  CHECK(!ph_auto_pair_candidate(pair_of, 4, 0x80000000u, 0u, NONE, 4u, NONE64) && !ph_auto_pair_candidate(pair_of, 5, 5u, 0u, NONE, NONE, NONE64));
  CHECK(ph_auto_scan_below_label_ranged(0) == PH_AUTO_SCAN_BELOW_LABEL_RANGED && ph_auto_scan_below_label_ranged(5) == 5u);
  CHECK(ph_auto_scan_below_label_ranged(UINT64_MAX) == UINT64_MAX && PH_AUTO_SCAN_BELOW_LABEL_RANGED == PH_AUTO_SCAN_BELOW_RANGED);
}

int main() {
  test_spans();
  test_route();
  std::printf("ALL OK\n");
  return 0;
}
