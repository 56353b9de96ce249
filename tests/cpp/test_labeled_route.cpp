// Stand-alone host check of the pure functions the calls by row label added (parallel_hnsw_amd/csrc/label_plan.h,
// filter_route.h): compiled with -fsanitize=address,undefined and run without a GPU (tests/test_labeled_route_cpp.py).
// The subset seeding of the lookup positions with a host model of the lookup over arrays of exactly the sizes a call
// allocates (an index out of bounds is a sanitizer report), the labeled scan_below default, and the candidate test of
// exclude[q] on a label column against the bitmap form of the same statement.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/filter_route.h"
#include "../../parallel_hnsw_amd/csrc/label_plan.h"

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

static const uint32_t NONE = 0xFFFFFFFFu;  // PHNSW_LABEL_NONE

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// the lookup kernel on the host: slot and iota by POSITION, the query from the seed
static void lookup(const std::vector<uint32_t> &values, const std::vector<uint32_t> &want, const uint32_t *list, uint32_t npos,
                   std::vector<uint32_t> *slot, std::vector<uint32_t> *iota) {
  slot->assign(npos, 0u), iota->assign(npos, 0u);
  for (uint32_t p = 0; p < npos; p++) {
    const uint32_t q = ph_label_seed(list, p);
    CHECK(q < want.size());
    (*slot)[p] = ph_label_slot(values.data(), values.size(), want[q], NONE);
    (*iota)[p] = q;
  }
}

int main() {
  // ---- the seed: identity without a list, the list's entry with one
  CHECK(ph_label_seed(nullptr, 0u) == 0u && ph_label_seed(nullptr, 0xFFFFFFFEu) == 0xFFFFFFFEu);
  {
    const std::vector<uint32_t> list = {7u, 0u, 0xFFFFFFF0u};
    for (uint32_t p = 0; p < 3u; p++) CHECK(ph_label_seed(list.data(), p) == list[p]);
  }
  // ---- a subset call looks up exactly the queries of its list, whatever their order, and nothing else
  for (int round = 0; round < 200; round++) {
    const uint32_t nq = 1u + (uint32_t)(rnd() % 300u);
    std::vector<uint32_t> values;
    for (uint32_t v = 0; v < 1u + rnd() % 20u; v++) values.push_back((uint32_t)(rnd() % 50u) * 3u);
    values.push_back(0xFFFFFFFEu);
    std::sort(values.begin(), values.end());
    values.erase(std::unique(values.begin(), values.end()), values.end());
    std::vector<uint32_t> want(nq);
    for (uint32_t &w : want) w = rnd() % 5u == 0u ? NONE : (rnd() % 3u == 0u ? 1u : values[rnd() % values.size()]);
    std::vector<uint32_t> slot, iota, full_slot, full_iota;
    lookup(values, want, nullptr, nq, &full_slot, &full_iota);
    for (uint32_t q = 0; q < nq; q++) {
      CHECK(full_iota[q] == q);
      const bool found = full_slot[q] != PH_LABEL_SLOT_NONE;
      CHECK(found == (want[q] != NONE && std::binary_search(values.begin(), values.end(), want[q])));
      if (found) CHECK(values[full_slot[q]] == want[q]);
    }
    std::vector<uint32_t> list;  // ascending, as the route kernel writes it, then with a tail appended out of order
    for (uint32_t q = 0; q < nq; q++)
      if (rnd() % 3u == 0u) list.push_back(q);
    std::vector<uint32_t> tail;
    for (uint32_t q = 0; q < nq; q++)
      if (!std::binary_search(list.begin(), list.end(), q) && rnd() % 4u == 0u) tail.push_back(q);
    std::reverse(tail.begin(), tail.end());
    list.insert(list.end(), tail.begin(), tail.end());
    CHECK(list.size() <= nq);  // what the scan list of a routed call holds: nq entries hold it
    lookup(values, want, list.data(), (uint32_t)list.size(), &slot, &iota);
    CHECK(slot.size() == list.size());
    for (size_t p = 0; p < list.size(); p++) CHECK(iota[p] == list[p] && slot[p] == full_slot[list[p]]);
  }
  // ---- the default threshold of a call by label: the measured crossover (profiles/labeled_walk/README.md)
  CHECK(PH_AUTO_SCAN_BELOW_LABELED == 20000u);
  CHECK(ph_auto_scan_below_labeled(0u) == PH_AUTO_SCAN_BELOW_LABELED);
  CHECK(ph_auto_scan_below(0u, true) == PH_AUTO_SCAN_BELOW_PER_QUERY);  // the bitmap calls keep theirs
  CHECK(ph_auto_scan_below_labeled(1u) == 1u && ph_auto_scan_below_labeled(UINT64_MAX) == UINT64_MAX);
  // ---- exclude[q] is a candidate iff it is listed under want[q]: the column against the bitmap of that label
  for (int round = 0; round < 200; round++) {
    const uint32_t n = 1u + (uint32_t)(rnd() % 200u);
    std::vector<uint32_t> label_of(n);
    for (uint32_t &l : label_of) l = rnd() % 4u == 0u ? NONE : (uint32_t)(rnd() % 4u) * 0x55555555u;  // 0xFFFFFFFF is NONE
    for (uint32_t want : {0u, 0x55555555u, 0xAAAAAAAAu, NONE, 9u}) {
      std::vector<uint32_t> bitmap((n + 31u) / 32u, 0u);
      for (uint32_t v = 0; v < n; v++)
        if (want != NONE && label_of[v] == want) bitmap[v >> 5] |= 1u << (v & 31u);
      for (uint32_t v : {0u, n - 1u, n, n + 31u, 0xFFFFFFFFu, (uint32_t)(rnd() % n)}) {
        const bool by_bitmap = v < n && ((bitmap[v >> 5] >> (v & 31u)) & 1u);
        CHECK(ph_auto_label_candidate(label_of.data(), n, want, v, NONE) == by_bitmap);
      }
    }
  }
  std::printf("ALL OK\n");
  return 0;
}
