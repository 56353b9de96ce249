// Hnsw::search_many_labeled and Hnsw::search_many_labeled_auto of include/phnsw.hpp: the graph walk and the routed call
// by row label against search_many_filtered and search_many_filtered_auto with the equivalent bitmaps laid out per query,
// and what the wrappers and the library refuse.  Built with g++ and linked to libphnsw.so by
// tests/test_gpu_labeled_walk_shim.py; needs a GPU.
#include <cstdio>

#include "phnsw.hpp"

using namespace phnsw;

static int failures = 0;
#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                            \
    }                                                        \
  } while (0)

template <class F>
static bool throws_invalid(F f) {
  try {
    f();
  } catch (const Error &e) {
    return e.code == PHNSW_E_INVALID;
  }
  return false;
}

int main() {
  try {
    const uint32_t n = 330, dim = 8;
    std::vector<float> rows(n * dim);
    for (size_t i = 0; i < rows.size(); i++) rows[i] = (float)((int)(i * 37 % 23) - 11) / 8.0f + (float)(i % 7) / 64.0f;
    Comparator c(rows.data(), n, dim, OneMinusDot);
    std::vector<VectorId> vs;
    for (uint64_t i = 0; i < n; i++) vs.push_back(i);
    BuildParameters bp;
    bp.order = 6;
    bp.neighborhood_size = 6;
    bp.zero_layer_neighborhood_size = 12;
    Hnsw hnsw = Hnsw::generate(c, vs, bp);
    std::vector<const float *> q;
    for (int i = 0; i < 9; i++) q.push_back(rows.data() + dim * (i * 31));
    // label 70000 on every second id, 0xFFFFFFFE on the last id alone, id 1 unlisted, 5 on the rest
    std::vector<uint32_t> lab(n);
    for (uint32_t v = 0; v < n; v++) lab[v] = v == n - 1 ? 0xFFFFFFFEu : (v == 1 ? Labels::NONE : (v % 2 == 0 ? 70000u : 5u));
    Labels labels(hnsw, lab);
    const std::vector<uint32_t> want = {70000u, 0xFFFFFFFEu, 999u, 5u, 70000u, Labels::NONE, 5u, 70000u, 5u};
    const uint32_t words = (n + 31) / 32;
    std::vector<uint32_t> per_query;  // one bitmap per query, `words` apart
    for (uint32_t w : want) {
      std::vector<uint32_t> bm(words, 0u);
      for (uint32_t v = 0; v < n; v++)
        if (w != Labels::NONE && lab[v] == w) bm[v >> 5] |= 1u << (v & 31u);
      per_query.insert(per_query.end(), bm.begin(), bm.end());
    }
    SearchParameters sp;
    sp.number_of_candidates = 32;
    sp.upper_layer_candidate_count = 16;
    sp.probe_depth = 2;
    for (bool strict : {false, true}) {
      for (uint64_t k : {0u, 5u, 32u}) {
        const auto got = hnsw.search_many_labeled(q, sp, labels, want, strict, k);
        EXPECT(got == hnsw.search_many_filtered(q, sp, k, per_query, words, strict));
        EXPECT(got.size() == 9);
        if (strict) {
          EXPECT(got[2].empty() && got[5].empty());
          for (const auto &e : got[0]) EXPECT(e.first % 2 == 0 && e.first != n - 1);
          for (const auto &e : got[3]) EXPECT(e.first % 2 == 1 && e.first != 1);
        }
      }
    }
    for (uint64_t scan_below : {1u, 100u, 1000u}) {
      std::vector<uint32_t> routes, routes_bitmap;
      const auto got = hnsw.search_many_labeled_auto(q, sp, 5, labels, want, scan_below, &routes);
      EXPECT(got == hnsw.search_many_filtered_auto(q, sp, 5, per_query, words, scan_below, &routes_bitmap));
      EXPECT(routes == routes_bitmap && routes.size() == 9);
      EXPECT(got[0].size() == 5 && got[3].size() == 5 && got[1].size() == 1 && got[1][0].first == n - 1);
      EXPECT(got[2].empty() && got[5].empty());
      if (scan_below == 1000u)
        for (uint32_t r : routes) EXPECT(r == PHNSW_ROUTE_SCAN);
      if (scan_below == 1u) EXPECT(routes[0] != PHNSW_ROUTE_SCAN && routes[3] != PHNSW_ROUTE_SCAN && routes[1] == PHNSW_ROUTE_SCAN);
    }
    EXPECT(throws_invalid([&] { hnsw.search_many_labeled(q, sp, labels, want, false, 33); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_labeled(q, sp, labels, {5u, 5u}); }));  // one label per query
    EXPECT(throws_invalid([&] { hnsw.search_many_labeled_auto(q, sp, 0, labels, want); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_labeled_auto(q, sp, 33, labels, want); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_labeled_auto(q, sp, 5, labels, {5u}); }));
    Hnsw other = Hnsw::generate(c, vs, bp);  // a handle made for another index is stale
    EXPECT(throws_invalid([&] { other.search_many_labeled(q, sp, labels, want); }));
    EXPECT(throws_invalid([&] { other.search_many_labeled_auto(q, sp, 5, labels, want); }));
  } catch (const Error &e) {
    printf("phnsw::Error %d: %s\n", e.code, e.what());
    return 2;
  }
  printf(failures ? "%d FAILURES\n" : "ALL OK%.0d\n", failures);
  return failures ? 1 : 0;
}
