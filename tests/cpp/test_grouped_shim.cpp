// Hnsw::search_many_exact_grouped of include/phnsw.hpp: a table of bitmaps and a selector per query against
// search_many_exact_filtered with the same bitmaps laid out per query, and what the wrapper refuses before the library
// is called.  Built with g++ and linked to libphnsw.so by tests/test_gpu_grouped_shim.py; needs a GPU.
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
    std::vector<float> wide(33 * 3);  // 33 vectors: a bitmap of 2 words, one valid bit in the second
    for (size_t i = 0; i < wide.size(); i++) wide[i] = (float)((int)(i * 37 % 17) - 8) / 8.0f;
    Comparator c(wide.data(), 33, 3, OneMinusDot);
    std::vector<VectorId> vs;
    for (uint64_t i = 0; i < 33; i++) vs.push_back(i);
    BuildParameters bp;
    bp.order = 6;
    bp.neighborhood_size = 3;
    bp.zero_layer_neighborhood_size = 6;
    Hnsw hnsw = Hnsw::generate(c, vs, bp);
    std::vector<const float *> q;
    for (int i = 0; i < 7; i++) q.push_back(wide.data() + 3 * i);
    // three bitmaps three words apart (the third word of each is padding, all ones): every second id, the last id
    // alone, none
    const std::vector<uint32_t> table = {0x55555555u, 1u, 0xFFFFFFFFu, 0u, 1u, 0xFFFFFFFFu, 0u, 0u, 0xFFFFFFFFu};
    const std::vector<uint32_t> of = {0, 1, 2, (uint32_t)PHNSW_FILTER_ALL, 0, 1, 0};
    const std::vector<uint32_t> all = {0xFFFFFFFFu, 1u};
    std::vector<uint32_t> per_query;  // what search_many_exact_filtered takes: one bitmap per query, two words apart
    for (uint32_t f : of)
      for (int w = 0; w < 2; w++) per_query.push_back(f == (uint32_t)PHNSW_FILTER_ALL ? all[w] : table[f * 3 + w]);
    for (uint64_t k : {1u, 5u, 40u}) {
      const auto got = hnsw.search_many_exact_grouped(q, k, table, 3, of);
      EXPECT(got == hnsw.search_many_exact_filtered(q, k, per_query, 2));
      EXPECT(got.size() == 7 && got[2].empty() && got[1].size() == 1 && got[1][0].first == 32);
      EXPECT(got[3].size() == (k < 33 ? k : 33) && got[0].size() == (k < 17 ? k : 17));
      for (const auto &e : got[0]) EXPECT(e.first % 2 == 0);
    }
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_grouped(q, 0, table, 3, of); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_grouped(q, 1025, table, 3, of); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_grouped(q, 5, table, 0, of); }));   // the stride is required
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_grouped(q, 5, table, 1, of); }));   // ... and at least a bitmap
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_grouped(q, 5, {}, 2, of); }));      // an empty table
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_grouped(q, 5, table, 2, of); }));   // 9 words: no whole bitmaps
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_grouped(q, 5, table, 3, {0, 1}); }));  // one selector per query
    std::vector<uint32_t> bad = of;
    bad[4] = 3;  // == nfilters
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_grouped(q, 5, table, 3, bad); }));
    bad[4] = 0xFFFFFFFEu;
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_grouped(q, 5, table, 3, bad); }));
  } catch (const Error &e) {
    printf("phnsw::Error %d: %s\n", e.code, e.what());
    return 2;
  }
  printf(failures ? "%d FAILURES\n" : "ALL OK%.0d\n", failures);
  return failures ? 1 : 0;
}
