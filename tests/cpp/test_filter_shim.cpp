// Hnsw::search_many_filtered of include/phnsw.hpp at the edges of its arguments: k 0 (the C call's "whole row of
// number_of_candidates entries", which sizes the wrapper's buffers), k past number_of_candidates, and an allow vector
// shorter than its bitmaps.  Built with g++ and linked to libphnsw.so by tests/test_gpu_filter_shims.py; needs a GPU.
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
    const float s = 0.70710678118f;
    const std::vector<float> data = {1, 0, 0, 0, 1, 0, 0, 0, 1, s, s, 0, 0.5773f, 0.5773f, 0.5773f,
                                     -1, 0, 0, 0, -1, 0, 0, 0, -1, 0, s, s};
    Comparator c(data.data(), 9, 3, OneMinusDot);
    std::vector<VectorId> vs;
    for (uint64_t i = 0; i < 9; i++) vs.push_back(i);
    BuildParameters bp;
    bp.order = 6;
    bp.neighborhood_size = 3;
    bp.zero_layer_neighborhood_size = 6;
    Hnsw hnsw = Hnsw::generate(c, vs, bp);
    const SearchParameters sp = hnsw.build_parameters.optimization.search;
    const uint64_t ef = sp.number_of_candidates;
    const std::vector<const float *> q = {data.data(), data.data() + 3};
    const std::vector<uint32_t> all = {0x1FFu};

    const auto plain = hnsw.search_many_topk(q, sp, ef);
    EXPECT(plain.size() == 2 && plain[0].size() >= 2);
    EXPECT(hnsw.search_many_filtered(q, sp, ef, all) == plain);
    EXPECT(hnsw.search_many_filtered(q, sp, 0, all) == plain);       // k 0: whole rows, ef entries each
    EXPECT(hnsw.search_many_filtered(q, sp, 0, {}) == plain);        // no bitmap and no default: unfiltered
    EXPECT(hnsw.search_many_filtered(q, sp, 0, {0x1FFu, 0x1FFu}, 1) == plain);  // one bitmap per query
    const auto two = hnsw.search_many_filtered(q, sp, 2, all);
    EXPECT(two.size() == 2 && two[0].size() == 2 && two[0][0] == plain[0][0] && two[0][1] == plain[0][1]);

    // one id disallowed, strict: the row without it (k 0 again: the row is read back with the stride it was written in)
    const VectorId gone = plain[0][1].first;
    const auto without = hnsw.search_many_filtered(q, sp, 0, {0x1FFu & ~(1u << gone)}, 0, true);
    EXPECT(without.size() == 2 && without[0].size() == plain[0].size() - 1);
    for (const auto &row : without)
      for (const auto &e : row) EXPECT(e.first != gone);

    EXPECT(throws_invalid([&] { hnsw.search_many_filtered(q, sp, ef + 1, all); }));      // k > number_of_candidates
    EXPECT(throws_invalid([&] { hnsw.search_many_filtered(q, sp, 0, {0x1FFu}, 1); }));   // 2 queries, 1 bitmap
    std::vector<float> wide(33 * 3);  // 33 vectors: a bitmap of 2 words
    for (size_t i = 0; i < wide.size(); i++) wide[i] = (float)((int)(i * 37 % 17) - 8) / 8.0f;
    Comparator c33(wide.data(), 33, 3, OneMinusDot);
    std::vector<VectorId> v33;
    for (uint64_t i = 0; i < 33; i++) v33.push_back(i);
    Hnsw h33 = Hnsw::generate(c33, v33, bp);
    const std::vector<const float *> q33 = {wide.data()};
    EXPECT(throws_invalid([&] { h33.search_many_filtered(q33, sp, 0, {0xFFFFFFFFu}); }));                  // 1 word of 2
    EXPECT(throws_invalid([&] { h33.search_many_filtered(q33, sp, 0, {0xFFFFFFFFu, 0xFFFFFFFFu}, 1); }));  // stride 1 < 2
    EXPECT(h33.search_many_filtered(q33, sp, 0, {0xFFFFFFFFu, 1u}) == h33.search_many_topk(q33, sp, ef));
  } catch (const Error &e) {
    printf("phnsw::Error %d: %s\n", e.code, e.what());
    return 2;
  }
  printf(failures ? "%d FAILURES\n" : "ALL OK%.0d\n", failures);
  return failures ? 1 : 0;
}
