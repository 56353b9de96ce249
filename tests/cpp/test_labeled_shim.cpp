// Labels and Hnsw::search_many_exact_labeled of include/phnsw.hpp: one label per vector against
// search_many_exact_filtered with the equivalent bitmaps laid out per query, and what the wrapper and the library
// refuse.  Built with g++ and linked to libphnsw.so by tests/test_gpu_labeled_shim.py; needs a GPU.
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
    // label 70000 on every second id, 0xFFFFFFFE on the last id alone, id 1 unlisted, 5 on the rest
    std::vector<uint32_t> lab(33);
    for (uint32_t v = 0; v < 33; v++) lab[v] = v == 32 ? 0xFFFFFFFEu : (v == 1 ? Labels::NONE : (v % 2 == 0 ? 70000u : 5u));
    Labels labels(hnsw, lab);
    EXPECT(labels.label_count() == 3 && labels.listed() == 32 && labels.longest() == 16);
    const std::vector<uint32_t> want = {70000u, 0xFFFFFFFEu, 999u, 5u, 70000u, Labels::NONE, 5u};
    std::vector<uint32_t> per_query;  // what search_many_exact_filtered takes: one bitmap per query, two words apart
    for (uint32_t w : want) {
      uint32_t words[2] = {0u, 0u};
      for (uint32_t v = 0; v < 33; v++)
        if (w != Labels::NONE && lab[v] == w) words[v >> 5] |= 1u << (v & 31u);
      per_query.push_back(words[0]);
      per_query.push_back(words[1]);
    }
    for (uint64_t k : {1u, 5u, 40u}) {
      const auto got = hnsw.search_many_exact_labeled(q, k, labels, want);
      EXPECT(got == hnsw.search_many_exact_filtered(q, k, per_query, 2));
      EXPECT(got.size() == 7 && got[2].empty() && got[5].empty() && got[1].size() == 1 && got[1][0].first == 32);
      EXPECT(got[0].size() == (k < 16 ? k : 16) && got[3].size() == (k < 15 ? k : 15));
      for (const auto &e : got[0]) EXPECT(e.first % 2 == 0 && e.first != 32);
      for (const auto &e : got[3]) EXPECT(e.first % 2 == 1 && e.first != 1);
    }
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_labeled(q, 0, labels, want); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_labeled(q, 1025, labels, want); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_labeled(q, 5, labels, {5u, 5u}); }));  // one label per query
    EXPECT(throws_invalid([&] { Labels short_column(hnsw, std::vector<uint32_t>(32, 5u)); }));  // n is the store's
    Hnsw other = Hnsw::generate(c, vs, bp);  // a handle made for another index is stale
    EXPECT(throws_invalid([&] { other.search_many_exact_labeled(q, 5, labels, want); }));
    Labels moved(std::move(labels));
    EXPECT(hnsw.search_many_exact_labeled(q, 5, moved, want) == hnsw.search_many_exact_filtered(q, 5, per_query, 2));
  } catch (const Error &e) {
    printf("phnsw::Error %d: %s\n", e.code, e.what());
    return 2;
  }
  printf(failures ? "%d FAILURES\n" : "ALL OK%.0d\n", failures);
  return failures ? 1 : 0;
}
