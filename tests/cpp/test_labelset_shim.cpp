// Hnsw::search_many_exact_labelset of include/phnsw.hpp: a set of labels per query against the rows the Python side
// computed for the same vectors, labels and sets (argv[1]: per query a line "len id bits id bits ..."), against
// search_many_exact_filtered with the union bitmaps laid out per query, and what the wrapper and the library refuse.
// Built with g++ and linked to libphnsw.so by tests/test_gpu_labelset_shim.py; needs a GPU.
#include <cstdio>
#include <cstring>

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

int main(int argc, char **argv) {
  if (argc != 2) {
    printf("usage: test_labelset_shim ROWS_FILE\n");
    return 2;
  }
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
    const std::vector<std::vector<uint32_t>> want = {{70000u, 5u}, {0xFFFFFFFEu}, {999u, Labels::NONE}, {5u, 5u, 0xFFFFFFFEu},
                                                     {}, {5u, 999u, 70000u, 0xFFFFFFFEu}, {70000u}};
    std::vector<uint32_t> per_query;  // what search_many_exact_filtered takes: one bitmap per query, two words apart
    for (const auto &s : want) {
      uint32_t words[2] = {0u, 0u};
      for (uint32_t w : s)
        for (uint32_t v = 0; v < 33; v++)
          if (w != Labels::NONE && lab[v] == w) words[v >> 5] |= 1u << (v & 31u);
      per_query.push_back(words[0]);
      per_query.push_back(words[1]);
    }
    const uint64_t K = 40;
    const auto got = hnsw.search_many_exact_labelset(q, K, labels, want);
    EXPECT(got == hnsw.search_many_exact_filtered(q, K, per_query, 2));
    EXPECT(got.size() == 7 && got[0].size() == 31 && got[1].size() == 1 && got[2].empty() && got[3].size() == 16 &&
           got[4].empty() && got[5].size() == 32 && got[6].size() == 16);
    // the rows of the Python side
    FILE *f = fopen(argv[1], "r");
    EXPECT(f != nullptr);
    for (size_t i = 0; f && i < got.size(); i++) {
      unsigned long long len = 0;
      EXPECT(fscanf(f, "%llu", &len) == 1 && len == got[i].size());
      for (size_t j = 0; j < len; j++) {
        unsigned long long id = 0;
        unsigned int bits = 0, mine = 0;
        EXPECT(fscanf(f, "%llu %u", &id, &bits) == 2);
        if (j < got[i].size()) {
          std::memcpy(&mine, &got[i][j].second, 4);
          EXPECT(id == got[i][j].first && bits == mine);
        }
      }
    }
    if (f) fclose(f);
    for (uint64_t k : {1u, 5u}) EXPECT(hnsw.search_many_exact_labelset(q, k, labels, want) == hnsw.search_many_exact_filtered(q, k, per_query, 2));
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_labelset(q, 0, labels, want); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_labelset(q, 1025, labels, want); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_labelset(q, 5, labels, {{5u}, {5u}}); }));  // one set per query
    Hnsw other = Hnsw::generate(c, vs, bp);  // a handle made for another index is stale
    EXPECT(throws_invalid([&] { other.search_many_exact_labelset(q, 5, labels, want); }));
  } catch (const Error &e) {
    printf("phnsw::Error %d: %s\n", e.code, e.what());
    return 2;
  }
  printf(failures ? "%d FAILURES\n" : "ALL OK%.0d\n", failures);
  return failures ? 1 : 0;
}
