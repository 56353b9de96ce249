// Attribute, attr_key and the searches by range of include/phnsw.hpp: one key per vector against the bitmap calls with
// the equivalent bitmaps laid out per query, the order of the key maps, and what the wrapper and the library refuse.
// Built with g++ and linked to libphnsw.so by tests/test_gpu_ranged_shim.py; needs a GPU.
#include <cstdio>
#include <limits>

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
    // the maps: strictly ascending over sorted ladders, -0.0 and +0.0 one key
    const float inf = std::numeric_limits<float>::infinity(), fmax = std::numeric_limits<float>::max();
    const float fl[] = {-inf, -fmax, -1.0f, -1e-45f, 0.0f, 1e-45f, 1.0f, fmax, inf};
    for (int i = 0; i + 1 < 9; i++) EXPECT(attr_key(fl[i]) < attr_key(fl[i + 1]));
    EXPECT(attr_key(-0.0f) == attr_key(0.0f) && attr_key(0.0f) == 0x80000000u);
    const int32_t il[] = {std::numeric_limits<int32_t>::min(), -1, 0, 1, std::numeric_limits<int32_t>::max()};
    for (int i = 0; i + 1 < 5; i++) EXPECT(attr_key(il[i]) < attr_key(il[i + 1]));
    EXPECT(attr_key(il[0]) == 0u && attr_key(il[4]) == Attribute::NONE && attr_key(7u) == 7u);

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
    // a float column in no id order; id 1 carries no value
    std::vector<float> val(33);
    std::vector<uint32_t> keys(33);
    for (uint32_t v = 0; v < 33; v++) val[v] = (float)((int)(v * 13 % 33) - 16) / 4.0f, keys[v] = attr_key(val[v]);
    keys[1] = Attribute::NONE;
    Attribute attr(hnsw, keys);
    EXPECT(attr.listed() == 32 && attr.key_range().first == attr_key(-4.0f) && attr.key_range().second == attr_key(4.0f));
    const float lof[] = {-4.0f, 0.0f, 1.0f, -0.3f, 3.9f, -100.0f, 0.25f};
    const float hif[] = {4.0f, 0.0f, -1.0f, 0.3f, 100.0f, -4.0f, 2.0f};
    std::vector<uint32_t> lo, hi, per_query;  // per_query: one bitmap per query, two words apart
    for (int i = 0; i < 7; i++) {
      lo.push_back(attr_key(lof[i])), hi.push_back(attr_key(hif[i]));
      uint32_t words[2] = {0u, 0u};
      for (uint32_t v = 0; v < 33; v++)
        if (v != 1 && val[v] >= lof[i] && val[v] <= hif[i]) words[v >> 5] |= 1u << (v & 31u);
      per_query.push_back(words[0]);
      per_query.push_back(words[1]);
    }
    for (uint64_t k : {1u, 5u, 40u}) {
      const auto got = hnsw.search_many_exact_ranged(q, k, attr, lo, hi);
      EXPECT(got == hnsw.search_many_exact_filtered(q, k, per_query, 2));
      EXPECT(got.size() == 7 && got[2].empty() && got[1].size() == 1 && got[5].size() == 1);
      EXPECT(got[0].size() == (k < 32 ? k : 32));
      for (const auto &e : got[0]) EXPECT(e.first != 1);
    }
    SearchParameters sp;
    sp.number_of_candidates = 16;
    sp.upper_layer_candidate_count = 16;
    sp.probe_depth = 2;
    for (bool strict : {false, true})
      for (uint64_t k : {0u, 4u})
        EXPECT(hnsw.search_many_ranged(q, sp, k, attr, lo, hi, strict) == hnsw.search_many_filtered(q, sp, k, per_query, 2, strict));
    std::vector<uint32_t> routes;
    const auto routed = hnsw.search_many_ranged_auto(q, sp, 5, attr, lo, hi, 3, &routes);
    EXPECT(routed == hnsw.search_many_filtered_auto(q, sp, 5, per_query, 2, 3));
    EXPECT(routes.size() == 7 && routed[0].size() == 5 && routed[2].empty());
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_ranged(q, 0, attr, lo, hi); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_ranged(q, 1025, attr, lo, hi); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_ranged(q, 5, attr, {5u, 5u}, hi); }));  // one bound per query
    EXPECT(throws_invalid([&] { hnsw.search_many_ranged_auto(q, sp, 17, attr, lo, hi); }));
    EXPECT(throws_invalid([&] { Attribute short_column(hnsw, std::vector<uint32_t>(32, 5u)); }));  // n is the store's
    Hnsw other = Hnsw::generate(c, vs, bp);  // a handle made for another index is stale
    EXPECT(throws_invalid([&] { other.search_many_exact_ranged(q, 5, attr, lo, hi); }));
    EXPECT(throws_invalid([&] { other.search_many_ranged(q, sp, 0, attr, lo, hi); }));
    Attribute moved(std::move(attr));
    EXPECT(hnsw.search_many_exact_ranged(q, 5, moved, lo, hi) == hnsw.search_many_exact_filtered(q, 5, per_query, 2));
  } catch (const Error &e) {
    printf("phnsw::Error %d: %s\n", e.code, e.what());
    return 2;
  }
  printf(failures ? "%d FAILURES\n" : "ALL OK%.0d\n", failures);
  return failures ? 1 : 0;
}
