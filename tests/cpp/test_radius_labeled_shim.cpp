// The radius searches by row label and by numeric range of include/phnsw.hpp: their segments against
// search_many_exact_radius called once per query with the equivalent bitmap, against the top-k calls cut at the radius,
// the two-call size negotiation, and what the wrapper and the library refuse.
// Built with g++ and linked to libphnsw.so by tests/test_gpu_radius_labeled.py; needs a GPU.
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
    const uint32_t n = 300;  // more rows under one label than the 64 results per query the first call has room for
    std::vector<float> rows(n * 3);
    for (size_t i = 0; i < rows.size(); i++) rows[i] = (float)((int)(i * 37 % 17) - 8) / 8.0f;
    Comparator c(rows.data(), n, 3, OneMinusDot);
    std::vector<VectorId> vs;
    for (uint64_t i = 0; i < n; i++) vs.push_back(i);
    BuildParameters bp;
    bp.order = 6;
    bp.neighborhood_size = 3;
    bp.zero_layer_neighborhood_size = 6;
    Hnsw hnsw = Hnsw::generate(c, vs, bp);
    std::vector<const float *> q;
    for (int i = 0; i < 7; i++) q.push_back(rows.data() + 3 * i);
    const float inf = std::numeric_limits<float>::infinity();
    const std::vector<float> radius = {inf, 0.5f, 1.0f, 0.0f, inf, -1.0f, 2.0f};
    const uint64_t words = (n + 31) / 32;

    // labels: v % 4, but id 1 carries none; label 0 has 75 rows
    std::vector<uint32_t> lab(n);
    for (uint32_t v = 0; v < n; v++) lab[v] = v % 4;
    lab[1] = Labels::NONE;
    Labels labels(hnsw, lab);
    const std::vector<uint32_t> want = {0, 1, 2, 3, 77, 0, Labels::NONE};
    const auto got = hnsw.search_many_exact_radius_labeled(q, radius, labels, want);
    const auto topk = hnsw.search_many_exact_labeled(q, 1024, labels, want);
    EXPECT(got.size() == 7 && got[0].size() == 75 && got[3].empty() && got[4].empty() && got[5].empty() && got[6].empty());
    for (int i = 0; i < 7; i++) {
      std::vector<uint32_t> bitmap(words, 0u);
      for (uint32_t v = 0; v < n; v++)
        if (lab[v] == want[i] && lab[v] != Labels::NONE) bitmap[v >> 5] |= 1u << (v & 31u);
      const auto one = hnsw.search_many_exact_radius({q[i]}, {radius[i]}, bitmap);
      EXPECT(one.size() == 1 && one[0] == got[i]);
      SearchResult cut;
      for (const auto &e : topk[i])
        if (radius[i] > 0 && e.second < radius[i]) cut.push_back(e);
      EXPECT(cut == got[i]);
      for (size_t j = 1; j < got[i].size(); j++)
        EXPECT(got[i][j - 1].second < got[i][j].second || (got[i][j - 1].second == got[i][j].second && got[i][j - 1].first < got[i][j].first));
    }

    // keys in no id order; id 1 carries no value
    std::vector<uint32_t> keys(n);
    for (uint32_t v = 0; v < n; v++) keys[v] = v * 13 % 50;
    keys[1] = Attribute::NONE;
    Attribute attr(hnsw, keys);
    const std::vector<uint32_t> lo = {0, 10, 20, 0, 30, 0, 49}, hi = {0xFFFFFFFFu, 10, 29, 49, 20, 49, 0xFFFFFFFFu};
    const auto rgot = hnsw.search_many_exact_radius_ranged(q, radius, attr, lo, hi);
    const auto rtopk = hnsw.search_many_exact_ranged(q, 1024, attr, lo, hi);
    EXPECT(rgot.size() == 7 && rgot[0].size() == n - 1 && rgot[3].empty() && rgot[4].empty() && rgot[5].empty());
    for (int i = 0; i < 7; i++) {
      std::vector<uint32_t> bitmap(words, 0u);
      for (uint32_t v = 0; v < n; v++)
        if (v != 1 && keys[v] >= lo[i] && keys[v] <= hi[i]) bitmap[v >> 5] |= 1u << (v & 31u);
      const auto one = hnsw.search_many_exact_radius({q[i]}, {radius[i]}, bitmap);
      EXPECT(one.size() == 1 && one[0] == rgot[i]);
      SearchResult cut;
      for (const auto &e : rtopk[i])
        if (radius[i] > 0 && e.second < radius[i]) cut.push_back(e);
      EXPECT(cut == rgot[i]);
      for (const auto &e : rgot[i]) EXPECT(e.first != 1);
    }

    EXPECT(throws_invalid([&] { hnsw.search_many_exact_radius_labeled(q, {1.0f}, labels, want); }));  // one radius per query
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_radius_labeled(q, radius, labels, {1u, 2u}); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_radius_ranged(q, radius, attr, {5u, 5u}, hi); }));
    Hnsw other = Hnsw::generate(c, vs, bp);  // a handle made for another index is stale
    EXPECT(throws_invalid([&] { other.search_many_exact_radius_labeled(q, radius, labels, want); }));
    EXPECT(throws_invalid([&] { other.search_many_exact_radius_ranged(q, radius, attr, lo, hi); }));
    // the zero-copy forms: the index and cap are looked at first, then the handle
    EXPECT(throws_invalid([&] {
      hnsw.search_exact_radius_labeled_device(labels, nullptr, 0, nullptr, 4, nullptr, nullptr, nullptr, 1ull << 31, nullptr, nullptr,
                                              nullptr, nullptr, nullptr, nullptr);
    }));
    EXPECT(throws_invalid([&] {
      other.search_exact_radius_ranged_device(attr, nullptr, 0, nullptr, 4, nullptr, nullptr, nullptr, nullptr, 8, nullptr, nullptr,
                                              nullptr, nullptr, nullptr, nullptr);
    }));
    hnsw.search_exact_radius_labeled_device(labels, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 8, nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr);  // nq == 0: nothing is enqueued
  } catch (const Error &e) {
    printf("phnsw::Error %d: %s\n", e.code, e.what());
    return 2;
  }
  printf(failures ? "%d FAILURES\n" : "ALL OK%.0d\n", failures);
  return failures ? 1 : 0;
}
