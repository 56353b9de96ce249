// The searches by a set of labels and a numeric range of include/phnsw.hpp: the sets of a batch and one range per query
// against the C ABI's rows and against the bitmap calls with the equivalent bitmaps laid out per query, the one-label
// sets against the calls by label and range, and what the wrapper and the library refuse.  Built with g++ and linked to
// libphnsw.so by tests/test_gpu_labelset_ranged_shim.py; needs a GPU.
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

// the rows of a C ABI call, cut to their lengths as the wrapper cuts them
static std::vector<SearchResult> rows_of(const std::vector<uint64_t> &ids, const std::vector<float> &d, const std::vector<uint64_t> &len,
                                         uint64_t row) {
  std::vector<SearchResult> out(len.size());
  for (size_t i = 0; i < len.size(); i++)
    for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * row + j], d[i * row + j]});
  return out;
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
    std::vector<float> flat;
    for (int i = 0; i < 7; i++) q.push_back(wide.data() + 3 * i), flat.insert(flat.end(), wide.data() + 3 * i, wide.data() + 3 * i + 3);
    // three labels (one at 2^31, one the largest) over a float column in no id order; id 1 carries no value, id 2 no label
    const uint32_t LBL[3] = {4u, 0x80000000u, 0xFFFFFFFEu}, NONE = LabeledAttribute::NONE;
    std::vector<float> val(33);
    std::vector<uint32_t> keys(33), labels(33);
    for (uint32_t v = 0; v < 33; v++) val[v] = (float)((int)(v * 13 % 33) - 16) / 4.0f, keys[v] = attr_key(val[v]), labels[v] = LBL[v % 3];
    keys[1] = NONE;
    labels[2] = NONE;
    LabeledAttribute attr(hnsw, labels, keys);
    // the sets: two labels, one twice and another, all three and NONE, one label, none, a label nobody carries, two again
    const std::vector<std::vector<uint32_t>> want = {{LBL[0], LBL[1]}, {LBL[1], LBL[1], LBL[2]}, {LBL[2], NONE, LBL[0], LBL[1]}, {LBL[0]},
                                                     {},               {5u, NONE},               {LBL[2], LBL[0]}};
    const float lof[] = {-4.0f, -4.0f, 1.0f, -0.3f, -4.0f, -4.0f, 0.25f};
    const float hif[] = {4.0f, 0.0f, -1.0f, 0.3f, 4.0f, 4.0f, 2.0f};
    std::vector<uint32_t> lo, hi, per_query, first = {0u}, values;  // per_query: one bitmap per query, two words apart
    for (int i = 0; i < 7; i++) {
      lo.push_back(attr_key(lof[i])), hi.push_back(attr_key(hif[i]));
      values.insert(values.end(), want[i].begin(), want[i].end());
      first.push_back((uint32_t)values.size());
      uint32_t words[2] = {0u, 0u};
      for (uint32_t v = 0; v < 33; v++) {
        bool in = false;
        for (uint32_t w : want[i]) in |= w != NONE && labels[v] == w;
        if (v != 1 && v != 2 && in && val[v] >= lof[i] && val[v] <= hif[i]) words[v >> 5] |= 1u << (v & 31u);
      }
      per_query.push_back(words[0]);
      per_query.push_back(words[1]);
    }
    hi[0] = NONE;  // no upper end within each label: what 4.0, the largest value, gives
    // one exact call: the C ABI's rows, and the bitmap call's
    for (uint64_t k : {1u, 5u, 40u}) {
      const auto got = hnsw.search_many_exact_labelset_ranged(q, k, attr, want, lo, hi);
      std::vector<uint64_t> ids(7 * k), len(7);
      std::vector<float> d(7 * k);
      check(phnsw_search_exact_labelset_ranged(hnsw.handle(), attr.handle(), flat.data(), nullptr, 7, nullptr, first.data(), values.data(),
                                               lo.data(), hi.data(), k, ids.data(), d.data(), len.data()));
      EXPECT(got == rows_of(ids, d, len, k));
      EXPECT(got == hnsw.search_many_exact_filtered(q, k, per_query, 2));
      EXPECT(got.size() == 7 && got[2].empty() && got[4].empty() && got[5].empty());
      EXPECT(got[0].size() == (k < 21 ? k : 21));  // labels 4 and 2^31: 11 + 11 ids, one of them (id 1) without a value
      for (const auto &e : got[0]) EXPECT(e.first % 3 != 2);
    }
    SearchParameters sp;
    sp.number_of_candidates = 16;
    sp.upper_layer_candidate_count = 16;
    sp.probe_depth = 2;
    for (bool strict : {false, true})
      for (uint64_t k : {0u, 4u})
        EXPECT(hnsw.search_many_labelset_ranged(q, sp, k, attr, want, lo, hi, strict) ==
               hnsw.search_many_filtered(q, sp, k, per_query, 2, strict));
    // one routed call: the C ABI's rows and routes, and the routed bitmap call's
    std::vector<uint32_t> routes, croutes(7);
    const auto routed = hnsw.search_many_labelset_ranged_auto(q, sp, 5, attr, want, lo, hi, 3, &routes);
    {
      std::vector<uint64_t> ids(7 * 5), len(7);
      std::vector<float> d(7 * 5);
      check(phnsw_search_labelset_ranged_auto(hnsw.handle(), attr.handle(), flat.data(), nullptr, 7, &sp, nullptr, first.data(),
                                              values.data(), lo.data(), hi.data(), 5, 3, ids.data(), d.data(), len.data(), croutes.data()));
      EXPECT(routed == rows_of(ids, d, len, 5) && routes == croutes);
    }
    EXPECT(routed == hnsw.search_many_filtered_auto(q, sp, 5, per_query, 2, 3));
    EXPECT(routes.size() == 7 && routed[0].size() == 5 && routed[2].empty() && routed[4].empty());
    // sets of one label are the calls by label and range
    {
      const std::vector<uint32_t> one = {LBL[0], LBL[1], LBL[2], LBL[0], NONE, 5u, LBL[2]};
      std::vector<std::vector<uint32_t>> sets;
      for (uint32_t w : one) sets.push_back({w});
      EXPECT(hnsw.search_many_exact_labelset_ranged(q, 5, attr, sets, lo, hi) == hnsw.search_many_exact_label_ranged(q, 5, attr, one, lo, hi));
      EXPECT(hnsw.search_many_labelset_ranged(q, sp, 0, attr, sets, lo, hi) == hnsw.search_many_label_ranged(q, sp, 0, attr, one, lo, hi));
    }
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_labelset_ranged(q, 0, attr, want, lo, hi); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_labelset_ranged(q, 1025, attr, want, lo, hi); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_labelset_ranged(q, 5, attr, want, {5u, 5u}, hi); }));  // one bound per query
    EXPECT(throws_invalid([&] { hnsw.search_many_exact_labelset_ranged(q, 5, attr, {{4u}}, lo, hi); }));      // one set per query
    EXPECT(throws_invalid([&] { hnsw.search_many_labelset_ranged(q, sp, 17, attr, want, lo, hi); }));
    EXPECT(throws_invalid([&] { hnsw.search_many_labelset_ranged_auto(q, sp, 17, attr, want, lo, hi); }));
    {  // the library refuses offsets that run backwards, naming the query
      std::vector<uint32_t> back = first;
      back[3] = back[2] - 1;
      std::vector<uint64_t> ids(7 * 5), len(7);
      std::vector<float> d(7 * 5);
      EXPECT(phnsw_search_exact_labelset_ranged(hnsw.handle(), attr.handle(), flat.data(), nullptr, 7, nullptr, back.data(), values.data(),
                                                lo.data(), hi.data(), 5, ids.data(), d.data(), len.data()) == PHNSW_E_INVALID);
      EXPECT(std::string(phnsw_last_error()).find("query 2") != std::string::npos);
    }
    Hnsw other = Hnsw::generate(c, vs, bp);  // a handle made for another index is stale
    EXPECT(throws_invalid([&] { other.search_many_exact_labelset_ranged(q, 5, attr, want, lo, hi); }));
    EXPECT(throws_invalid([&] { other.search_many_labelset_ranged(q, sp, 0, attr, want, lo, hi); }));
    EXPECT(throws_invalid([&] { other.search_many_labelset_ranged_auto(q, sp, 5, attr, want, lo, hi); }));
  } catch (const Error &e) {
    printf("phnsw::Error %d: %s\n", e.code, e.what());
    return 2;
  }
  printf(failures ? "%d FAILURES\n" : "ALL OK%.0d\n", failures);
  return failures ? 1 : 0;
}
