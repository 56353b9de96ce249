// Stand-alone host check of the integer rules behind the search by a SET of row labels and a numeric range
// (parallel_hnsw_amd/csrc/labelset_range_plan.h, the header the launcher and the kernels include, on top of
// labelset_plan.h and label_range_plan.h; ph_pairset_holds and ph_auto_pairset_candidate of filter_route.h): compiled with
// -fsanitize=address,undefined and run without a GPU (tests/test_labelset_range_plan_cpp.py).  On random columns and
// random batches, against brute force: the span per pair, the duplicate rule on the span-start order (the kept
// positions of a query are exactly its distinct labels with non-empty spans), the count against the popcount of the
// mask, the walk's predicate against the mask bit of every (row, query), and claims over offsets that overlap and run
// backwards.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <set>
#include <utility>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/filter_route.h"
#include "../../parallel_hnsw_amd/csrc/labelset_range_plan.h"

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

static const uint32_t NONE = 0xFFFFFFFFu;
static const uint64_t NONE64 = 0xFFFFFFFFFFFFFFFFull;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below) {  // xorshift: the same sequence everywhere
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 20) % below);
}

// labels that matter: 0, neighbours at 3 | 4 and across 2^31, the last one; 5 is carried by nobody
static const uint32_t CARRIED[] = {0u, 3u, 4u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu};
static const uint32_t WANTED[] = {0u, 3u, 4u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 5u, NONE};
static const uint32_t BOUNDS[] = {0u, 1u, 7u, 40u, 41u, 100u, 0x80000000u, 0xFFFFFFFEu, NONE};

struct World {
  std::vector<uint32_t> labels, keys;  // per row; NONE = no label, no value
  std::vector<uint64_t> pair_of;       // per row: the composite, NONE64 where the row is not listed
  std::vector<uint64_t> spairs;        // the listed composites, ascending
};

static World make_world(uint32_t n) {
  World w;
  for (uint32_t v = 0; v < n; v++) {
    const uint32_t lbl = rnd(9) == 0 ? NONE : CARRIED[rnd(7)];
    const uint32_t r = rnd(12);
    const uint32_t key = r == 0 ? NONE : (r == 1 ? 0xFFFFFFFEu : (r == 2 ? 0u : (r == 3 ? 0x80000000u : rnd(120))));
    w.labels.push_back(lbl), w.keys.push_back(key);
    const bool listed = lbl != NONE && key != NONE;
    w.pair_of.push_back(listed ? (uint64_t)lbl * 4294967296ull + key : NONE64);  // label in the top word, written here
    if (listed) w.spairs.push_back(w.pair_of.back());
  }
  std::sort(w.spairs.begin(), w.spairs.end());
  w.spairs.shrink_to_fit();  // a read past either end is the sanitizer's
  return w;
}

// the mask bit of (row v, a set, a range) from the contract: listed, label in the set, key inside
static bool mask_bit(const World &w, uint32_t v, const std::vector<uint32_t> &set, uint32_t lo, uint32_t hi) {
  if (w.labels[v] == NONE || w.keys[v] == NONE) return false;
  bool in = false;
  for (uint32_t x : set) in |= x != NONE && x == w.labels[v];
  return in && w.keys[v] >= lo && w.keys[v] <= hi;
}

// one batch with honest offsets: the whole pipeline of the scan on the host, position by position
static void check_batch(const World &w, uint32_t nq) {
  const uint64_t *sp = w.spairs.empty() ? nullptr : w.spairs.data();
  const uint64_t listed = w.spairs.size();
  std::vector<std::vector<uint32_t>> sets(nq);
  std::vector<uint32_t> first = {0u}, values, lo, hi;
  for (uint32_t q = 0; q < nq; q++) {
    const uint32_t len = rnd(4) == 0 ? 0u : (rnd(10) == 0 ? 70u : rnd(6));  // empty, longer than a wave is wide, short
    for (uint32_t i = 0; i < len; i++) sets[q].push_back(WANTED[rnd(9)]);
    values.insert(values.end(), sets[q].begin(), sets[q].end());
    first.push_back((uint32_t)values.size());
    lo.push_back(BOUNDS[rnd(9)]), hi.push_back(rnd(3) == 0 ? NONE : BOUNDS[rnd(9)]);  // lo > hi among them
  }
  const uint64_t nwant = values.size();
  values.shrink_to_fit();
  // the claim (labelset_plan.h, unchanged), in a random order of the queries: the lowest query keeps a pair
  std::vector<uint32_t> owner(nwant, PH_LABELSET_OWNER_NONE), turn(nq);
  std::iota(turn.begin(), turn.end(), 0u);
  for (uint32_t i = nq; i > 1; i--) std::swap(turn[i - 1], turn[rnd(i)]);
  for (uint32_t q : turn) {
    CHECK(ph_labelset_range_ok(first[q], first[q + 1], nwant));
    for (uint32_t i = first[q]; i < first[q + 1]; i++) CHECK(ph_labelset_claim(owner.data(), i, q));
  }
  // the span per pair against a walk over the sorted column
  std::vector<uint32_t> at(nwant), len(nwant), key(nwant);
  for (uint64_t i = 0; i < nwant; i++) {
    const uint32_t q = owner[i];
    CHECK(q < nq && first[q] <= i && i < first[q + 1]);
    ph_label_range_span(sp, listed, values[i], lo[q], hi[q], &at[i], &len[i]);
    uint64_t count = 0, start = 0;
    for (uint64_t p = 0; p < listed; p++) {
      const uint32_t lbl = (uint32_t)(w.spairs[p] / 4294967296ull), k = (uint32_t)(w.spairs[p] % 4294967296ull);
      const bool in = values[i] != NONE && lbl == values[i] && k >= lo[q] && k <= hi[q];
      if (in && !count) start = p;
      count += in ? 1u : 0u;
    }
    CHECK(len[i] == count && (count ? at[i] == start : at[i] == 0u) && (uint64_t)at[i] + len[i] <= listed);
    key[i] = ph_label_range_sort_key(at[i], len[i]);
  }
  // the stable sort by span start, then the duplicate rule position by position
  std::vector<uint32_t> sorted(nwant);
  std::iota(sorted.begin(), sorted.end(), 0u);
  std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  std::vector<uint32_t> dup(nwant, 0u);
  for (uint64_t pos = 1; pos < nwant; pos++) {
    const uint32_t i = sorted[pos], j = sorted[pos - 1];
    dup[i] = ph_labelset_range_dup(at[i], len[i], owner[i], at[j], len[j], owner[j]) ? 1u : 0u;
  }
  for (uint32_t q = 0; q < nq; q++) {
    // the kept positions of a query are exactly its distinct labels with non-empty spans, each once
    std::multiset<uint32_t> kept;
    std::set<uint32_t> distinct;
    uint64_t kept_rows = 0;
    for (uint32_t i = first[q]; i < first[q + 1]; i++) {
      if (len[i] && !dup[i]) kept.insert(values[i]), kept_rows += len[i];
      if (len[i]) distinct.insert(values[i]);
    }
    CHECK(kept.size() == distinct.size() && std::set<uint32_t>(kept.begin(), kept.end()) == distinct);
    // the count equals the popcount of the mask, and so do the rows the kept positions scan
    uint64_t pop = 0;
    for (uint32_t v = 0; v < w.labels.size(); v++) {
      const bool bit = mask_bit(w, v, sets[q], lo[q], hi[q]);
      pop += bit ? 1u : 0u;
      // the walk's predicate and the routed call's candidate test say what the mask says, for every (row, query)
      CHECK(ph_pairset_holds(w.pair_of[v], first[q], first[q + 1], values.data(), lo[q], hi[q], NONE64) == bit);
      CHECK(ph_auto_pairset_candidate(w.pair_of.data(), (uint32_t)w.labels.size(), first[q], first[q + 1], values.data(), lo[q], hi[q], v,
                                      NONE64) == bit);
    }
    CHECK(ph_labelset_range_count(sp, listed, values.data(), first[q], first[q + 1], nwant, lo[q], hi[q]) == pop && kept_rows == pop);
    uint32_t by_pair = 0;
    for (uint32_t i = first[q]; i < first[q + 1]; i++) by_pair += ph_labelset_range_count_pair(sp, listed, values.data(), first[q], i, lo[q], hi[q]);
    CHECK(by_pair == pop);
    // an id at or past n is no candidate, and nothing is read for it
    CHECK(!ph_auto_pairset_candidate(w.pair_of.data(), (uint32_t)w.labels.size(), first[q], first[q + 1], values.data(), lo[q], hi[q],
                                     (uint32_t)w.labels.size(), NONE64));
    CHECK(!ph_auto_pairset_candidate(w.pair_of.data(), (uint32_t)w.labels.size(), first[q], first[q + 1], values.data(), lo[q], hi[q], NONE, NONE64));
  }
}

static void test_predicate_edges() {
  const uint32_t set[] = {NONE, 0x80000000u, 0xFFFFFFFEu, 3u, 3u};
  const auto holds = [&](uint64_t pair, uint32_t b, uint32_t e, uint32_t lo, uint32_t hi) { return ph_pairset_holds(pair, b, e, set, lo, hi, NONE64); };
  // a row that is not listed passes nothing, although NONE is in the set and its key word lies inside an open range
  CHECK(!holds(NONE64, 0, 5, 0u, NONE) && !holds(NONE64, 0, 1, NONE, NONE));
  CHECK(holds(ph_pair_bound(0x80000000u, 9u), 0, 5, 9u, 9u) && !holds(ph_pair_bound(0x80000000u, 9u), 0, 1, 0u, NONE));
  CHECK(holds(ph_pair_bound(0xFFFFFFFEu, 0xFFFFFFFEu), 0, 5, 0u, NONE) && holds(ph_pair_bound(0xFFFFFFFEu, 0u), 2, 3, 0u, 0u));
  CHECK(!holds(ph_pair_bound(0xFFFFFFFEu, 5u), 0, 5, 6u, 4u));   // lo > hi, with the key between
  CHECK(!holds(ph_pair_bound(0x7FFFFFFFu, 5u), 0, 5, 0u, NONE));  // the neighbour below 2^31 is not in the set
  CHECK(!holds(ph_pair_bound(4u, 5u), 0, 5, 0u, NONE) && holds(ph_pair_bound(3u, 5u), 3, 5, 5u, 5u) && holds(ph_pair_bound(3u, 5u), 4, 5, 0u, NONE));
  CHECK(!holds(ph_pair_bound(3u, 5u), 3, 3, 0u, NONE));  // an empty set
  CHECK(ph_auto_scan_below_labelset_ranged(0) == PH_AUTO_SCAN_BELOW_LABELSET_RANGED && ph_auto_scan_below_labelset_ranged(5) == 5u);
  CHECK(ph_auto_scan_below_labelset_ranged(UINT64_MAX) == UINT64_MAX && PH_AUTO_SCAN_BELOW_LABELSET_RANGED == 5000u);
  // the duplicate rule: an empty span repeats nothing; another query, another start, another length do not either
  CHECK(ph_labelset_range_dup(7u, 3u, 2u, 7u, 3u, 2u) && !ph_labelset_range_dup(0u, 0u, 2u, 0u, 0u, 2u));
  CHECK(!ph_labelset_range_dup(7u, 3u, 2u, 7u, 3u, 1u) && !ph_labelset_range_dup(7u, 3u, 2u, 6u, 3u, 2u) && !ph_labelset_range_dup(7u, 3u, 2u, 7u, 4u, 2u));
  // a range that is not sound counts 0 and reads nothing
  CHECK(ph_labelset_range_count(nullptr, 0, nullptr, 5, 3, 10, 0u, NONE) == 0u && ph_labelset_range_count(nullptr, 0, nullptr, 3, 11, 10, 0u, NONE) == 0u);
}

// claims over offsets nobody checked: ranges that overlap, run backwards or leave [0, nwant]; the lowest query keeps a
// pair whatever the order of the claims, a query that does not own its whole range is refused
static void test_claims() {
  const uint64_t nwant = 12;
  const uint32_t first[] = {0, 3, 5, 5, 9, 7, 12, 17, 14, 12};  // q4 backwards, q5 overlaps q3, q6 past nwant, q7 backwards, q8 sound
  const uint32_t nq = 9;
  for (int round = 0; round < 50; round++) {
    std::vector<uint32_t> owner(nwant, PH_LABELSET_OWNER_NONE), turn(nq);
    owner.shrink_to_fit();
    std::iota(turn.begin(), turn.end(), 0u);
    for (uint32_t i = nq; i > 1; i--) std::swap(turn[i - 1], turn[rnd(i)]);
    for (uint32_t q : turn) {
      if (!ph_labelset_range_ok(first[q], first[q + 1], nwant)) continue;
      for (uint32_t i = first[q]; i < first[q + 1]; i++)
        if (!ph_labelset_claim(owner.data(), i, q)) break;
    }
    std::vector<bool> ok(nq);
    for (uint32_t q = 0; q < nq; q++) {
      ok[q] = ph_labelset_range_ok(first[q], first[q + 1], nwant);
      for (uint32_t i = first[q]; ok[q] && i < first[q + 1]; i++) ok[q] = owner[i] == q;
    }
    const bool expect[] = {true, true, true, true, false, false, false, false, false};  // q8 = [14, 12): backwards too
    for (uint32_t q = 0; q < nq; q++) CHECK(ok[q] == expect[q]);
    for (uint32_t i = 5; i < 9; i++) CHECK(owner[i] == 3u);  // the lower query keeps what both claimed
  }
  CHECK(ph_labelset_first_bad(first, nq) == 4u);
}

int main() {
  test_predicate_edges();
  test_claims();
  for (uint32_t n : {0u, 1u, 2u, 17u, 64u, 65u, 300u}) {
    const World w = make_world(n);
    for (int round = 0; round < 6; round++) check_batch(w, round == 0 ? 1u : 1u + rnd(40));
  }
  std::printf("ALL OK\n");
  return 0;
}
