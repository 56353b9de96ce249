// Stand-alone host check of the pure functions the calls by a SET of row labels added to
// parallel_hnsw_amd/csrc/filter_route.h: compiled with -fsanitize=address,undefined and run without a GPU
// (tests/test_labelset_route_cpp.py).  The range soundness test of the untrusted offsets, the membership predicate of the
// walk (ph_set_holds) and the candidate test of exclude[q] (ph_auto_set_candidate) over arrays of exactly the sizes a call
// holds -- an index out of bounds is a sanitizer report --, each against the bitmap form of the same statement, and the
// default resolution of scan_below.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/filter_route.h"

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

// the statement itself: v is listed (its label is a label) and its label occurs in the set
static bool holds(uint32_t lbl, const std::vector<uint32_t> &set) {
  if (lbl == NONE) return false;
  for (uint32_t s : set)
    if (s == lbl) return true;
  return false;
}

int main() {
  // ---- the range of a query: inside [0, nwant], not backwards
  for (uint64_t nwant : {0ull, 1ull, 7ull, 0x7FFFFFFEull}) {
    CHECK(ph_set_range_sound(0u, 0u, nwant));          // empty at the start
    CHECK(ph_set_range_sound(nwant, nwant, nwant));    // empty at the end
    CHECK(ph_set_range_sound(0u, nwant, nwant));       // the whole table
    CHECK(!ph_set_range_sound(0u, nwant + 1u, nwant)); // one past
    CHECK(!ph_set_range_sound(nwant + 1u, nwant + 1u, nwant));  // empty, but outside
    CHECK(!ph_set_range_sound(nwant + 1u, nwant, nwant));
    if (nwant) {
      CHECK(!ph_set_range_sound(nwant, nwant - 1u, nwant));  // backwards inside
      CHECK(!ph_set_range_sound(1u, 0u, nwant));
      CHECK(ph_set_range_sound(nwant - 1u, nwant, nwant));
    }
    CHECK(!ph_set_range_sound(0u, 0xFFFFFFFFu, nwant));
    CHECK(!ph_set_range_sound(0xFFFFFFFFu, 0u, nwant));
  }
  // a walk reads values[first .. last) of a sound range only: a table of exactly nwant words serves every such range
  for (int round = 0; round < 200; round++) {
    const uint32_t nwant = (uint32_t)(rnd() % 70u);
    std::vector<uint32_t> values(nwant);
    for (uint32_t &v : values) v = (uint32_t)(rnd() % 6u);
    for (int t = 0; t < 50; t++) {
      const uint32_t b = (uint32_t)(rnd() % (nwant + 3u)), e = (uint32_t)(rnd() % (nwant + 3u));
      if (!ph_set_range_sound(b, e, nwant)) continue;
      const std::vector<uint32_t> set(values.begin() + b, values.begin() + e);
      for (uint32_t lbl : {0u, 1u, 5u, 6u, NONE}) CHECK(ph_set_holds(lbl, b, e, values.data(), NONE) == holds(lbl, set));
    }
  }
  // ---- membership: the cases by name
  {
    const std::vector<uint32_t> label_of = {3u, NONE, 7u, 3u, 0u, NONE};  // v = 1 and v = 5 are not listed
    const uint32_t n = (uint32_t)label_of.size();
    auto cand = [&](const std::vector<uint32_t> &values, uint32_t b, uint32_t e, uint32_t v) {
      return ph_auto_set_candidate(label_of.data(), n, b, e, values.data(), v, NONE);
    };
    const std::vector<uint32_t> with_none = {NONE, 3u};
    CHECK(cand(with_none, 0u, 2u, 0u) && cand(with_none, 0u, 2u, 3u));
    CHECK(!cand(with_none, 0u, 2u, 1u));  // NONE in the set does not admit an unlisted vector
    CHECK(!cand(with_none, 0u, 1u, 1u) && !cand(with_none, 0u, 1u, 0u));  // a set of NONE alone admits nothing
    CHECK(!cand(with_none, 0u, 2u, 2u));  // another label
    CHECK(!cand(with_none, 0u, 2u, n) && !cand(with_none, 0u, 2u, n + 1u) && !cand(with_none, 0u, 2u, 0xFFFFFFFFu));  // v >= n
    const std::vector<uint32_t> dup = {7u, 7u, 0u, 7u};
    CHECK(cand(dup, 0u, 4u, 2u) && cand(dup, 0u, 4u, 4u) && !cand(dup, 0u, 4u, 0u));
    CHECK(cand(dup, 1u, 2u, 2u) && !cand(dup, 2u, 3u, 2u));  // the range, not the table, is the set
    CHECK(!cand(dup, 0u, 0u, 2u) && !cand(dup, 4u, 4u, 2u) && !cand(dup, 2u, 2u, 4u));  // an empty set
    std::vector<uint32_t> long_set(65u, 1000u);  // 64 labels nobody carries, the match past one chunk of 64
    for (uint32_t i = 0; i < 64u; i++) long_set[i] = 1000u + i;
    long_set[64] = 0u;
    CHECK(cand(long_set, 0u, 65u, 4u) && !cand(long_set, 0u, 64u, 4u) && !cand(long_set, 0u, 65u, 0u));
  }
  // ---- exclude[q] is a candidate iff it is listed under a label of the set: the column against the bitmap of the set
  for (int round = 0; round < 200; round++) {
    const uint32_t n = 1u + (uint32_t)(rnd() % 200u);
    std::vector<uint32_t> label_of(n);
    for (uint32_t &l : label_of) l = rnd() % 4u == 0u ? NONE : (uint32_t)(rnd() % 4u) * 0x55555555u;  // 0xFFFFFFFF is NONE
    const uint32_t nwant = (uint32_t)(rnd() % 9u);
    std::vector<uint32_t> values(nwant);
    for (uint32_t &v : values) v = rnd() % 5u == 0u ? 9u : (uint32_t)(rnd() % 4u) * 0x55555555u;
    const uint32_t b = nwant ? (uint32_t)(rnd() % nwant) : 0u, e = b + (nwant ? (uint32_t)(rnd() % (nwant - b + 1u)) : 0u);
    CHECK(ph_set_range_sound(b, e, nwant));
    const std::vector<uint32_t> set(values.begin() + b, values.begin() + e);
    std::vector<uint32_t> bitmap((n + 31u) / 32u, 0u);
    for (uint32_t v = 0; v < n; v++)
      if (holds(label_of[v], set)) bitmap[v >> 5] |= 1u << (v & 31u);
    for (uint32_t v : {0u, n - 1u, n, n + 31u, 0xFFFFFFFFu, (uint32_t)(rnd() % n)}) {
      const bool by_bitmap = v < n && ((bitmap[v >> 5] >> (v & 31u)) & 1u);
      CHECK(ph_auto_set_candidate(label_of.data(), n, b, e, values.data(), v, NONE) == by_bitmap);
    }
  }
  // ---- the default threshold of a call by set resolves through its own constant; the other calls keep theirs
  CHECK(ph_auto_scan_below_labelset(0u) == PH_AUTO_SCAN_BELOW_LABELSET);
  CHECK(ph_auto_scan_below_labelset(1u) == 1u && ph_auto_scan_below_labelset(UINT64_MAX) == UINT64_MAX);
  CHECK(ph_auto_scan_below_labeled(0u) == PH_AUTO_SCAN_BELOW_LABELED);
  CHECK(ph_auto_scan_below(0u, true) == PH_AUTO_SCAN_BELOW_PER_QUERY && ph_auto_scan_below(0u, false) == PH_AUTO_SCAN_BELOW_SHARED);
  std::printf("ALL OK\n");
  return 0;
}
