// Stand-alone host check of the integer rules behind the exact scan over an allow-list (parallel_hnsw_amd/csrc/
// exact_slices.h, the header the launcher and the kernels include): compiled with -fsanitize=address,undefined and run
// without a GPU (tests/test_exact_slices_cpp.py).  It checks the k and stride argument rules, the slice-count rule and
// that the slices' pass ranges tile the bitmap, and it walks a host model of the scan's indexing -- bitmap words, the
// staged ids of a pass, the two key lists -- over real arrays of exactly the sizes the launcher allocates, so that an
// index out of bounds is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/exact_slices.h"

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

// the stride rule of phnsw_search_batch_filtered, which the exact calls share: 0 = one bitmap, else >= ceil(n / 32)
static bool stride_valid(uint64_t n, uint32_t stride) { return stride == 0 || stride >= ph_exact_words(n); }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// one query's scan as the kernel indexes it: returns the candidates it visited, in order
static std::vector<uint32_t> model_scan(const std::vector<uint32_t> &bitmap, uint64_t n, uint32_t nlim, uint32_t exclude,
                                        uint32_t slices, uint32_t k) {
  const uint64_t nwords = ph_exact_words(n), passes = ph_exact_passes(n);
  CHECK(bitmap.size() == nwords);
  std::vector<uint64_t> lds(ph_exact_own_lds(k) / 8);  // the scan's LDS: two key lists, the survivors, the staged ids
  uint64_t *const keys = lds.data();
  uint32_t *const stage = (uint32_t *)(keys + 2u * k + 64u);
  CHECK((char *)(stage + PH_EXACT_PASS_IDS) == (char *)lds.data() + ph_exact_own_lds(k));
  std::vector<uint32_t> seen;
  for (uint32_t s = 0; s < slices; s++) {
    uint64_t p0, p1;
    ph_exact_slice_range(s, slices, passes, &p0, &p1);
    for (uint64_t p = p0; p < p1; p++) {
      uint32_t total = 0;
      for (uint32_t lane = 0; lane < 64; lane++) {
        const uint32_t widx = (uint32_t)(p * PH_EXACT_PASS_WORDS) + lane;
        uint32_t w = 0;
        if (widx < nwords && widx * 32u < nlim) {
          w = bitmap[widx];
          if (nlim - widx * 32u < 32u) w &= (1u << (nlim - widx * 32u)) - 1u;
        }
        if (exclude != 0xFFFFFFFFu && (exclude >> 5) == widx) w &= ~(1u << (exclude & 31u));
        for (uint32_t t = w; t; t &= t - 1u) {
          CHECK(total < PH_EXACT_PASS_IDS);
          stage[total++] = widx * 32u + (uint32_t)__builtin_ctz(t);
        }
      }
      for (uint32_t i = 0; i < total; i++) {
        CHECK(stage[i] < nlim && stage[i] < n);
        seen.push_back(stage[i]);
        keys[i % k] = stage[i], keys[k + i % k] = stage[i], keys[2u * k + i % 64u] = stage[i];  // every list, every slot
      }
    }
  }
  return seen;
}

int main() {
  // k: 1..1024
  CHECK(!ph_exact_k_valid(0) && ph_exact_k_valid(1) && ph_exact_k_valid(1024) && !ph_exact_k_valid(1025));
  CHECK(!ph_exact_k_valid(UINT64_MAX) && !ph_exact_k_valid(1ull << 32));
  // stride: 0 or at least one bitmap
  CHECK(stride_valid(5000, 0) && stride_valid(5000, 157) && stride_valid(5000, 160) && !stride_valid(5000, 156));
  CHECK(stride_valid(32, 1) && !stride_valid(33, 1) && stride_valid(1, 1));
  // words and passes
  CHECK(ph_exact_words(1) == 1 && ph_exact_words(32) == 1 && ph_exact_words(33) == 2 && ph_exact_words(5000) == 157);
  CHECK(ph_exact_passes(1) == 1 && ph_exact_passes(2048) == 1 && ph_exact_passes(2049) == 2 && ph_exact_passes(5000) == 3);
  CHECK(ph_exact_passes(0x7FFFFFFEull) == (1ull << 20));
  // LDS: 16 * k + 8704 bytes (phnsw.h quotes it)
  CHECK(ph_exact_own_lds(1) == 16 + 8704 && ph_exact_own_lds(1024) == 16 * 1024 + 8704);
  // slice count: one when the queries fill the device, else enough to fill it, at most the passes, never 0
  CHECK(ph_exact_slice_count(10000, 4096, 489, 0) == 1);
  CHECK(ph_exact_slice_count(4096, 4096, 489, 0) == 1);
  CHECK(ph_exact_slice_count(16, 4096, 489, 0) == 256);
  CHECK(ph_exact_slice_count(16, 4096, 3, 0) == 3);
  CHECK(ph_exact_slice_count(1, 4096, 489, 0) == 489);
  CHECK(ph_exact_slice_count(16, 4096, 3, 1) == 1 && ph_exact_slice_count(16, 4096, 3, 2) == 2);
  CHECK(ph_exact_slice_count(16, 4096, 3, 1000) == 3 && ph_exact_slice_count(16, 4096, 3, -5) == 3);
  CHECK(ph_exact_slice_count(0, 4096, 3, 0) == 1 && ph_exact_slice_count(16, 0, 3, 0) == 1);
  CHECK(ph_exact_slice_count(16, 4096, 0, 0) == 1 && ph_exact_slice_count(1, UINT64_MAX, 1ull << 20, 0) == (1u << 20));
  CHECK(ph_exact_slice_count(5, 4096, 1ull << 40, 1ll << 40) == 0xFFFFFFFFu);
  // the ranges tile [0, passes) in order, sizes within one of each other
  for (uint64_t passes : {1ull, 2ull, 3ull, 7ull, 64ull, 489ull, 1ull << 20})
    for (uint32_t slices : {1u, 2u, 3u, 5u, 64u, 489u}) {
      if (slices > passes) continue;
      uint64_t at = 0, lo = UINT64_MAX, hi = 0;
      for (uint32_t s = 0; s < slices; s++) {
        uint64_t p0, p1;
        ph_exact_slice_range(s, slices, passes, &p0, &p1);
        CHECK(p0 == at && p1 >= p0 && p1 <= passes);
        lo = p1 - p0 < lo ? p1 - p0 : lo;
        hi = p1 - p0 > hi ? p1 - p0 : hi;
        at = p1;
      }
      CHECK(at == passes && hi - lo <= 1 && lo >= 1);
    }
  // the host model of the scan: every slicing visits exactly the candidates, each once, in id order
  for (uint64_t n : {1ull, 31ull, 32ull, 33ull, 2047ull, 2048ull, 2049ull, 5000ull, 70001ull})
    for (int fill = 0; fill < 3; fill++) {
      std::vector<uint32_t> bitmap(ph_exact_words(n));
      for (uint32_t &w : bitmap) w = fill == 0 ? 0xFFFFFFFFu : (fill == 1 ? (uint32_t)rnd() & (uint32_t)rnd() : 0u);
      if (fill == 2) bitmap.back() = 0xFFFFFFFFu;  // the last word only, garbage past n included
      for (uint32_t nlim : {(uint32_t)n, (uint32_t)(n > 100 ? n - 100 : n)}) {
        const uint32_t exclude = fill == 1 ? (uint32_t)(rnd() % n) : 0xFFFFFFFFu;
        std::vector<uint32_t> want;
        for (uint32_t v = 0; v < nlim; v++)
          if (((bitmap[v >> 5] >> (v & 31)) & 1u) && v != exclude) want.push_back(v);
        const uint64_t passes = ph_exact_passes(n);
        for (long long forced : {0ll, 1ll, 2ll, 3ll, 1000ll})
          for (uint32_t k : {1u, 10u, 1024u}) {
            const uint32_t slices = ph_exact_slice_count(16, 4096, passes, forced);
            CHECK(slices >= 1 && slices <= passes);
            CHECK(model_scan(bitmap, n, nlim, exclude, slices, k) == want);
          }
      }
    }
  std::puts("ALL OK");
  return 0;
}
