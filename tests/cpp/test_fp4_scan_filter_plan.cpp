// The integer rules of the filtered MXFP4 scan (parallel_hnsw_amd/csrc/fp4_scan_filter_plan.h) in a stand-alone host
// program: built by g++ under AddressSanitizer and UBSan, run as a process of its own
// (tests/test_fp4_scan_filter_plan_cpp.py).  The word masks count exactly the rows below n; the compaction, replayed
// on the host into a buffer of exactly ph_fp4_scan_pre_bytes(n), stays inside it, leaves an ascending list padded to whole
// row groups with its last id; and the list's row groups, cut by ph_exact_slice_range into more slices than there are
// groups, tile it without gap or overlap.
#include <cstdio>
#include <random>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/fp4_scan_filter_plan.h"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      if (failures++ < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                         \
  } while (0)

int main() {
  std::mt19937 rng(11);
  for (uint64_t n : {1ull, 15ull, 16ull, 17ull, 31ull, 32ull, 33ull, 1000ull, 4097ull, 70001ull}) {
    const uint64_t nwords = ph_exact_words(n);
    uint64_t bits = 0;
    for (uint64_t w = 0; w < nwords + 2u; w++) bits += (uint64_t)__builtin_popcount(ph_fp4_scan_word_mask(w, n));
    CHECK(bits == n);
    CHECK(ph_fp4_scan_pre_list(n) % 64u == 0 && ph_fp4_scan_pre_list(n) >= PH_FP4_SCAN_HEAD_WORDS + nwords + 1u);
    CHECK(ph_fp4_scan_pre_bytes(n) % 256u == 0);
    for (double density : {0.0, 0.001, 0.5, 1.0}) {
      std::vector<uint32_t> filter(nwords);
      for (auto &w : filter) w = density >= 1.0 ? 0xFFFFFFFFu : 0u;  // all ones: bits past n set
      if (density > 0.0 && density < 1.0)
        for (uint64_t v = 0; v < nwords * 32u; v++)
          if (rng() < density * 4294967296.0 || v == n - 1u) filter[v / 32u] |= 1u << (v % 32u);
      std::vector<uint32_t> pre(ph_fp4_scan_pre_bytes(n) / 4u);  // exactly the scratch: ASan sees a step outside
      uint32_t *const off = pre.data() + PH_FP4_SCAN_HEAD_WORDS, *const list = pre.data() + ph_fp4_scan_pre_list(n);
      uint32_t m = 0;
      for (uint64_t w = 0; w < nwords; w++) off[w] = m, m += (uint32_t)__builtin_popcount(filter[w] & ph_fp4_scan_word_mask(w, n));
      off[nwords] = pre[0] = m;
      for (uint64_t w = 0; w < nwords; w++) {
        const uint32_t b = filter[w] & ph_fp4_scan_word_mask(w, n);
        uint32_t o = off[w];
        for (uint32_t t = b; t; t &= t - 1u) list[o++] = (uint32_t)w * 32u + (uint32_t)__builtin_ctz(t);
        if (b && o == m)
          for (uint64_t p = m; p < ph_fp4_scan_list_len(m); p++) list[p] = (uint32_t)w * 32u + 31u - (uint32_t)__builtin_clz(b);
      }
      const uint64_t len = ph_fp4_scan_list_len(m), groups = ph_fp4_scan_list_groups(m);
      CHECK(m <= n && len % 16u == 0 && len >= m && len < m + 16u && groups * 16u == len);
      for (uint64_t i = 0; i < len; i++) {
        CHECK(list[i] < n);
        if (i) CHECK(i < m ? list[i] > list[i - 1] : list[i] == list[m - 1]);
      }
      for (uint32_t slices : {1u, 3u, 7u, (uint32_t)ph_fp4_scan_groups(n)}) {  // cut from n's groups, more than m's
        uint64_t at = 0;
        for (uint32_t s = 0; s < slices; s++) {
          uint64_t g0, g1;
          ph_exact_slice_range(s, slices, groups, &g0, &g1);
          CHECK(g0 == at && g1 >= g0 && g1 <= groups);
          at = g1;
        }
        CHECK(at == groups);
      }
    }
  }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
