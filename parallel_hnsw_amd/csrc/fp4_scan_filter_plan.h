// The integer rules the filtered MXFP4 scan (scan_fp4_filtered.hip) adds to fp4_scan_plan.h: which bits of a bitmap word
// count, how long the compacted row list of a shared bitmap is and where list, prefix and counter lie in the scan's
// scratch.  Shared by the launcher, the kernels and tests/cpp/test_fp4_scan_filter_plan.cpp (host sanitizers, no GPU).
//
//   bitmap  = ceil(n / 32) words, bit v % 32 of word v / 32 allows row v; bits at or past n do not count
//   list    = the m allowed rows of a shared bitmap, ascending, then its last id again up to a multiple of 16 entries:
//             row group g of the LIST form is entries 16 g .. 16 g + 15, one aligned run, every entry a row of the store;
//             only positions below m become keys
//   pre     = the scratch of the compaction: a head of 64 words (word 0 = m), the words' exclusive prefix, the list
#pragma once
#include <stdint.h>

#include "fp4_scan_plan.h"

#define PH_FP4_SCAN_HEAD_WORDS 64u  // 256 bytes: what follows stays 256-byte aligned

// the bits of bitmap word w that name rows below n
PH_EXACT_HD static inline uint32_t ph_fp4_scan_word_mask(uint64_t w, uint64_t n) {
  if (32u * w >= n) return 0u;
  const uint64_t left = n - 32u * w;
  return left >= 32u ? 0xFFFFFFFFu : (1u << (uint32_t)left) - 1u;
}
// entries of the list of m allowed rows, padding included, and its row groups
PH_EXACT_HD static inline uint64_t ph_fp4_scan_list_len(uint64_t m) { return (m + 15u) & ~(uint64_t)15u; }
PH_EXACT_HD static inline uint64_t ph_fp4_scan_list_groups(uint64_t m) { return ph_fp4_scan_groups(m); }
// words of the prefix (one past the last word holds the total), rounded so that the list starts on 256 bytes
PH_EXACT_HD static inline uint64_t ph_fp4_scan_off_words(uint64_t n) { return (ph_exact_words(n) + 1u + 63u) & ~(uint64_t)63u; }
// the list's word offset inside `pre` (the prefix starts behind the head), and the bytes of `pre` for a store of n rows
// (m <= n is not known on the host)
PH_EXACT_HD static inline uint64_t ph_fp4_scan_pre_list(uint64_t n) { return PH_FP4_SCAN_HEAD_WORDS + ph_fp4_scan_off_words(n); }
PH_EXACT_HD static inline uint64_t ph_fp4_scan_pre_bytes(uint64_t n) {
  return (ph_fp4_scan_pre_list(n) + ((ph_fp4_scan_list_len(n) + 63u) & ~(uint64_t)63u)) * 4u;
}
