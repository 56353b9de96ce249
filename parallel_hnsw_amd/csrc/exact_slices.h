// How the exact scan over an allow-list (filter_exact.hip) is cut: pure integer rules, shared by the launcher, the
// kernels and tests/cpp/test_exact_slices.cpp (which runs them under the host sanitizers, no GPU).
//
// A bitmap of ceil(n / 32) words is read in PASSES of 64 words (one word per lane of a wave64).  A query's passes are
// dealt to `slices` waves, slice s taking the contiguous range [s * passes / slices, (s + 1) * passes / slices): the
// ranges tile [0, passes) without gap or overlap and differ by at most one pass.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PH_EXACT_HD __host__ __device__
#else
#define PH_EXACT_HD
#endif

#define PH_EXACT_KMAX 1024u      // largest k of phnsw_search_exact_filtered (phnsw.h)
#define PH_EXACT_PASS_WORDS 64u  // bitmap words per pass
#define PH_EXACT_PASS_IDS 2048u  // ids one pass can expand to: 64 words x 32 bits

PH_EXACT_HD static inline uint64_t ph_exact_words(uint64_t n) { return (n + 31u) / 32u; }
static inline bool ph_exact_k_valid(uint64_t k) { return k >= 1u && k <= PH_EXACT_KMAX; }
PH_EXACT_HD static inline uint64_t ph_exact_passes(uint64_t n) {
  return (ph_exact_words(n) + PH_EXACT_PASS_WORDS - 1u) / PH_EXACT_PASS_WORDS;
}

// slices per query: one when the queries alone fill the device (nq >= resident waves), else enough to fill it, never
// more than there are passes and never 0.  forced > 0 (PHNSW_EXACT_SLICES) replaces the rule, clamped the same way.
static inline uint32_t ph_exact_slice_count(uint64_t nq, uint64_t resident, uint64_t passes, long long forced) {
  if (passes == 0) return 1u;
  uint64_t s = 1;
  if (forced > 0)
    s = (uint64_t)forced;
  else if (nq > 0 && nq < resident)
    s = (resident + nq - 1) / nq;
  if (s > passes) s = passes;
  if (s > 0xFFFFFFFFull) s = 0xFFFFFFFFull;
  return s ? (uint32_t)s : 1u;
}

// passes of slice `slice`: [*p0, *p1)
PH_EXACT_HD static inline void ph_exact_slice_range(uint32_t slice, uint32_t slices, uint64_t passes, uint64_t *p0,
                                                    uint64_t *p1) {
  *p0 = (uint64_t)slice * passes / slices;
  *p1 = ((uint64_t)slice + 1u) * passes / slices;
}

// dynamic LDS of the scan besides a PQ store's table: two key lists of k entries (the running top-k and the one being
// merged into), 64 sorted survivor keys, the ids of one pass
PH_EXACT_HD static inline uint64_t ph_exact_own_lds(uint64_t k) { return 2u * k * 8u + 64u * 8u + PH_EXACT_PASS_IDS * 4u; }
