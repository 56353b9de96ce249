// How the exhaustive Hamming scan over a bits store (scan_bits.hip) is cut: pure integer rules, shared by the launcher,
// the kernels and tests/cpp/test_bits_scan_plan.cpp (which runs them under the host sanitizers, no GPU).
//
//   batch     = 64 consecutive rows, one per lane of a wave64; a store of n rows has ceil(n / 64) of them
//   tile      = T consecutive queries of a launch, T = ph_bits_scan_tile(r): what fits a workgroup's share of the LDS
//   slice     = a contiguous range of batches (ph_exact_slice_range over the batches: no gap, no overlap)
//   work item = (tile, slice), slice-major: item = slice * tiles + tile, one 64-thread workgroup each
//   chunk     = the queries of one launch: with more than one slice the per-slice lists [queries][slices][r] stay
//               under PH_BITS_SCAN_SCRATCH bytes
// None of these changes a result: the keys are distinct, so the r smallest are one set in one order.
#pragma once
#include <stdint.h>

#include "exact_slices.h"

#define PH_BITS_SCAN_RMAX 1024u                  // largest r of phnsw_bits_scan_topk (phnsw.h)
#define PH_BITS_SCAN_TMAX 16u                    // largest tile
#define PH_BITS_SCAN_LDS (160u * 1024u / 4u)     // a workgroup's LDS budget: four workgroups a CU on gfx950's 160 KB
#define PH_BITS_SCAN_SCRATCH (64ull << 20)       // bound of the per-slice lists of one launch, in bytes
#define PH_BITS_SCAN_CHUNK_MAX 65536ull          // queries of one launch at the most (their sign words are scratch too)

static inline bool ph_bits_scan_r_valid(uint64_t r) { return r >= 1u && r <= PH_BITS_SCAN_RMAX; }
PH_EXACT_HD static inline uint64_t ph_bits_scan_batches(uint64_t n) { return (n + 63u) / 64u; }
// keys of one query of a tile: the running top-r and the list it is merged into (r each), the 64 sorted survivors of
// an insert (PhExactTopK), the 64 staged keys
PH_EXACT_HD static inline uint32_t ph_bits_scan_query_keys(uint32_t r) { return 2u * r + 64u + 64u; }
// ... and its bytes of LDS: the keys and four words of state (hmax, staged, len, which list is current)
PH_EXACT_HD static inline uint32_t ph_bits_scan_query_lds(uint32_t r) { return ph_bits_scan_query_keys(r) * 8u + 16u; }
PH_EXACT_HD static inline uint32_t ph_bits_scan_lds(uint32_t r, uint32_t T) { return T * ph_bits_scan_query_lds(r); }
// LDS of the merge kernel: one PhExactTopK
PH_EXACT_HD static inline uint32_t ph_bits_scan_merge_lds(uint32_t r) { return (2u * r + 64u) * 8u; }

// queries per tile: what the budget holds, 1 .. 16.  forced > 0 (PHNSW_BITS_SCAN_TILE) replaces the rule, clamped to
// 1 .. 16 and to what a whole workgroup's LDS (four budgets) holds.
static inline uint32_t ph_bits_scan_tile(uint32_t r, long long forced) {
  uint32_t t = PH_BITS_SCAN_LDS / ph_bits_scan_query_lds(r);
  if (forced > 0) {
    const uint32_t cap = 4u * PH_BITS_SCAN_LDS / ph_bits_scan_query_lds(r);
    t = forced > (long long)cap ? cap : (uint32_t)forced;
  }
  return t < 1u ? 1u : (t > PH_BITS_SCAN_TMAX ? PH_BITS_SCAN_TMAX : t);
}
static inline uint64_t ph_bits_scan_tiles(uint64_t nq, uint32_t T) { return (nq + T - 1u) / T; }

// slices of a launch of `tiles` tiles: the rule of ph_exact_slice_count over the batches (one when the tiles alone fill
// the device's `resident` workgroups, else enough to fill it; forced > 0: PHNSW_BITS_SCAN_SLICES), then cut so that the
// lists of a single tile fit the scratch
static inline uint32_t ph_bits_scan_slices(uint64_t tiles, uint64_t resident, uint64_t batches, long long forced,
                                           uint32_t r, uint32_t T) {
  uint32_t s = ph_exact_slice_count(tiles, resident, batches, forced);
  const uint64_t fit = PH_BITS_SCAN_SCRATCH / ((uint64_t)T * r * 8u);  // >= 512: T r <= 16 * 1024
  if (s > fit) s = (uint32_t)fit;
  return s;
}

// queries of one launch: whole tiles, at most PH_BITS_SCAN_CHUNK_MAX, and -- when the rows are cut into `slices` > 1
// slices -- no more than the scratch holds lists for; never fewer than one tile (ph_bits_scan_slices saw to its fit)
static inline uint64_t ph_bits_scan_chunk(uint32_t slices, uint32_t r, uint32_t T) {
  uint64_t q = PH_BITS_SCAN_CHUNK_MAX;
  if (slices > 1u) {
    const uint64_t fit = PH_BITS_SCAN_SCRATCH / ((uint64_t)slices * r * 8u);
    if (fit < q) q = fit;
  }
  q -= q % T;
  return q < T ? T : q;
}
// bytes of the per-slice lists of a launch of nq queries (0 with one slice: the rows are written directly)
static inline uint64_t ph_bits_scan_scratch_bytes(uint64_t nq, uint32_t slices, uint32_t r) {
  return slices > 1u ? nq * slices * r * 8u : 0u;
}
