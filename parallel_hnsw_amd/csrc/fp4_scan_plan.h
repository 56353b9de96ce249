// How the exhaustive MXFP4 scan over an fp4 store (scan_fp4.hip) is cut: pure integer rules (and the one float rule of
// the threshold), shared by the launcher, the kernels and tests/cpp/test_fp4_scan_plan.cpp (which runs them under the
// host sanitizers, no GPU).
//
//   block     = 32 consecutive components under one E8M0 scale: one lane's operand of a block-scaled MFMA
//   step      = 128 components, four blocks: one v_mfma_scale_f32_16x16x128_f8f6f4; a row of ld components has
//               ceil(ld / 128) of them, the kernels are compiled for classes of 2, 6 and 12
//   group     = 16 consecutive rows (the M side of the instruction); a store of n rows has ceil(n / 16) of them
//   tile      = T = 16, 32 or 64 consecutive queries of a launch: the 1, 2 or 4 query groups (the N side) whose codes a
//               wave keeps in registers
//   slice     = a contiguous range of row groups (ph_exact_slice_range: no gap, no overlap)
//   work item = (tile, slice), slice-major: item = slice * tiles + tile, one 64-thread workgroup each
//   chunk     = the queries of one launch: every (query, slice) owns 3 r keys of scratch (the two lists of its running
//               top-r and the list the merge reads), all under PH_FP4_SCAN_SCRATCH bytes
// None of these changes which rows share a query's MFMA (a group is 16 consecutive rows whatever the cut), so none
// changes a score; the keys are distinct, so the r smallest are one set in one order.
#pragma once
#include <stdint.h>

#include "exact_slices.h"

#define PH_FP4_SCAN_RMAX 1024u              // largest r of phnsw_fp4_scan_topk (phnsw.h)
#define PH_FP4_SCAN_TMAX 64u                // largest tile
#define PH_FP4_SCAN_SCRATCH (1ull << 30)    // bound of the lists of one launch, in bytes
#define PH_FP4_SCAN_CHUNK_MAX 65536ull      // queries of one launch at the most

static inline bool ph_fp4_scan_r_valid(uint64_t r) { return r >= 1u && r <= PH_FP4_SCAN_RMAX; }
PH_EXACT_HD static inline uint64_t ph_fp4_scan_groups(uint64_t n) { return (n + 15u) / 16u; }
PH_EXACT_HD static inline uint32_t ph_fp4_scan_blocks(uint32_t ld) { return (ld + 31u) / 32u; }
PH_EXACT_HD static inline uint32_t ph_fp4_scan_steps(uint32_t ld) { return (ld + 127u) / 128u; }
// the compiled class of a step count (0: none, ld > 1536)
static inline int ph_fp4_scan_class(uint32_t steps) { return steps <= 2u ? 2 : (steps <= 6u ? 6 : (steps <= 12u ? 12 : 0)); }

// Bytes of a query in the prepared operand buffers: 4 * steps blocks of 16 code bytes, block order; and its scale
// bytes, arranged for the lanes that read them: lane group kb = lane / 16 owns blocks 4 s + kb, its scale of step s is
// byte s of a run of `ph_fp4_scan_scale_run` bytes (whole dwords: byte s & 3 of dword s >> 2)
PH_EXACT_HD static inline uint32_t ph_fp4_scan_code_bytes(uint32_t steps) { return 64u * steps; }
PH_EXACT_HD static inline uint32_t ph_fp4_scan_scale_run(uint32_t steps) { return (steps + 3u) & ~3u; }
PH_EXACT_HD static inline uint32_t ph_fp4_scan_scale_bytes(uint32_t steps) { return 4u * ph_fp4_scan_scale_run(steps); }

// staged keys per query: a row group adds at most 16, a flush takes at most 64 (one per lane).  A long list is slow
// to fill 16 keys at a time, so it gets the larger stage
PH_EXACT_HD static inline uint32_t ph_fp4_scan_stage(uint32_t r) { return r >= 512u ? 64u : 32u; }
// LDS of a workgroup: the stages, 64 sorted survivors of an insert, four words of state per query
PH_EXACT_HD static inline uint32_t ph_fp4_scan_lds(uint32_t r, uint32_t T) { return T * ph_fp4_scan_stage(r) * 8u + 64u * 8u + T * 16u; }
PH_EXACT_HD static inline uint32_t ph_fp4_scan_merge_lds(uint32_t r) { return (2u * r + 64u) * 8u; }

// queries per tile: 64 while the codes of four query groups fit the registers beside two row groups (classes 2 and 6),
// else 32.  forced > 0 (PHNSW_FP4_SCAN_TILE) replaces the rule, rounded down to 16, 32 or 64 and held to the class's cap.
static inline uint32_t ph_fp4_scan_tile(int cls, long long forced) {
  const uint32_t cap = cls <= 6 ? 64u : 32u;
  uint32_t t = cap;
  if (forced > 0) t = forced >= 64 ? 64u : (forced >= 32 ? 32u : 16u);
  return t > cap ? cap : t;
}
static inline uint64_t ph_fp4_scan_tiles(uint64_t nq, uint32_t T) { return (nq + T - 1u) / T; }

// scratch of one (query, slice): two lists of the running top-r and the finished list
PH_EXACT_HD static inline uint64_t ph_fp4_scan_pair_bytes(uint32_t r) { return 3ull * r * 8u; }

// slices of a launch of `tiles` tiles: the rule of ph_exact_slice_count over the row groups (one when the tiles alone
// fill the device's `resident` workgroups, else enough to fill it; forced > 0: PHNSW_FP4_SCAN_SLICES), then cut so that
// the lists of a single tile fit the scratch
static inline uint32_t ph_fp4_scan_slices(uint64_t tiles, uint64_t resident, uint64_t groups, long long forced, uint32_t r,
                                          uint32_t T) {
  uint32_t s = ph_exact_slice_count(tiles, resident, groups, forced);
  const uint64_t fit = PH_FP4_SCAN_SCRATCH / (T * ph_fp4_scan_pair_bytes(r));  // >= 682: T r <= 64 * 1024
  if (s > fit) s = (uint32_t)fit;
  return s;
}

// queries of one launch: whole tiles, at most PH_FP4_SCAN_CHUNK_MAX and no more than the scratch holds lists for;
// never fewer than one tile (ph_fp4_scan_slices saw to its fit)
static inline uint64_t ph_fp4_scan_chunk(uint32_t slices, uint32_t r, uint32_t T) {
  uint64_t q = PH_FP4_SCAN_CHUNK_MAX;
  const uint64_t fit = PH_FP4_SCAN_SCRATCH / (slices * ph_fp4_scan_pair_bytes(r));
  if (fit < q) q = fit;
  q -= q % T;
  return q < T ? T : q;
}
// bytes of the lists of a launch of `tiles` tiles
static inline uint64_t ph_fp4_scan_scratch_bytes(uint64_t tiles, uint32_t T, uint32_t slices, uint32_t r) {
  return tiles * T * slices * ph_fp4_scan_pair_bytes(r);
}

// The threshold on the raw score.  A dot-product metric's last step is d = fl(1 - s) (ONE_MINUS_DOT) or fl(1 - s) / 2
// (COSINE_HALF; the halving is exact), not increasing in s.  Given the distance dk of a full list's last key, every s
// with distance <= dk has fl(1 - s) <= D = dk or 2 dk, so 1 - s <= D + 2^-24 |D| and s >= 1 - D - 2^-24 |D|.  The value
// returned lies below that: fl(1 - D) is within 2^-24 |1 - D| of 1 - D, the margin taken is 2^-22 (|1 - D| + |D|) and
// the last subtraction rounds by at most 2^-24 of its result.  Conservative only: a key that passes is tested again
// as a key.
PH_EXACT_HD static inline float ph_fp4_scan_smin(float dk, bool half) {
  const float D = half ? 2.0f * dk : dk;
  const float c = 1.0f - D;
  const float ac = c < 0.f ? -c : c, aD = D < 0.f ? -D : D;
  return c - (ac + aD) * (1.0f / 4194304.0f);
}
