// How the exhaustive int8 scan over an i8q store (scan_i8q.hip) is cut: pure integer rules, shared by the launcher, the
// kernels and tests/cpp/test_i8q_scan_plan.cpp (which runs them under the host sanitizers, no GPU).
//
//   image     = a stored row read as bytes: its f32 scale (4 bytes), ld int8 codes, zero padding to a multiple of 16
//               (RowI8, rowstore.hip: stride = (4 + ld + 15) & ~15).  The codes start at byte 4, so no 16 codes of a row
//               are 16-byte aligned; the scan therefore multiplies IMAGES: the query's image has four zero bytes where
//               the row has its scale, and whatever bytes the scale has, they add 0 to an integer sum
//   run       = 16 aligned bytes of an image, one lane's operand of a step; a row has ceil((4 + ld) / 16) of them
//   step      = 64 image bytes, four runs: one v_mfma_i32_16x16x64_i8; ceil((4 + ld) / 64) a row, the kernels are
//               compiled for classes of 2, 7, 13 and 25 (ld up to 124, 444, 828, 1596)
//   group     = 16 consecutive rows (the M side of the instruction)
//   row tile  = 1, 2 or 4 consecutive groups: what a workgroup stages in LDS at a time, rows `pitch` bytes apart
//   query tile= 64 consecutive queries of a launch: 16 for each of the four waves of a workgroup (the N side)
//   slice     = a contiguous range of row tiles (ph_exact_slice_range: no gap, no overlap)
//   work item = (query tile, slice), slice-major, one 256-thread workgroup each
//   chunk     = the queries of one launch, bounded by the lists' scratch as the fp4 scan's (fp4_scan_plan.h)
// None of these changes a dot product (an integer sum has no order) and the keys are distinct, so none changes a result.
#pragma once
#include <stdint.h>

#include "fp4_scan_plan.h"  // the stage, slice, chunk and threshold rules this scan shares

#define PH_I8Q_SCAN_RMAX 1024u   // largest r of phnsw_i8q_scan_topk (phnsw.h)
#define PH_I8Q_SCAN_QTILE 64u    // queries of a workgroup
#define PH_I8Q_SCAN_THREADS 256u
#define PH_I8Q_SCAN_LD_MAX 1536u

static inline bool ph_i8q_scan_r_valid(uint64_t r) { return r >= 1u && r <= PH_I8Q_SCAN_RMAX; }
PH_EXACT_HD static inline uint64_t ph_i8q_scan_groups(uint64_t n) { return (n + 15u) / 16u; }
PH_EXACT_HD static inline uint32_t ph_i8q_scan_runs(uint32_t ld) { return (4u + ld + 15u) / 16u; }
PH_EXACT_HD static inline uint32_t ph_i8q_scan_steps(uint32_t ld) { return (4u + ld + 63u) / 64u; }
// the compiled class of a step count (0: none, ld > 1596)
static inline int ph_i8q_scan_class(uint32_t steps) {
  return steps <= 2u ? 2 : (steps <= 7u ? 7 : (steps <= 13u ? 13 : (steps <= 25u ? 25 : 0)));
}
// bytes of a prepared query: its image, zero padded to whole steps
PH_EXACT_HD static inline uint32_t ph_i8q_scan_query_bytes(uint32_t steps) { return 64u * steps; }

// LDS bytes from one staged row to the next: every run a step reads, and one more.  An odd count of 16-byte runs:
// the 16 lanes that read the same run of 16 consecutive rows in one ds_read_b128 then fall on 16 different bank
// groups of four (ph_tiny_table_i8_kernel's 144-byte rule, 9 runs, is this for two steps).
PH_EXACT_HD static inline uint32_t ph_i8q_scan_pitch(uint32_t steps) { return (4u * steps + 1u) * 16u; }

// groups of a row tile: as many as keep a tile near 16 KiB (two of them are resident; a class-25 tile of one group is
// 25 KiB).  forced > 0 (PHNSW_I8Q_SCAN_TILE, in rows) replaces the rule, rounded down to 16, 32 or 64 rows and held to
// the class's cap: the kernels keep cap * class / 4 staging registers.
static inline uint32_t ph_i8q_scan_tile_cap(int cls) { return cls <= 7 ? 4u : (cls <= 13 ? 2u : 1u); }
static inline uint32_t ph_i8q_scan_tile_default(int cls) { return cls <= 2 ? 4u : (cls <= 7 ? 2u : 1u); }
static inline uint32_t ph_i8q_scan_tile(int cls, long long forced) {
  const uint32_t cap = ph_i8q_scan_tile_cap(cls);
  uint32_t t = ph_i8q_scan_tile_default(cls);
  if (forced > 0) t = forced >= 64 ? 4u : (forced >= 32 ? 2u : 1u);
  return t > cap ? cap : t;
}
PH_EXACT_HD static inline uint64_t ph_i8q_scan_row_tiles(uint64_t n, uint32_t tile_groups) {
  return (ph_i8q_scan_groups(n) + tile_groups - 1u) / tile_groups;
}
// 16-byte loads a thread makes for a row tile at the most (the register array of an instance)
PH_EXACT_HD static inline uint32_t ph_i8q_scan_loads(uint32_t tile_groups, uint32_t cls) {
  return (16u * tile_groups * 4u * cls + PH_I8Q_SCAN_THREADS - 1u) / PH_I8Q_SCAN_THREADS;
}

// LDS of a workgroup: two row tiles, then per wave the stages of its 16 queries, 64 sorted survivors of an insert and
// four words of state per query
PH_EXACT_HD static inline uint32_t ph_i8q_scan_tile_bytes(uint32_t steps, uint32_t tile_groups) {
  return 16u * tile_groups * ph_i8q_scan_pitch(steps);
}
PH_EXACT_HD static inline uint32_t ph_i8q_scan_wave_bytes(uint32_t r) { return 16u * ph_fp4_scan_stage(r) * 8u + 64u * 8u + 16u * 16u; }
PH_EXACT_HD static inline uint32_t ph_i8q_scan_lds(uint32_t r, uint32_t steps, uint32_t tile_groups) {
  return 2u * ph_i8q_scan_tile_bytes(steps, tile_groups) + 4u * ph_i8q_scan_wave_bytes(r);
}
PH_EXACT_HD static inline uint32_t ph_i8q_scan_merge_lds(uint32_t r) { return ph_fp4_scan_merge_lds(r); }

static inline uint64_t ph_i8q_scan_qtiles(uint64_t nq) { return (nq + PH_I8Q_SCAN_QTILE - 1u) / PH_I8Q_SCAN_QTILE; }
// slices of a launch (forced > 0: PHNSW_I8Q_SCAN_SLICES), queries of a launch and bytes of its lists: the fp4 scan's
// rules at a tile of 64 queries, the slices cutting row tiles
static inline uint32_t ph_i8q_scan_slices(uint64_t qtiles, uint64_t resident, uint64_t row_tiles, long long forced, uint32_t r) {
  return ph_fp4_scan_slices(qtiles, resident, row_tiles, forced, r, PH_I8Q_SCAN_QTILE);
}
static inline uint64_t ph_i8q_scan_chunk(uint32_t slices, uint32_t r) { return ph_fp4_scan_chunk(slices, r, PH_I8Q_SCAN_QTILE); }
static inline uint64_t ph_i8q_scan_scratch_bytes(uint64_t qtiles, uint32_t slices, uint32_t r) {
  return ph_fp4_scan_scratch_bytes(qtiles, PH_I8Q_SCAN_QTILE, slices, r);
}
