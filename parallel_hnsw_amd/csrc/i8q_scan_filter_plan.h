// The integer rules the filtered int8 scan (scan_i8q_filtered.hip) adds to i8q_scan_plan.h.  The bitmap, the compacted
// row list of a shared bitmap and its scratch `pre` are fp4_scan_filter_plan.h's, unchanged; what is new is that a ROW
// TILE of the LIST form is 16, 32 or 64 list positions while the list is padded to 16 only.  Shared by the launcher, the
// kernels and tests/cpp/test_i8q_scan_filter_plan.cpp (host sanitizers, no GPU).
//
//   position  = an index into the ascending list of the m allowed rows; row tile t of the LIST form is positions
//               T t .. T t + T - 1 (T = 16 tile_groups), cut over ceil(m / T) tiles
//   clamp     = a position becomes a row address only through ph_i8q_scan_list_pos: positions at or past m read entry
//               m - 1, the last allowed row.  Entries at or past ph_fp4_scan_list_len(m) are unwritten scratch and are
//               never read; a position at or past m is never a key
//   id ring   = the ids of a tile's rows in LDS, one u32 a row, behind everything i8q_scan_plan.h lays out: four slots
//               of 16 tile_groups words.  Tile t lives in slot t & 3.  Slot t + 1 is written before the barrier of tile
//               t while a slow wave may still read slot t - 1 and every wave is about to read slot t: three are live,
//               the fourth makes the slot a mask
#pragma once
#include <stdint.h>

#include "fp4_scan_filter_plan.h"
#include "i8q_scan_plan.h"

#define PH_I8Q_SCAN_ID_SLOTS 4u

// the list entry position p of a list of m > 0 rows reads
PH_EXACT_HD static inline uint64_t ph_i8q_scan_list_pos(uint64_t p, uint64_t m) { return p < m ? p : m - 1u; }
// row tiles of the LIST form: over the m listed rows
PH_EXACT_HD static inline uint64_t ph_i8q_scan_list_tiles(uint64_t m, uint32_t tile_groups) { return ph_i8q_scan_row_tiles(m, tile_groups); }
PH_EXACT_HD static inline uint32_t ph_i8q_scan_ids_bytes(uint32_t tile_groups) { return PH_I8Q_SCAN_ID_SLOTS * 16u * tile_groups * 4u; }
PH_EXACT_HD static inline uint32_t ph_i8q_scan_ids_slot(uint64_t tile) { return (uint32_t)tile & (PH_I8Q_SCAN_ID_SLOTS - 1u); }
// LDS of a LIST workgroup: ph_i8q_scan_lds, then the id ring (16-byte aligned: every term before it is)
PH_EXACT_HD static inline uint32_t ph_i8q_scan_list_lds(uint32_t r, uint32_t steps, uint32_t tile_groups) {
  return ph_i8q_scan_lds(r, steps, tile_groups) + ph_i8q_scan_ids_bytes(tile_groups);
}
