// The integer rules the filtered int8 scan adds (parallel_hnsw_amd/csrc/i8q_scan_filter_plan.h) in a stand-alone host
// program: built by g++ under AddressSanitizer and UBSan, run as a process of its own
// (tests/test_i8q_scan_filter_plan_cpp.py).  The LIST form is replayed on the host over a list allocated at exactly
// ph_fp4_scan_list_len(m) entries, so a position that escaped the clamp is a heap overflow ASan reports: every tile of
// every slice reads only written entries, every position below m is read exactly once as itself, none at or past m can
// be a key.  The tile count follows m; the LDS with the id ring fits a workgroup and keeps the ring 16-byte aligned.
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/i8q_scan_filter_plan.h"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      if (failures++ < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                         \
  } while (0)

int main() {
  for (uint32_t tg : {1u, 2u, 4u}) {
    const uint32_t T = 16u * tg;
    for (uint64_t m = 0; m <= 300; m++) {
      const uint64_t tiles = ph_i8q_scan_list_tiles(m, tg);
      CHECK(tiles * T >= m && (m == 0 || (tiles - 1u) * T < m) && (m != 0 || tiles == 0));
      std::vector<uint32_t> list(ph_fp4_scan_list_len(m));  // what the compaction writes, and not a word more
      for (uint64_t p = 0; p < list.size(); p++) list[p] = 1000u + (uint32_t)(p < m ? p : m - 1u);
      for (uint32_t slices : {1u, 3u, 7u}) {
        std::vector<uint32_t> seen(m, 0u);
        uint64_t at = 0;
        for (uint32_t s = 0; s < slices; s++) {
          uint64_t t0, t1;
          ph_exact_slice_range(s, slices, tiles, &t0, &t1);
          CHECK(t0 == at && t1 >= t0);
          at = t1;
          for (uint64_t t = t0; t < t1; t++)
            for (uint32_t r = 0; r < T; r++) {
              const uint64_t p = t * T + r, c = ph_i8q_scan_list_pos(p, m);
              CHECK(c < m && c < list.size() && (p >= m || c == p));
              const uint32_t id = list[c];  // the row address; ASan sees an escape
              CHECK(id == 1000u + (uint32_t)c);
              if (p < m) seen[p]++;  // the key rule: a position at or past m is never one
            }
        }
        CHECK(at == tiles);
        for (uint64_t p = 0; p < m; p++) CHECK(seen[p] == 1u);
      }
    }
    CHECK(ph_i8q_scan_ids_bytes(tg) == PH_I8Q_SCAN_ID_SLOTS * T * 4u);
  }
  // three slots are live at a time (i8q_scan_filter_plan.h): consecutive tiles never share one
  for (uint64_t t = 0; t < 64; t++)
    CHECK(ph_i8q_scan_ids_slot(t) < PH_I8Q_SCAN_ID_SLOTS && ph_i8q_scan_ids_slot(t) != ph_i8q_scan_ids_slot(t + 1u) &&
          ph_i8q_scan_ids_slot(t) != ph_i8q_scan_ids_slot(t + 2u) && ph_i8q_scan_ids_slot(t + 1u) != ph_i8q_scan_ids_slot(t + 2u));
  for (uint32_t r = 1; r <= PH_I8Q_SCAN_RMAX; r++)
    for (int cls : {2, 7, 13, 25})
      for (uint32_t tg = 1; tg <= ph_i8q_scan_tile_cap(cls); tg *= 2u) {
        const uint32_t plain = ph_i8q_scan_lds(r, cls, tg), lds = ph_i8q_scan_list_lds(r, cls, tg);
        CHECK(lds == plain + ph_i8q_scan_ids_bytes(tg) && plain % 16u == 0 && lds <= 160u * 1024u);
      }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
