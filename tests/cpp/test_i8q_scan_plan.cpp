// The cutting rules of the exhaustive int8 scan (parallel_hnsw_amd/csrc/i8q_scan_plan.h) in a stand-alone host program:
// built by g++ under AddressSanitizer and UBSan, run as a process of its own (tests/test_i8q_scan_plan_cpp.py).
// Over every row length up to 1536: the runs cover the image and fit the stored stride, the steps cover the runs, a
// class exists, the pitch is an odd count of runs that holds every run a step reads.  Over every r and class: the row
// tile is 1, 2 or 4 groups inside its cap, the staging registers of the instance cover it, the LDS fits a workgroup's,
// the slices tile the row tiles without gap or overlap, the chunk is whole query tiles and keeps the lists in bound.
#include <cstdio>
#include <initializer_list>

#include "../../parallel_hnsw_amd/csrc/i8q_scan_plan.h"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      if (failures++ < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                         \
  } while (0)

int main() {
  for (uint32_t ld = 4; ld <= PH_I8Q_SCAN_LD_MAX; ld += 4) {
    const uint32_t runs = ph_i8q_scan_runs(ld), steps = ph_i8q_scan_steps(ld), stride = (4u + ld + 15u) & ~15u;  // rowstore.hip
    const int cls = ph_i8q_scan_class(steps);
    CHECK(16u * runs >= 4u + ld && 16u * (runs - 1u) < 4u + ld && 16u * runs == stride);
    CHECK(4u * steps >= runs && 4u * (steps - 1u) < runs && cls >= (int)steps);
    CHECK(ph_i8q_scan_query_bytes(steps) == 64u * steps && ph_i8q_scan_query_bytes(steps) >= 4u + ld);
    const uint32_t pitch = ph_i8q_scan_pitch(steps);
    CHECK(pitch % 16u == 0 && (pitch / 16u) % 2u == 1u && pitch >= 64u * steps && pitch >= stride);
    CHECK((uint64_t)1536u * 127u * 127u < (1ull << 31));  // the accumulator
  }
  CHECK(ph_i8q_scan_class(26) == 0 && ph_i8q_scan_steps(PH_I8Q_SCAN_LD_MAX) == 25u);
  const uint64_t residents[] = {1, 256, 1024};
  const long long forced_tiles[] = {0, 1, 16, 33, 64, 1000}, forced_slices[] = {0, 1, 5, 16, 1000, 1ll << 40};
  for (uint32_t r = 1; r <= PH_I8Q_SCAN_RMAX; r++) {
    CHECK(ph_i8q_scan_r_valid(r));
    for (int cls : {2, 7, 13, 25})
      for (long long ft : forced_tiles) {
        const uint32_t tg = ph_i8q_scan_tile(cls, ft), cap = ph_i8q_scan_tile_cap(cls);
        CHECK((tg == 1u || tg == 2u || tg == 4u) && tg <= cap && ph_i8q_scan_tile_default(cls) <= cap);
        if (ft == 16 || (ft == 32 && cap >= 2u) || (ft == 64 && cap >= 4u)) CHECK(16u * tg == (uint32_t)ft);
        // every run of the largest tile has a (thread, round) of the instance compiled for the cap
        CHECK(ph_i8q_scan_loads(cap, cls) * PH_I8Q_SCAN_THREADS >= 16u * tg * 4u * cls);
        CHECK(ph_i8q_scan_lds(r, cls, tg) <= 160u * 1024u && ph_i8q_scan_merge_lds(r) <= 64u * 1024u);
        CHECK(ph_i8q_scan_tile_bytes(cls, tg) % 16u == 0 && ph_i8q_scan_wave_bytes(r) % 8u == 0);
        if ((r + cls) % 5u && r > 64u && r < 1000u) continue;  // (the whole product is minutes under ASan)
        for (uint64_t n : {0ull, 1ull, 16ull, 17ull, 4097ull, 1000000ull, 0x7FFFFFFFull}) {
          const uint64_t row_tiles = ph_i8q_scan_row_tiles(n, tg);
          CHECK(row_tiles * 16u * tg >= n && (n == 0 || (row_tiles - 1u) * 16u * tg < n));
          for (uint64_t nq : {1ull, 70ull, 10000ull, 1000000ull})
            for (uint64_t resident : residents)
              for (long long fs : forced_slices) {
                const uint64_t first = nq < PH_FP4_SCAN_CHUNK_MAX ? nq : PH_FP4_SCAN_CHUNK_MAX;
                const uint32_t slices = ph_i8q_scan_slices(ph_i8q_scan_qtiles(first), resident, row_tiles, fs, r);
                CHECK(slices >= 1u && (slices <= row_tiles || row_tiles == 0));
                uint64_t at = 0;
                for (uint32_t s = 0; s < slices && slices <= 4096u; s++) {
                  uint64_t t0, t1;
                  ph_exact_slice_range(s, slices, row_tiles, &t0, &t1);
                  CHECK(t0 == at && t1 >= t0);
                  at = t1;
                }
                if (slices <= 4096u) CHECK(at == row_tiles);
                const uint64_t chunk = ph_i8q_scan_chunk(slices, r);
                CHECK(chunk >= PH_I8Q_SCAN_QTILE && chunk % PH_I8Q_SCAN_QTILE == 0 && chunk <= PH_FP4_SCAN_CHUNK_MAX);
                CHECK(ph_i8q_scan_scratch_bytes(ph_i8q_scan_qtiles(chunk), slices, r) <= PH_FP4_SCAN_SCRATCH);
                CHECK(ph_i8q_scan_qtiles(chunk) * slices < (1ull << 31));
              }
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
