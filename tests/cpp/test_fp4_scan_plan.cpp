// The cutting rules of the exhaustive MXFP4 scan (parallel_hnsw_amd/csrc/fp4_scan_plan.h) in a stand-alone host program:
// built by g++ under AddressSanitizer and UBSan, run as a process of its own (tests/test_fp4_scan_plan_cpp.py).
// Over every r in 1 .. 1024 and every step class: the tile is 16, 32 or 64 and its LDS inside a workgroup's, the slices
// tile the row groups of n rows (n around multiples of 16) without gap or overlap, the chunk is whole tiles, never
// smaller than one, and keeps the lists under their bound; the query operand layout has a place for every block; and
// the threshold on the raw score lets no score through that the metric's last step maps at or below the r-th distance.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <random>

#include "../../parallel_hnsw_amd/csrc/fp4_scan_plan.h"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      if (failures++ < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                         \
  } while (0)

int main() {
  const uint64_t residents[] = {1, 256, 1024, 2048};
  const long long forced_tiles[] = {0, 1, 16, 33, 64, 1000}, forced_slices[] = {0, 1, 3, 1000, 1ll << 40};
  for (uint32_t ld : {4u, 8u, 32u, 100u, 104u, 128u, 132u, 256u, 768u, 1024u, 1056u, 1536u}) {
    const uint32_t steps = ph_fp4_scan_steps(ld), nb = ph_fp4_scan_blocks(ld);
    CHECK(4u * steps >= nb && 4u * (steps - 1u) < nb && ph_fp4_scan_class(steps) >= (int)steps);
    CHECK(ph_fp4_scan_scale_run(steps) >= steps && ph_fp4_scan_scale_run(steps) % 4u == 0);
    CHECK(ph_fp4_scan_code_bytes(steps) == 16u * 4u * steps);
  }
  CHECK(ph_fp4_scan_class(13) == 0);
  for (uint32_t r = 1; r <= PH_FP4_SCAN_RMAX; r++) {
    CHECK(ph_fp4_scan_r_valid(r));
    const uint32_t stage = ph_fp4_scan_stage(r);
    CHECK(stage >= 32u && stage <= 64u && stage % 16u == 0);  // a row group's 16 always fit behind stage - 16; one key a lane
    for (int cls : {2, 6, 12})
      for (long long ft : forced_tiles) {
        const uint32_t T = ph_fp4_scan_tile(cls, ft);
        CHECK(T == 16u || T == 32u || T == 64u);
        CHECK(T <= (cls == 12 ? 32u : 64u) && T <= PH_FP4_SCAN_TMAX);
        if (ft == 16 || ft == 32 || (ft == 64 && cls != 12)) CHECK(T == (uint32_t)ft);
        CHECK(ph_fp4_scan_lds(r, T) <= 64u * 1024u && ph_fp4_scan_merge_lds(r) <= 64u * 1024u);
        for (uint64_t n : {0ull, 1ull, 15ull, 16ull, 17ull, 4096ull, 4097ull, 1000000ull, 0x7FFFFFFFull}) {
          const uint64_t groups = ph_fp4_scan_groups(n);
          CHECK(groups * 16u >= n && (n == 0 || (groups - 1u) * 16u < n));
          for (uint64_t nq : {1ull, 37ull, 10000ull, 1000000ull}) {
            if ((r + cls + n + nq) % 3u && r > 64u && r < 1000u) continue;  // (the whole product is minutes under ASan)
            for (uint64_t resident : residents)
              for (long long fs : forced_slices) {
                const uint64_t first = nq < PH_FP4_SCAN_CHUNK_MAX ? nq : PH_FP4_SCAN_CHUNK_MAX;
                const uint32_t slices = ph_fp4_scan_slices(ph_fp4_scan_tiles(first, T), resident, groups, fs, r, T);
                CHECK(slices >= 1u && (slices <= groups || groups == 0));
                uint64_t at = 0;
                for (uint32_t s = 0; s < slices && slices <= 4096u; s++) {
                  uint64_t g0, g1;
                  ph_exact_slice_range(s, slices, groups, &g0, &g1);
                  CHECK(g0 == at && g1 >= g0);
                  at = g1;
                }
                if (slices <= 4096u) CHECK(at == groups);
                const uint64_t chunk = ph_fp4_scan_chunk(slices, r, T);
                CHECK(chunk >= T && chunk % T == 0 && chunk <= PH_FP4_SCAN_CHUNK_MAX);
                CHECK(ph_fp4_scan_scratch_bytes(ph_fp4_scan_tiles(chunk, T), T, slices, r) <= PH_FP4_SCAN_SCRATCH);
                CHECK(ph_fp4_scan_tiles(chunk, T) * slices < (1ull << 31));
              }
          }
        }
      }
  }
  // the threshold: d(s) <= dk implies s >= smin(dk), for both metrics, over scores around the r-th one and far from it
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<float> wide(-3000.f, 3000.f), unit(-1.f, 1.f);
  for (int half = 0; half < 2; half++)
    for (int i = 0; i < 2000000; i++) {
      const float sk = i & 1 ? wide(rng) : unit(rng) * 4.f;
      const float s = i & 2 ? std::nextafter(sk, i & 4 ? 4000.f : -4000.f) : (i & 4 ? sk + unit(rng) * 1e-3f : wide(rng));
      const volatile float ok = 1.0f - sk, os = 1.0f - s;
      const float dk = half ? ok / 2.0f : ok, d = half ? os / 2.0f : os;
      if (d <= dk) CHECK(s >= ph_fp4_scan_smin(dk, half != 0));
      CHECK(ph_fp4_scan_smin(dk, half != 0) <= sk);
    }
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("ALL OK\n");
  return 0;
}
