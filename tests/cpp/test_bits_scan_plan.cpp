// The cutting rules of the exhaustive Hamming scan (parallel_hnsw_amd/csrc/bits_scan_plan.h) in a stand-alone host
// program: built by g++ under AddressSanitizer and UBSan, run as a process of its own (tests/test_bits_scan_plan_cpp.py).
// Over every r in 1 .. 1024 and NV in {1, 3, 6}: the tile is 1 .. 16 and its LDS inside the budget, the slices tile the
// batches of n rows (n around multiples of 64) without gap or overlap, and the chunk rule keeps the per-slice lists
// under their bound.
#include <cstdio>
#include <initializer_list>

#include "../../parallel_hnsw_amd/csrc/bits_plan.h"
#include "../../parallel_hnsw_amd/csrc/bits_scan_plan.h"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      if (failures++ < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                         \
  } while (0)

int main() {
  const uint64_t residents[] = {1, 256, 1024, 2048};
  const long long forced_tiles[] = {0, 1, 5, 16, 1000}, forced_slices[] = {0, 1, 3, 1000, 1ll << 40};
  for (uint32_t r = 1; r <= PH_BITS_SCAN_RMAX; r++) {
    CHECK(ph_bits_scan_r_valid(r));
    for (long long ft : forced_tiles) {
      const uint32_t T = ph_bits_scan_tile(r, ft);
      CHECK(T >= 1u && T <= PH_BITS_SCAN_TMAX);
      // the rule's own tile stays inside one budget; a forced one inside the workgroup's LDS
      CHECK(ph_bits_scan_lds(r, T) <= (ft ? 4u : 1u) * PH_BITS_SCAN_LDS || T == 1u);
      CHECK(ph_bits_scan_lds(r, T) <= 160u * 1024u);
      CHECK(ph_bits_scan_merge_lds(r) <= ph_bits_scan_query_lds(r));
      if (ft > 0 && ft <= 16 && ph_bits_scan_lds(r, (uint32_t)ft) <= 4u * PH_BITS_SCAN_LDS) CHECK(T == (uint32_t)ft);
      for (int nv : {1, 3, 6}) {
        const uint32_t dim = nv == 1 ? 256u : (nv == 3 ? 768u : 1536u);
        CHECK(ph_bits_class(dim) == nv && ph_bits_stride_words(nv) * 32u >= dim);
        for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 4096ull, 4097ull, 1000000ull, 0x7FFFFFFFull}) {
          const uint64_t batches = ph_bits_scan_batches(n);
          CHECK(batches * 64u >= n && (n == 0 || (batches - 1u) * 64u < n));
          for (uint64_t nq : {1ull, 37ull, 10000ull, 1000000ull}) {
            if ((r + nv + n + nq) % 3u && r > 64u && r < 1000u) continue;  // (the whole product is minutes under ASan)
            for (uint64_t resident : residents)
              for (long long fs : forced_slices) {
                const uint64_t first = nq < PH_BITS_SCAN_CHUNK_MAX ? nq : PH_BITS_SCAN_CHUNK_MAX;
                const uint32_t slices = ph_bits_scan_slices(ph_bits_scan_tiles(first, T), resident, batches, fs, r, T);
                CHECK(slices >= 1u && (slices <= batches || batches == 0));
                uint64_t at = 0;
                for (uint32_t s = 0; s < slices && slices <= 4096u; s++) {
                  uint64_t b0, b1;
                  ph_exact_slice_range(s, slices, batches, &b0, &b1);
                  CHECK(b0 == at && b1 >= b0);
                  at = b1;
                }
                if (slices <= 4096u) CHECK(at == batches);
                const uint64_t chunk = ph_bits_scan_chunk(slices, r, T);
                CHECK(chunk >= T && chunk % T == 0 && chunk <= PH_BITS_SCAN_CHUNK_MAX);
                CHECK(ph_bits_scan_scratch_bytes(chunk, slices, r) <= PH_BITS_SCAN_SCRATCH);
                CHECK(ph_bits_scan_tiles(chunk, T) * slices <= (1ull << 23) || slices == 1u);
                CHECK(ph_bits_scan_tiles(chunk, T) * slices < (1ull << 31));
              }
          }
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
