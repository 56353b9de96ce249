// Stand-alone host check of the integer rules behind the exact search by row label (parallel_hnsw_amd/csrc/label_plan.h,
// the header the launcher and the kernels include): compiled with -fsanitize=address,undefined and run without a GPU
// (tests/test_label_plan_cpp.py).  Slice ranges over a list's 64-id batches, the tile size T and its LDS, the slot of a
// wanted label, a host model of the tile cut over sorted slots, and the scratch sizes at the largest batch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/label_plan.h"

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

static const uint32_t NONE = 0xFFFFFFFFu;

static void test_slices() {
  const uint64_t lens[] = {0, 1, 63, 64, 65, 2048, 2049};
  for (uint64_t len : lens) {
    const uint64_t nb = ph_label_batches(len);
    CHECK(nb * 64u >= len && (nb == 0 || (nb - 1u) * 64u < len));
    for (uint32_t slices = 1; slices <= 9; slices++) {
      std::vector<uint32_t> seen(len, 0u);  // every id of the list, counted as the kernels index it
      uint64_t next = 0;
      for (uint32_t s = 0; s < slices; s++) {
        uint64_t b0, b1;
        ph_label_slice_range(s, slices, len, &b0, &b1);
        CHECK(b0 == next && b1 >= b0 && b1 <= nb);  // no gap, no overlap
        next = b1;
        for (uint64_t b = b0; b < b1; b++) {
          CHECK(b * 64u < len);  // a batch of the range holds at least one id: m >= 1 in the tile kernel
          for (uint32_t lane = 0; lane < 64u; lane++)
            if (b * 64u + lane < len) seen[b * 64u + lane]++;
        }
      }
      CHECK(next == nb);
      for (uint32_t c : seen) CHECK(c == 1u);
    }
    // the slice count never exceeds the batches and is never 0
    for (long long forced : {0ll, 1ll, 3ll, 7ll, 1000ll})
      for (uint64_t items : {1ull, 10ull, 100000ull}) {
        const uint32_t s = ph_label_slice_count(items, 2048, len, forced);
        CHECK(s >= 1u && (nb == 0 ? s == 1u : s <= nb));
        if (forced > 0 && nb) CHECK(s == std::min<uint64_t>((uint64_t)forced, nb));
      }
  }
  CHECK(ph_label_slice_count(10000, 2048, 10000, 0) == 1u);  // the queries alone fill the device
  CHECK(ph_label_slice_count(8, 2048, 100000, 0) == 256u);
}

static void test_tile_size() {
  const uint64_t ks[] = {1, 10, 64, 1024};
  const uint64_t lds[] = {256, 768, 1536};  // NV 1 / 3 / 6
  for (uint64_t ld : lds) {
    uint32_t before = 0xFFFFFFFFu;
    for (uint64_t k : ks) {
      for (long long knob : {0ll, 1ll, 3ll, 1000ll}) {
        const uint32_t T = ph_label_tile(k, ld, PH_LABEL_LDS_BYTES, knob);
        CHECK(T >= 1u);
        if (knob > 0) CHECK(T <= (uint32_t)knob);
        if (knob == 0) CHECK(T <= PH_LABEL_TILE_CAP);
        if (T > 1u) CHECK(ph_label_tile_lds(T, k, ld) <= PH_LABEL_LDS_BYTES);
        if (T > 1u) CHECK(ph_label_tile_lds(T, k, ld) * PH_LABEL_TILE_WAVES <= PH_LABEL_LDS_BYTES);
      }
      CHECK(ph_label_scan_lds(k) <= PH_LABEL_LDS_BYTES);  // T = 1: the per-query scan's own LDS
      const uint32_t T = ph_label_tile(k, ld, PH_LABEL_LDS_BYTES, 1000);
      CHECK(T <= before);  // monotone: never grows with k
      before = T;
    }
  }
  for (uint64_t k : ks) CHECK(ph_label_tile(k, 1536, PH_LABEL_LDS_BYTES, 0) <= ph_label_tile(k, 256, PH_LABEL_LDS_BYTES, 0));
  CHECK(ph_label_tile(10, 768, PH_LABEL_LDS_BYTES, 0) == 10u);  // 40 960 / (3072 + 672 + 256 + 16)
  CHECK(ph_label_tile(10, 768, PH_LABEL_LDS_BYTES, 1) == 1u);
  CHECK(ph_label_tile(1024, 1536, PH_LABEL_LDS_BYTES, 0) == 1u);
  // the layout the kernel carves: rows, key lists (8-byte aligned), distances, state -- inside the figure
  for (uint64_t ld : lds)
    for (uint64_t k : ks) {
      const uint64_t T = ph_label_tile(k, ld, PH_LABEL_LDS_BYTES, 0);
      const uint64_t keys_at = T * ld * 4u, dbuf_at = keys_at + T * (2u * k + 64u) * 8u, state_at = dbuf_at + T * 64u * 4u;
      CHECK(keys_at % 16u == 0 && dbuf_at % 8u == 0);
      CHECK(state_at + T * 16u == ph_label_tile_lds(T, k, ld));
    }
}

static void test_slots() {
  const std::vector<uint32_t> values = {0u, 5u, 7u, 0x7FFFFFFFu, 0xFFFFFFFEu};
  for (uint32_t i = 0; i < values.size(); i++) CHECK(ph_label_slot(values.data(), values.size(), values[i], NONE) == i);
  for (uint32_t w : {1u, 6u, 8u, 0x80000000u, 0xFFFFFFFDu}) CHECK(ph_label_slot(values.data(), values.size(), w, NONE) == PH_LABEL_SLOT_NONE);
  CHECK(ph_label_slot(values.data(), values.size(), NONE, NONE) == PH_LABEL_SLOT_NONE);
  CHECK(ph_label_slot(nullptr, 0, 3u, NONE) == PH_LABEL_SLOT_NONE);  // no label at all: nothing is read
}

// every query in exactly one tile, no tile across two labels, none above T
static void model_tiles(const std::vector<uint32_t> &group_sizes, uint32_t T) {
  std::vector<uint32_t> sslot;
  uint32_t slot = 3;
  for (uint32_t g : group_sizes) {
    for (uint32_t i = 0; i < g; i++) sslot.push_back(slot);
    slot += 2;
  }
  for (uint32_t i = 0; i < 3; i++) sslot.push_back(PH_LABEL_SLOT_NONE);  // absent labels sort last and tile like a group
  const uint64_t nq = sslot.size();
  std::vector<uint32_t> flags(nq + 1u), tidx(nq + 1u), tile_first(nq, 0xDEADu), covered(nq, 0u);
  for (uint64_t p = 0; p <= nq; p++) flags[p] = p < nq && ph_label_tile_head(sslot.data(), p, T) ? 1u : 0u;
  uint32_t run = 0;
  for (uint64_t p = 0; p <= nq; p++) tidx[p] = run, run += flags[p];
  const uint32_t ntiles = tidx[nq];
  CHECK(ntiles <= nq && ntiles >= (nq + T - 1u) / T);
  for (uint64_t p = 0; p < nq; p++)
    if (flags[p]) {
      CHECK(tidx[p] < ntiles);
      tile_first[tidx[p]] = (uint32_t)p;
    }
  uint64_t expect_tiles = 0;
  for (uint32_t g : group_sizes) expect_tiles += (g + T - 1u) / T;
  expect_tiles += (3u + T - 1u) / T;
  CHECK(ntiles == expect_tiles);
  for (uint32_t t = 0; t < ntiles; t++) {
    const uint32_t p0 = tile_first[t];
    CHECK(p0 < nq);
    const uint32_t tsz = ph_label_tile_size(sslot.data(), nq, p0, T);
    CHECK(tsz >= 1u && tsz <= T && p0 + tsz <= nq);
    for (uint32_t i = 0; i < tsz; i++) {
      CHECK(sslot[p0 + i] == sslot[p0]);
      covered[p0 + i]++;
    }
    if (t) CHECK(tile_first[t - 1u] < p0);  // label-major, in position order
  }
  for (uint32_t c : covered) CHECK(c == 1u);
}

static void test_tiles() {
  for (uint32_t T : {1u, 2u, 3u, 10u, 16u}) {
    model_tiles({1u, T, T + 1u, 2u * T + 1u}, T);
    model_tiles({2u * T + 1u, 1u, 1u, T}, T);
    model_tiles({65u}, T);
    model_tiles({}, T);
  }
}

static void test_scratch() {
  const uint64_t nq = PH_LABEL_NQ_MAX;  // 2^31 - 2
  const PhLabelPre l = ph_label_pre(nq);
  CHECK(l.head == 0 && l.slot == 4u && l.sslot == l.slot + nq && l.iota == l.sslot + nq && l.order == l.iota + nq);
  CHECK(l.tile_first == l.order + nq && l.flags == l.tile_first + nq && l.tidx == l.flags + nq + 1u);
  CHECK(l.words == 7u * nq + 6u && l.words > 0xFFFFFFFFull);  // counted in 64 bits
  CHECK(l.words * 4u / 4u == l.words);
  uint64_t bytes = 0;
  CHECK(ph_label_key_bytes(nq, 1, 1024, &bytes) && bytes == nq * 8192u);
  CHECK(ph_label_key_bytes(nq, 9, 10, &bytes) && bytes == nq * 720u);
  CHECK(ph_label_key_bytes(nq, 0xFFFFFFFFull, 1024, &bytes) == false);  // past 64 bits: refused, not wrapped
  CHECK(ph_label_key_bytes(nq + 1u, 1, 10, &bytes) == false);
  CHECK(ph_label_key_bytes(10, 1, 1025, &bytes) == false);
  CHECK(ph_label_key_bytes(0, 4, 10, &bytes) && bytes == 0);
  const PhLabelPre s = ph_label_pre(1);
  CHECK(s.words == 13u);
}

int main() {
  test_slices();
  test_tile_size();
  test_slots();
  test_tiles();
  test_scratch();
  std::printf("ALL OK\n");
  return 0;
}
