// The integer rules of the exact radius search over lists (parallel_hnsw_amd/csrc/list_radius_plan.h) under the host
// sanitizers: the pool's records against a 128-bit restatement (0 and products near 2^63 and past 2^64 among them), the
// layout with no table block, and the staging buffer -- its flush arithmetic at 0, 1, buffer - 1, buffer and buffer + 1
// hits, and a host model of an item (stage, flush with one add on the cursor, write below the capacity, drop but count
// the rest) over arrays of EXACTLY the sizes the kernel and the launcher use, so that an index past any of them is an
// AddressSanitizer report.  No GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/label_plan.h"
#include "../../parallel_hnsw_amd/csrc/list_radius_plan.h"

#define CHECK(x)                                                         \
  do {                                                                   \
    if (!(x)) {                                                          \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

typedef unsigned __int128 u128;

static void check_records(uint64_t cap, uint64_t nq, uint64_t longest) {
  const uint64_t rec = ph_list_radius_pool_records(cap, nq, longest);
  const u128 pairs = (u128)nq * longest;
  CHECK((u128)rec == ((u128)cap < pairs ? (u128)cap : pairs));
  CHECK(rec <= cap && (cap != 0 || rec == 0) && (nq != 0 || rec == 0) && (longest != 0 || rec == 0));
  if (ph_radius_cap_valid(cap)) CHECK(rec <= 0x7FFFFFFFull);  // the sort counts in int
  if (pairs < ((u128)1 << 64)) CHECK(rec == ph_radius_pool_records(cap, nq, longest));  // where that rule's product fits: one rule
  if (!ph_radius_cap_valid(cap) && rec > 0x7FFFFFFFull) return;  // (refused before a layout is made)
  const PhRadiusLayout l = ph_list_radius_layout(nq > 0xFFFFFFFFull ? 0xFFFFFFFFull : nq, rec);
  const uint64_t lnq = nq > 0xFFFFFFFFull ? 0xFFFFFFFFull : nq;
  const uint64_t off[] = {l.head, l.count, l.keys_a, l.keys_b, l.q_a, l.q_b, l.table, l.bytes};
  const u128 size[] = {(u128)PH_RADIUS_HEAD_WORDS * 8, ((u128)lnq + 1) * 4, (u128)rec * 8, (u128)rec * 8, (u128)rec * 4,
                       (u128)rec * 4, 0};
  CHECK(l.head == 0);
  for (int i = 0; i < 7; i++) {  // in order, 16-byte aligned, each block at least its size, no overlap
    CHECK(off[i] % 16u == 0);
    CHECK((u128)off[i] + size[i] <= (u128)off[i + 1]);
    CHECK((u128)off[i + 1] < (u128)off[i] + size[i] + 16);
  }
  CHECK(l.table == l.bytes);  // no table block: the pool ends the scratch
}

// the flush arithmetic for a run of batches bringing `per` hits each until `hits` are in
static void check_flushes(uint64_t hits, uint32_t per) {
  std::vector<uint32_t> h;
  for (uint64_t left = hits; left;) {
    const uint32_t c = (uint32_t)std::min<uint64_t>(left, per);
    h.push_back(c), left -= c;
  }
  const PhListRadiusFlushes f = ph_list_radius_flushes(h.data(), h.size());
  CHECK(f.total == hits && f.largest <= PH_LIST_RADIUS_STAGE);
  CHECK((f.flushes == 0) == (hits == 0));
  if (PH_LIST_RADIUS_STAGE % per == 0) {  // full buffers, then the rest
    CHECK(f.flushes == (hits + PH_LIST_RADIUS_STAGE - 1) / PH_LIST_RADIUS_STAGE);
    CHECK(f.largest == (uint32_t)std::min<uint64_t>(hits, PH_LIST_RADIUS_STAGE));
  } else {  // a batch is never split: a flush carries at least buffer - per + 1 keys unless it is the last
    CHECK(f.flushes >= (hits + PH_LIST_RADIUS_STAGE - 1) / PH_LIST_RADIUS_STAGE);
    CHECK(f.flushes <= hits / (PH_LIST_RADIUS_STAGE - per + 1u) + 1u);
  }
}

// One call on the host: per query a list of `len[q]` ids cut into slices, the items in an order a seed decides (the
// waves' order is not fixed), a staging buffer of exactly PH_LIST_RADIUS_STAGE keys per item, a pool of exactly the
// layout's size; then the two stable sorts.
static uint64_t model_call(const std::vector<uint32_t> &len, uint32_t slices, uint64_t cap, uint32_t density, uint32_t seed) {
  std::mt19937 rng(seed);
  const uint64_t nq = len.size();
  uint64_t longest = 0;
  for (uint32_t v : len) longest = std::max<uint64_t>(longest, v);
  const uint64_t rec = ph_list_radius_pool_records(cap, nq, longest);
  const PhRadiusLayout l = ph_list_radius_layout(nq, rec);
  std::vector<unsigned char> post(l.bytes);
  uint64_t *const cursor = (uint64_t *)(post.data() + l.head);
  uint32_t *const count = (uint32_t *)(post.data() + l.count);
  uint64_t *const keys = (uint64_t *)(post.data() + l.keys_a);
  uint32_t *const qs = (uint32_t *)(post.data() + l.q_a);
  *cursor = 0;
  for (uint64_t q = 0; q <= nq; q++) count[q] = 0;
  // in[q][j]: whether entry j of query q's list is inside its radius; the key of a hit: (a small distance, the id)
  std::vector<std::vector<uint64_t>> key(nq);
  std::vector<std::vector<bool>> in(nq);
  for (uint64_t q = 0; q < nq; q++)
    for (uint32_t j = 0; j < len[q]; j++) {
      key[q].push_back(((uint64_t)(rng() % 5u) << 32) | (uint32_t)(7u * j + q));
      in[q].push_back(rng() % 100u < density);
    }
  std::vector<uint64_t> items(nq * slices);
  for (uint64_t i = 0; i < items.size(); i++) items[i] = i;
  std::shuffle(items.begin(), items.end(), rng);
  uint64_t atomics = 0;
  for (uint64_t item : items) {
    const uint64_t q = item % nq;
    const uint32_t slice = (uint32_t)(item / nq);
    uint64_t b0, b1;
    ph_label_slice_range(slice, slices, len[q], &b0, &b1);
    std::vector<uint64_t> stage(PH_LIST_RADIUS_STAGE);
    uint32_t staged = 0, cnt = 0;
    auto flush = [&]() {
      uint64_t slot = *cursor;
      *cursor += staged, atomics++;
      for (uint32_t i = 0; i < staged; i++, slot++)
        if (slot < rec) keys[slot] = stage[i], qs[slot] = (uint32_t)q;
      staged = 0;
    };
    for (uint64_t b = b0; b < b1; b++) {
      uint32_t hits = 0;
      for (uint32_t lane = 0; lane < 64u; lane++) {
        const uint64_t j = b * PH_LABEL_BATCH + lane;
        hits += j < len[q] && in[q][j];
      }
      cnt += hits;
      if (!rec || !hits) continue;
      if (ph_list_radius_flush_first(staged, hits)) flush();
      for (uint32_t lane = 0; lane < 64u; lane++) {
        const uint64_t j = b * PH_LABEL_BATCH + lane;
        if (j < len[q] && in[q][j]) stage[staged++] = key[q][j];  // an index past the buffer is an ASan report
      }
    }
    if (!cnt) continue;
    if (staged) flush();
    if (!rec) *cursor += cnt;
    count[q] += cnt;
  }
  std::vector<std::vector<uint64_t>> want(nq);
  uint64_t total = 0;
  for (uint64_t q = 0; q < nq; q++) {
    for (uint32_t j = 0; j < len[q]; j++)
      if (in[q][j]) want[q].push_back(key[q][j]);
    std::sort(want[q].begin(), want[q].end());
    CHECK(count[q] == want[q].size());
    total += want[q].size();
  }
  CHECK(*cursor == total && count[nq] == 0);  // exact whatever the capacity and the slice count
  if (rec) CHECK(atomics <= nq * slices * (longest / (PH_LIST_RADIUS_STAGE - PH_LIST_RADIUS_BATCH + 1u) + 1u));
  if (!ph_radius_emits(total, cap)) return total;
  CHECK(total <= rec);  // nothing was dropped
  std::vector<uint64_t> perm(total);
  for (uint64_t i = 0; i < total; i++) perm[i] = i;
  std::stable_sort(perm.begin(), perm.end(), [&](uint64_t a, uint64_t b) { return keys[a] < keys[b]; });
  std::stable_sort(perm.begin(), perm.end(), [&](uint64_t a, uint64_t b) { return qs[a] < qs[b]; });
  uint64_t at = 0;
  for (uint64_t q = 0; q < nq; q++)
    for (uint64_t k : want[q]) {
      CHECK(qs[perm[at]] == q && keys[perm[at]] == k);
      at++;
    }
  CHECK(at == total);
  return total;
}

int main() {
  const uint64_t caps[] = {0, 1, 63, 64, 65, 1000, 0x7FFFFFFFull, 0x80000000ull, ~0ull};
  const uint64_t nqs[] = {0, 1, 2, 65, 10000, 0x7FFFFFFEull, 0xFFFFFFFFull, 1ull << 32, 3037000499ull, 3037000500ull};
  const uint64_t longs[] = {0, 1, 64, 5000, 0x7FFFFFFFull, 0xFFFFFFFFull, 3037000499ull, 3037000500ull, 1ull << 62, ~0ull};
  for (uint64_t cap : caps)
    for (uint64_t nq : nqs)
      for (uint64_t c : longs) check_records(cap, nq, c);
  // products at 2^63 - small, 2^63, 2^64 - 1 and past 2^64: the rule saturates, it does not wrap
  CHECK(ph_list_radius_pool_records(~0ull, 1ull << 31, 1ull << 32) == 1ull << 63);
  CHECK(ph_list_radius_pool_records(~0ull, 0xFFFFFFFFull, 0xFFFFFFFFull) == 0xFFFFFFFE00000001ull);
  CHECK(ph_list_radius_pool_records(~0ull, 1ull << 32, 1ull << 32) == ~0ull);
  CHECK(ph_list_radius_pool_records(77, 1ull << 32, 1ull << 32) == 77);
  CHECK(ph_list_radius_pool_records(77, 0, 5) == 0 && ph_list_radius_pool_records(77, 5, 0) == 0);

  // the staging buffer
  const uint32_t S = PH_LIST_RADIUS_STAGE;
  CHECK(S >= PH_LIST_RADIUS_BATCH && PH_LIST_RADIUS_BATCH == PH_LABEL_BATCH);
  CHECK(!ph_list_radius_flush_first(0, 0) && !ph_list_radius_flush_first(0, 64) && !ph_list_radius_flush_first(S - 64, 64));
  CHECK(ph_list_radius_flush_first(S - 63, 64) && !ph_list_radius_flush_first(S - 1, 1) && ph_list_radius_flush_first(S, 1));
  CHECK(!ph_list_radius_flush_first(S, 0));
  const uint64_t hit_counts[] = {0, 1, S - 1u, S, S + 1u, 2u * S, 2u * S + 1u, 10u * S - 1u};
  for (uint64_t hits : hit_counts)
    for (uint32_t per : {1u, 3u, 63u, 64u}) check_flushes(hits, per);
  {
    const uint32_t none[] = {0, 0, 0};
    CHECK(ph_list_radius_flushes(none, 3).flushes == 0 && ph_list_radius_flushes(none, 0).flushes == 0);
    const uint32_t one[] = {0, 1, 0};
    const PhListRadiusFlushes f1 = ph_list_radius_flushes(one, 3);
    CHECK(f1.flushes == 1 && f1.total == 1 && f1.largest == 1);
    const uint32_t full[] = {64, 64, 64, 64};  // exactly the buffer: one flush, at the end
    const PhListRadiusFlushes ff = ph_list_radius_flushes(full, 4);
    CHECK(ff.flushes == 1 && ff.largest == S);
    const uint32_t over[] = {64, 64, 64, 64, 1};  // one more: the buffer first, then the one
    const PhListRadiusFlushes fo = ph_list_radius_flushes(over, 5);
    CHECK(fo.flushes == 2 && fo.largest == S && fo.total == S + 1);
    const uint32_t under[] = {64, 64, 64, 63, 1};  // buffer - 1, then 1: they share a flush
    CHECK(ph_list_radius_flushes(under, 5).flushes == 1);
  }

  uint32_t seed = 1;
  const std::vector<uint32_t> lens = {0, 1, 63, 64, 65, 255, 256, 257, 1000, 5000};
  for (uint32_t slices : {1u, 3u, 16u})
    for (uint32_t density : {0u, 1u, 30u, 100u})
      for (uint64_t cap : {0ull, 1ull, 17ull, 1ull << 20}) model_call(lens, slices, cap, density, seed++);
  // every pair fits; then a cap of exactly the total, and of one less (same seed: the same lists and hits)
  const uint64_t total = model_call(lens, 3, 1ull << 20, 100, seed);
  CHECK(total == 0 + 1 + 63 + 64 + 65 + 255 + 256 + 257 + 1000 + 5000);
  CHECK(model_call(lens, 3, total, 100, seed) == total && model_call(lens, 16, total - 1, 100, seed) == total);
  printf("ALL OK\n");
  return 0;
}
