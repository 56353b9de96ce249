// The integer rules of the exact radius search (parallel_hnsw_amd/csrc/radius_plan.h) under the host sanitizers: the
// pool's capacity and the scratch layout at their edges against a 128-bit restatement, and a host model of the
// compaction (reserve with one add on the cursor, write below the capacity, drop but count the rest) and of the sort
// and unpack over arrays of EXACTLY the sizes the launcher allocates, so that an index past any of them is an
// AddressSanitizer report.  No GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/dense_plan.h"
#include "../../parallel_hnsw_amd/csrc/radius_plan.h"

#define CHECK(x)                                                         \
  do {                                                                   \
    if (!(x)) {                                                          \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

typedef unsigned __int128 u128;

static void check_rules(uint64_t cap, uint64_t nq, uint64_t c, uint64_t table_floats) {
  const uint64_t rec = ph_radius_pool_records(cap, nq, c);
  const u128 pairs = (u128)nq * c;
  CHECK((u128)rec == ((u128)cap < pairs ? (u128)cap : pairs));
  CHECK(rec <= cap && (cap != 0 || rec == 0));
  if (ph_radius_cap_valid(cap)) CHECK(rec <= 0x7FFFFFFFull);  // the sort counts in int
  const PhRadiusLayout l = ph_radius_layout(nq, rec, table_floats);
  const uint64_t off[] = {l.head, l.count, l.keys_a, l.keys_b, l.q_a, l.q_b, l.table, l.bytes};
  const u128 size[] = {(u128)PH_RADIUS_HEAD_WORDS * 8, ((u128)nq + 1) * 4, (u128)rec * 8, (u128)rec * 8, (u128)rec * 4,
                       (u128)rec * 4, (u128)table_floats * 4};
  CHECK(l.head == 0);
  for (int i = 0; i < 7; i++) {  // in order, 16-byte aligned, each block at least its size, no overlap
    CHECK(off[i] % 16u == 0);
    CHECK((u128)off[i] + size[i] <= (u128)off[i + 1]);
    CHECK((u128)off[i + 1] < (u128)off[i] + size[i] + 16);
  }
}

static void check_bits() {
  CHECK(ph_radius_query_bits(1) == 1 && ph_radius_query_bits(2) == 1 && ph_radius_query_bits(3) == 2);
  CHECK(ph_radius_query_bits(4) == 2 && ph_radius_query_bits(5) == 3 && ph_radius_query_bits(65) == 7);
  CHECK(ph_radius_query_bits(0x7FFFFFFEull) == 31 && ph_radius_query_bits(0xFFFFFFFFull) == 32);
  for (uint64_t nq = 1; nq < 5000; nq++) {
    const int b = ph_radius_query_bits(nq);
    CHECK(b >= 1 && b <= 32 && ((nq - 1) >> b) == 0 && (b == 1 || ((nq - 1) >> (b - 1)) != 0));
  }
}

// A call on the host: tables of the chunk plan, rows compacted position by position in an order a seed decides (the
// waves' order is not fixed), into a pool of exactly the layout's size; then the two stable sorts and the unpack.
static uint64_t model_call(uint64_t nq, uint64_t c, uint32_t nodes, uint64_t table_bytes, uint64_t cap, uint32_t seed) {
  std::mt19937 rng(seed);
  std::vector<uint32_t> list(c);
  for (uint64_t i = 0; i < c; i++) list[i] = (uint32_t)(3u * i + 1u);  // ascending ids
  std::vector<uint32_t> dist(nq * c);                                  // a distance as its ordered 32-bit key
  for (auto &v : dist) v = rng() % 7u;                                 // many ties
  std::vector<uint32_t> radius(nq);
  for (auto &v : radius) v = rng() % 8u;

  const PhDensePlan plan = ph_dense_plan(c, nq, nodes, table_bytes);
  const uint64_t rec = ph_radius_pool_records(cap, nq, c);
  const PhRadiusLayout l = ph_radius_layout(nq, rec, plan.table_floats);
  std::vector<unsigned char> post(l.bytes);
  uint64_t *const cursor = (uint64_t *)(post.data() + l.head);
  uint32_t *const count = (uint32_t *)(post.data() + l.count);
  uint64_t *const keys = (uint64_t *)(post.data() + l.keys_a);
  uint32_t *const qs = (uint32_t *)(post.data() + l.q_a);
  uint32_t *const D = (uint32_t *)(post.data() + l.table);
  *cursor = 0;
  for (uint64_t q = 0; q <= nq; q++) count[q] = 0;

  for (uint32_t i = 0; i < plan.node_chunks; i++) {
    uint64_t nfirst;
    uint32_t tn, stride;
    ph_dense_node_chunk(plan, i, &nfirst, &tn, &stride);
    for (uint64_t j = 0; j < plan.pos_chunks; j++) {
      uint64_t pfirst;
      uint32_t npos;
      ph_dense_pos_chunk(plan, j, &pfirst, &npos);
      for (uint32_t p = 0; p < npos; p++)
        for (uint32_t t = 0; t < tn; t++) D[(uint64_t)p * stride + t] = dist[(pfirst + p) * c + nfirst + t];
      std::vector<uint32_t> order(npos);
      for (uint32_t p = 0; p < npos; p++) order[p] = p;
      std::shuffle(order.begin(), order.end(), rng);
      CHECK(ph_radius_grid(npos) >= 1u && ph_radius_grid(npos) <= npos);
      for (uint32_t p : order) {
        const uint64_t q = pfirst + p;
        uint32_t cnt = 0;
        for (uint32_t t = 0; t < tn; t++) cnt += D[(uint64_t)p * stride + t] < radius[q];
        if (!cnt) continue;
        uint64_t slot = *cursor;
        *cursor += cnt, count[q] += cnt;
        if (!rec) continue;
        for (uint32_t t = 0; t < tn; t++)
          if (D[(uint64_t)p * stride + t] < radius[q]) {
            if (slot < rec) keys[slot] = ((uint64_t)D[(uint64_t)p * stride + t] << 32) | list[nfirst + t], qs[slot] = (uint32_t)q;
            slot++;
          }
      }
    }
  }

  // the truth, straight from the matrix
  std::vector<std::vector<uint64_t>> want(nq);
  uint64_t total = 0;
  for (uint64_t q = 0; q < nq; q++) {
    for (uint64_t t = 0; t < c; t++)
      if (dist[q * c + t] < radius[q]) want[q].push_back(((uint64_t)dist[q * c + t] << 32) | list[t]);
    std::sort(want[q].begin(), want[q].end());
    CHECK(count[q] == want[q].size());
    total += want[q].size();
  }
  CHECK(*cursor == total && count[nq] == 0);  // exact whatever the capacity
  if (!ph_radius_emits(total, cap)) return total;
  CHECK(total <= rec);  // nothing was dropped
  std::vector<uint64_t> perm(total);
  for (uint64_t i = 0; i < total; i++) perm[i] = i;
  std::stable_sort(perm.begin(), perm.end(), [&](uint64_t a, uint64_t b) { return keys[a] < keys[b]; });
  std::stable_sort(perm.begin(), perm.end(), [&](uint64_t a, uint64_t b) { return qs[a] < qs[b]; });
  uint64_t at = 0;
  for (uint64_t q = 0; q < nq; q++)
    for (uint64_t key : want[q]) {
      CHECK(qs[perm[at]] == q && keys[perm[at]] == key);
      at++;
    }
  CHECK(at == total);
  return total;
}

int main() {
  const uint64_t caps[] = {0, 1, 63, 64, 65, 1000, 0x7FFFFFFFull};
  const uint64_t nqs[] = {1, 2, 65, 10000, 0x7FFFFFFEull};
  const uint64_t cs[] = {0, 1, 64, 5000, 0x7FFFFFFFull};
  for (uint64_t cap : caps)
    for (uint64_t nq : nqs)
      for (uint64_t c : cs) check_rules(cap, nq, c, (c % 4096u) * 3u);
  CHECK(ph_radius_cap_valid(0) && ph_radius_cap_valid(0x7FFFFFFFull) && !ph_radius_cap_valid(0x80000000ull));
  CHECK(!ph_radius_cap_valid(~0ull));
  CHECK(!ph_radius_emits(0, 0) && !ph_radius_emits(0, 5) && ph_radius_emits(5, 5) && !ph_radius_emits(6, 5) && !ph_radius_emits(1, 0));
  check_bits();
  uint32_t seed = 1;
  for (uint64_t nq : {1ull, 5ull, 65ull})
    for (uint64_t c : {0ull, 1ull, 63ull, 64ull, 65ull, 200ull})
      for (uint32_t nodes : {64u, 128u})
        for (uint64_t bytes : {1ull, 64ull * 4 * 2, 1ull << 20})
          for (uint64_t cap : {0ull, 1ull, 17ull, 1ull << 20}) model_call(nq, c, nodes, bytes, cap, seed++);
  // every pair fits; then a cap of exactly the total, and of one less (same seed: the same distances and radii)
  const uint64_t total = model_call(65, 200, 64, 64ull * 4 * 22, 65ull * 200, seed);
  CHECK(total > 1 && model_call(65, 200, 64, 64ull * 4 * 22, total, seed) == total);
  CHECK(model_call(65, 200, 64, 64ull * 4 * 22, total - 1, seed) == total);
  printf("ALL OK\n");
  return 0;
}
