// How the exact radius search (filter_radius.hip) sizes its record pool and its sort: pure integer rules, shared by the
// launcher and tests/cpp/test_radius_plan.cpp (which runs them under the host sanitizers, no GPU).
//
// A RECORD is one (query, candidate) pair inside the query's radius: the 8-byte key mkkey(distance, id) and the 4-byte
// query index, kept in two parallel arrays.  The compaction kernel reserves a row's records with one atomic add on a
// 64-bit cursor and drops -- but still counts -- what lands at or past the pool's capacity, so the cursor ends as the
// exact total whatever the capacity.  The pool is sorted by (query, key) with two stable radix passes, key first, so
// every array exists twice (a pass reads one and writes the other).  All products in 64 bits.
#pragma once
#include <stdint.h>

#define PH_RADIUS_CAP_MAX 0x7FFFFFFFull  // cap of a call, and so the records of a sort: the sort counts in int
#define PH_RADIUS_HEAD_WORDS 2u          // 8-byte words in front of the pool: [0] the cursor, [1] spare

// the caller's cap is acceptable
static inline bool ph_radius_cap_valid(uint64_t cap) { return cap <= PH_RADIUS_CAP_MAX; }

// Records the pool holds: no call needs more than its cap (a larger total is reported, not emitted) nor more than every
// (query, candidate) pair; cap == 0 is the count-only form, without a pool.  nq * c < 2^64: nq < 2^32, c < 2^31.
static inline uint64_t ph_radius_pool_records(uint64_t cap, uint64_t nq, uint64_t c) {
  const uint64_t pairs = nq * c;
  return cap < pairs ? cap : pairs;
}

// whether the records are emitted at all: a pool, and a total that fits it (then nothing was dropped)
static inline bool ph_radius_emits(uint64_t total, uint64_t cap) { return total != 0 && total <= cap; }

// the bits of the query index the second pass sorts by: enough for nq - 1, at least 1
static inline int ph_radius_query_bits(uint64_t nq) {
  int b = 1;
  while (b < 32 && (nq - 1u) >> b) b++;
  return b;
}

// The scratch of one call, in bytes, every block on a 16-byte boundary:
//   head [PH_RADIUS_HEAD_WORDS] u64 | count [nq + 1] u32 (count[nq] stays 0: the exclusive sum runs over nq + 1)
//   | keys A, keys B [records] u64 | query A, query B [records] u32 | the table
static inline uint64_t ph_radius_round16(uint64_t v) { return (v + 15u) / 16u * 16u; }
struct PhRadiusLayout {
  uint64_t head, count, keys_a, keys_b, q_a, q_b, table, bytes;  // offsets, then the size
};
static inline PhRadiusLayout ph_radius_layout(uint64_t nq, uint64_t records, uint64_t table_floats) {
  PhRadiusLayout l;
  l.head = 0;
  l.count = ph_radius_round16(PH_RADIUS_HEAD_WORDS * 8u);
  l.keys_a = l.count + ph_radius_round16((nq + 1u) * 4u);
  l.keys_b = l.keys_a + ph_radius_round16(records * 8u);
  l.q_a = l.keys_b + ph_radius_round16(records * 8u);
  l.q_b = l.q_a + ph_radius_round16(records * 4u);
  l.table = l.q_b + ph_radius_round16(records * 4u);
  l.bytes = l.table + ph_radius_round16(table_floats * 4u);
  return l;
}

// the grid of the compaction kernel: one wave64 per position, striding when a chunk has more positions than this
static inline uint32_t ph_radius_grid(uint64_t npos) { return (uint32_t)(npos < (1u << 20) ? npos : (1u << 20)); }
