// How the exact top-k for a SHARED allow-list (filter_dense.hip) is cut into distance tables: pure integer rules,
// shared by the launcher and tests/cpp/test_dense_plan.cpp (which runs them under the host sanitizers, no GPU).
//
// The c candidates of the one bitmap, as an ascending id list, are cut into NODE CHUNKS of `nodes` ids (a multiple of
// 64; the last one shorter), the nq queries into POSITION CHUNKS of `positions` queries.  One table holds
// positions x stride floats, stride = the chunk's ids rounded up to 64, and stays within the byte budget unless that
// is smaller than one row (then one position per chunk).  Node chunks are the outer loop: the packed node operand of
// a chunk serves every position chunk.  All products in 64 bits.
#pragma once
#include <stdint.h>

#define PH_DENSE_NODES_DEFAULT 8192u            // PHNSW_DENSE_NODES
#define PH_DENSE_NODES_MAX 65536u               // ... clamped to this: 1024 node tiles, far inside every grid limit
#define PH_DENSE_TABLE_BYTES_DEFAULT (1ull << 30)  // PHNSW_DENSE_TABLE_BYTES: 32 768 positions x 8192 nodes
#define PH_DENSE_TABLE_BYTES_MAX ((4ull << 30) - 1u)  // below the 4 GiB cap of the search tables (tiny.hip)
#define PH_DENSE_POSITIONS_MAX (1u << 20)       // positions of one table call, whatever the budget: 16 384 position tiles
#define PH_DENSE_HEAD_WORDS 4u                  // [0] ph_filter_count's count, [1] the list's length

static inline uint64_t ph_dense_round64(uint64_t v) { return (v + 63u) / 64u * 64u; }

// the knobs as the launcher takes them: 0 or negative = the default, anything else clamped and (nodes) rounded up to 64
static inline uint32_t ph_dense_nodes_knob(long long v) {
  if (v <= 0) return PH_DENSE_NODES_DEFAULT;
  if (v > (long long)PH_DENSE_NODES_MAX) return PH_DENSE_NODES_MAX;
  return (uint32_t)ph_dense_round64((uint64_t)v);
}
static inline uint64_t ph_dense_bytes_knob(long long v) {
  if (v <= 0) return PH_DENSE_TABLE_BYTES_DEFAULT;
  return (uint64_t)v > PH_DENSE_TABLE_BYTES_MAX ? PH_DENSE_TABLE_BYTES_MAX : (uint64_t)v;
}

struct PhDensePlan {
  uint64_t c, nq;          // candidates (c <= 2^31 - 1), queries (nq <= 2^32 - 1)
  uint32_t nodes;          // ids per node chunk, a multiple of 64
  uint32_t node_chunks;    // ceil(c / nodes); 0 when c == 0
  uint32_t stride_max;     // the widest table row: min(c, nodes) rounded up to 64
  uint32_t positions;      // queries per position chunk, >= 1
  uint64_t pos_chunks;     // ceil(nq / positions)
  uint64_t table_floats;   // the table buffer: min(nq, positions) * stride_max
};

static inline PhDensePlan ph_dense_plan(uint64_t c, uint64_t nq, uint32_t nodes, uint64_t table_bytes) {
  PhDensePlan p;
  p.c = c, p.nq = nq, p.nodes = nodes;
  p.node_chunks = (uint32_t)((c + nodes - 1u) / nodes);
  p.stride_max = (uint32_t)ph_dense_round64(c < nodes ? c : nodes);
  uint64_t pos = p.stride_max ? table_bytes / ((uint64_t)p.stride_max * 4u) : PH_DENSE_POSITIONS_MAX;
  if (pos > PH_DENSE_POSITIONS_MAX) pos = PH_DENSE_POSITIONS_MAX;
  if (pos > nq) pos = nq;
  if (pos < 1u) pos = 1u;
  p.positions = (uint32_t)pos;
  p.pos_chunks = (nq + pos - 1u) / pos;
  p.table_floats = (nq < pos ? nq : pos) * (uint64_t)p.stride_max;
  return p;
}

// ids [*first, *first + *tn) of the list are node chunk i (i < node_chunks); its table rows are *stride floats apart
static inline void ph_dense_node_chunk(const PhDensePlan &p, uint32_t i, uint64_t *first, uint32_t *tn, uint32_t *stride) {
  *first = (uint64_t)i * p.nodes;
  const uint64_t left = p.c - *first;
  *tn = (uint32_t)(left < p.nodes ? left : p.nodes);
  *stride = (uint32_t)ph_dense_round64(*tn);
}

// queries [*first, *first + *npos) are position chunk j (j < pos_chunks)
static inline void ph_dense_pos_chunk(const PhDensePlan &p, uint64_t j, uint64_t *first, uint32_t *npos) {
  *first = j * p.positions;
  const uint64_t left = p.nq - *first;
  *npos = (uint32_t)(left < p.positions ? left : p.positions);
}

// The scratch sized BEFORE the candidate count is known, in 4-byte words: head | off [nwords + 1] (per-word counts,
// then their exclusive prefix; the last entry the total) | list [cap] (cap = the ids the bottom layer can hold at
// most) | sanitised qids [nq] | flags [nq]
static inline uint64_t ph_dense_off_words(uint64_t nwords) { return nwords + 1u; }
static inline uint64_t ph_dense_pre_words(uint64_t nwords, uint64_t cap, uint64_t nq) {
  return PH_DENSE_HEAD_WORDS + ph_dense_off_words(nwords) + cap + 2u * nq;
}
// ... and AFTER, in bytes: the [nq][k] key scratch (8-byte keys, first), then the table
static inline uint64_t ph_dense_key_bytes(uint64_t nq, uint64_t k) { return nq * k * 8u; }
static inline uint64_t ph_dense_post_bytes(const PhDensePlan &p, uint64_t k) {
  return ph_dense_key_bytes(p.nq, k) + p.table_floats * 4u;
}
// dynamic LDS of the select: two key lists of k entries and 64 sorted survivor keys
static inline uint64_t ph_dense_select_lds(uint64_t k) { return (2u * k + 64u) * 8u; }
