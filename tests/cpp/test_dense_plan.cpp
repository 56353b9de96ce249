// The integer rules of the exact search for a shared allow-list (parallel_hnsw_amd/csrc/dense_plan.h) under the host
// sanitizers: the chunk plan at its edges against a 128-bit restatement, and host models of the list expansion and of
// the select's indexing over arrays of EXACTLY the sizes the launcher allocates, so that an index past any of them is
// an AddressSanitizer report.  No GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/dense_plan.h"

#define CHECK(x)                                                         \
  do {                                                                   \
    if (!(x)) {                                                          \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

typedef unsigned __int128 u128;

// the plan restated in 128 bits: nothing here can wrap
static void check_plan(uint64_t c, uint64_t nq, uint32_t nodes, uint64_t bytes) {
  const PhDensePlan p = ph_dense_plan(c, nq, nodes, bytes);
  CHECK(nodes % 64u == 0 && nodes >= 64u);
  CHECK(p.c == c && p.nq == nq && p.nodes == nodes);
  const u128 chunks = ((u128)c + nodes - 1) / nodes;
  CHECK((u128)p.node_chunks == chunks);
  const u128 widest = (((u128)(c < nodes ? c : nodes)) + 63) / 64 * 64;
  CHECK((u128)p.stride_max == widest && p.stride_max % 64u == 0);
  CHECK(p.positions >= 1u && p.positions <= PH_DENSE_POSITIONS_MAX);
  if (nq) CHECK(p.positions <= nq);
  // the table stays within the budget, unless the budget is below one row: then one position
  const u128 row = widest * 4;
  if (row && row <= (u128)bytes) CHECK((u128)p.positions * row <= (u128)bytes);
  if (row > (u128)bytes) CHECK(p.positions == 1u);
  // ... and is not needlessly small: one more position would break a limit
  if (row && (u128)p.positions < nq && p.positions < PH_DENSE_POSITIONS_MAX && p.positions > 1u)
    CHECK(((u128)p.positions + 1) * row > (u128)bytes);
  CHECK((u128)p.pos_chunks == ((u128)nq + p.positions - 1) / p.positions);
  CHECK((u128)p.table_floats == (u128)std::min<uint64_t>(nq, p.positions) * widest);
  CHECK((u128)ph_dense_post_bytes(p, 1024) == (u128)nq * 1024 * 8 + (u128)p.table_floats * 4);
  // node chunks tile [0, c) without gap or overlap; strides cover their chunk and never exceed the widest
  uint64_t at = 0;
  const uint32_t probe[] = {0u, 1u, p.node_chunks / 2u, p.node_chunks ? p.node_chunks - 2u : 0u, p.node_chunks ? p.node_chunks - 1u : 0u};
  for (uint32_t i : probe) {
    if (i >= p.node_chunks) continue;
    uint64_t first;
    uint32_t tn, stride;
    ph_dense_node_chunk(p, i, &first, &tn, &stride);
    CHECK((u128)first == (u128)i * nodes && tn >= 1u && tn <= nodes && first + tn <= c);
    CHECK(i + 1u == p.node_chunks ? first + tn == c : tn == nodes);
    CHECK(stride % 64u == 0 && stride >= tn && stride < tn + 64u && stride <= p.stride_max);
  }
  if (p.node_chunks <= 4096u)
    for (uint32_t i = 0; i < p.node_chunks; i++) {
      uint64_t first;
      uint32_t tn, stride;
      ph_dense_node_chunk(p, i, &first, &tn, &stride);
      CHECK(first == at);
      at += tn;
    }
  else
    at = c;
  CHECK(at == c);
  at = 0;
  if (p.pos_chunks <= 4096u) {
    for (uint64_t j = 0; j < p.pos_chunks; j++) {
      uint64_t first;
      uint32_t npos;
      ph_dense_pos_chunk(p, j, &first, &npos);
      CHECK(first == at && npos >= 1u && npos <= p.positions);
      CHECK((u128)npos * p.stride_max <= (u128)p.table_floats);
      at += npos;
    }
    CHECK(at == nq);
  } else {
    uint64_t first;
    uint32_t npos;
    ph_dense_pos_chunk(p, p.pos_chunks - 1u, &first, &npos);
    CHECK(first + npos == nq && npos >= 1u);
  }
}

static void test_knobs() {
  CHECK(ph_dense_nodes_knob(0) == PH_DENSE_NODES_DEFAULT && ph_dense_nodes_knob(-5) == PH_DENSE_NODES_DEFAULT);
  CHECK(ph_dense_nodes_knob(1) == 64u && ph_dense_nodes_knob(63) == 64u && ph_dense_nodes_knob(64) == 64u);
  CHECK(ph_dense_nodes_knob(65) == 128u && ph_dense_nodes_knob(100) == 128u && ph_dense_nodes_knob(192) == 192u);
  CHECK(ph_dense_nodes_knob(193) == 256u && ph_dense_nodes_knob(8191) == 8192u);
  CHECK(ph_dense_nodes_knob(1ll << 40) == PH_DENSE_NODES_MAX && ph_dense_nodes_knob(65537) == PH_DENSE_NODES_MAX);
  CHECK(PH_DENSE_NODES_DEFAULT % 64u == 0 && PH_DENSE_NODES_MAX % 64u == 0);
  CHECK(ph_dense_bytes_knob(0) == PH_DENSE_TABLE_BYTES_DEFAULT && ph_dense_bytes_knob(-1) == PH_DENSE_TABLE_BYTES_DEFAULT);
  CHECK(ph_dense_bytes_knob(1) == 1u && ph_dense_bytes_knob(1ll << 40) == PH_DENSE_TABLE_BYTES_MAX);
  CHECK(PH_DENSE_TABLE_BYTES_DEFAULT < (4ull << 30) && PH_DENSE_TABLE_BYTES_MAX < (4ull << 30));
  CHECK(ph_dense_round64(0) == 0 && ph_dense_round64(1) == 64 && ph_dense_round64(64) == 64 && ph_dense_round64(65) == 128);
}

static void test_plan_edges() {
  const uint64_t cs[] = {0, 1, 63, 64, 65, 191, 192, 193, 8191, 8192, 8193, 100000, (1ull << 31) - 1u};
  const uint64_t nqs[] = {1, 16, 40, 65, 10000, (1ull << 20) + 1u, 0xFFFFFFFFull};
  const long long node_knobs[] = {0, 1, 64, 100, 192, 8192, 10000, 1ll << 40};
  const long long byte_knobs[] = {0, 1, 255, 256, 257, 768, 49152, 1ll << 20, 1ll << 40};
  for (uint64_t c : cs)
    for (uint64_t nq : nqs)
      for (long long nk : node_knobs)
        for (long long bk : byte_knobs) check_plan(c, nq, ph_dense_nodes_knob(nk), ph_dense_bytes_knob(bk));
  // the cases the GPU test forces: 65 queries in three position chunks, one position per chunk
  PhDensePlan p = ph_dense_plan(1500, 65, 192, 192u * 4u * 22u);
  CHECK(p.positions == 22u && p.pos_chunks == 3u && p.node_chunks == 8u && p.stride_max == 192u);
  p = ph_dense_plan(193, 16, 192, 1);
  CHECK(p.positions == 1u && p.pos_chunks == 16u && p.node_chunks == 2u);
  p = ph_dense_plan(0, 16, 8192, PH_DENSE_TABLE_BYTES_DEFAULT);
  CHECK(p.node_chunks == 0u && p.stride_max == 0u && p.table_floats == 0u);
  p = ph_dense_plan((1ull << 31) - 1u, 0xFFFFFFFFull, PH_DENSE_NODES_DEFAULT, PH_DENSE_TABLE_BYTES_DEFAULT);
  CHECK(p.node_chunks == 262144u && p.positions == 32768u && p.table_floats == 32768ull * 8192ull);
  // the default budget holds a 10 000-query batch against a full node chunk in one table
  p = ph_dense_plan(100000, 10000, PH_DENSE_NODES_DEFAULT, PH_DENSE_TABLE_BYTES_DEFAULT);
  CHECK(p.pos_chunks == 1u && p.node_chunks == 13u);
}

// ---- host model of the list expansion: per-word popcount, exclusive prefix in place, every word writes at its offset
static std::vector<uint32_t> expand(const std::vector<uint32_t> &bitmap, uint64_t n, uint32_t cap, uint32_t *total) {
  const uint64_t nwords = (n + 31u) / 32u;
  std::vector<uint32_t> pre(ph_dense_pre_words(nwords, cap, 3));  // the launcher's block, nq = 3
  uint32_t *const head = pre.data(), *const off = head + PH_DENSE_HEAD_WORDS, *const list = off + ph_dense_off_words(nwords);
  uint32_t *const safe = list + cap, *const flags = safe + 3;
  auto word = [&](uint64_t w) {
    uint32_t v = bitmap[w];
    if (n - w * 32u < 32u) v &= (1u << (n - w * 32u)) - 1u;
    return v;
  };
  for (uint64_t w = 0; w < nwords; w++) off[w] = (uint32_t)__builtin_popcount(word(w));
  uint32_t base = 0;
  for (uint64_t w = 0; w < nwords; w++) {
    const uint32_t v = off[w];
    off[w] = base;
    base += v;
  }
  off[nwords] = base, head[1] = base;
  for (uint64_t w = 0; w < nwords; w++) {
    uint32_t o = off[w];
    for (uint32_t t = word(w); t; t &= t - 1u) {
      if (o < cap) list[o] = (uint32_t)w * 32u + (uint32_t)__builtin_ctz(t);
      o++;
    }
    CHECK(o == off[w + 1]);
  }
  for (int q = 0; q < 3; q++) safe[q] = 0u, flags[q] = 0u;  // the last words of the block
  *total = base;
  return std::vector<uint32_t>(list, list + std::min(base, cap));
}

static void test_list_model() {
  std::mt19937 rng(5);
  for (uint64_t n : {1ull, 31ull, 32ull, 33ull, 5000ull, 4096ull}) {
    const uint64_t nwords = (n + 31u) / 32u;
    for (double density : {0.0, 0.01, 0.5, 1.0}) {
      std::vector<uint32_t> bm(nwords);
      std::vector<uint32_t> want;
      for (uint64_t v = 0; v < nwords * 32u; v++)
        if ((double)(rng() % 10000u) < density * 10000.0) {
          bm[v >> 5] |= 1u << (v & 31u);  // bits at and past n are set too: they must not be listed
          if (v < n) want.push_back((uint32_t)v);
        }
      uint32_t total = 0;
      const std::vector<uint32_t> got = expand(bm, n, (uint32_t)n, &total);
      CHECK(total == want.size() && got == want);
      CHECK(std::is_sorted(got.begin(), got.end()));
    }
  }
}

// ---- host model of the select's indexing: every (node chunk, position chunk) reads its table rows and the list, and
// the key scratch / output rows by query index, over arrays of the launcher's sizes; the result is the plain top-k
static void test_select_model() {
  std::mt19937 rng(9);
  struct Case { uint64_t c, nq; long long nodes, bytes; uint32_t k; };
  const Case cases[] = {{1, 1, 0, 0, 1},      {63, 16, 64, 1, 10},      {64, 40, 64, 0, 10},   {65, 65, 64, 64 * 4 * 22, 100},
                        {193, 16, 192, 0, 10}, {1500, 65, 192, 192 * 4 * 22, 1024}, {700, 5, 100, 1000, 7}};
  for (const Case &cs : cases) {
    const PhDensePlan p = ph_dense_plan(cs.c, cs.nq, ph_dense_nodes_knob(cs.nodes), ph_dense_bytes_knob(cs.bytes));
    std::vector<uint32_t> list(cs.c);
    for (uint64_t i = 0; i < cs.c; i++) list[i] = (uint32_t)(3u * i + 1u);
    std::vector<float> dist(cs.nq * cs.c);
    for (float &d : dist) d = (float)(rng() % 97u);  // many ties
    std::vector<uint8_t> post(ph_dense_post_bytes(p, cs.k));
    uint64_t *const keys = (uint64_t *)post.data();
    float *const D = (float *)(post.data() + ph_dense_key_bytes(cs.nq, cs.k));
    std::vector<uint64_t> out(cs.nq * cs.k, ~0ull);
    for (uint32_t i = 0; i < p.node_chunks; i++) {
      uint64_t nfirst;
      uint32_t tn, stride;
      ph_dense_node_chunk(p, i, &nfirst, &tn, &stride);
      for (uint64_t j = 0; j < p.pos_chunks; j++) {
        uint64_t pfirst;
        uint32_t npos;
        ph_dense_pos_chunk(p, j, &pfirst, &npos);
        for (uint32_t pp = 0; pp < npos; pp++)  // the table kernels: entries [0, tn) of each row
          for (uint32_t t = 0; t < tn; t++) D[(uint64_t)pp * stride + t] = dist[(pfirst + pp) * cs.c + nfirst + t];
        for (uint32_t pp = 0; pp < npos; pp++) {
          const uint64_t q = pfirst + pp;
          std::vector<uint64_t> top;
          if (i)
            for (uint32_t e = 0; e < cs.k; e++)
              if (keys[q * cs.k + e] != ~0ull) top.push_back(keys[q * cs.k + e]);
          for (uint32_t b = 0; b < tn; b += 64u)
            for (uint32_t lane = 0; lane < 64u; lane++) {
              const uint32_t t = b + lane;
              if (t < tn) top.push_back(((uint64_t)(uint32_t)D[(uint64_t)pp * stride + t] << 32) | list[nfirst + t]);
            }
          std::sort(top.begin(), top.end());
          if (top.size() > cs.k) top.resize(cs.k);
          uint64_t *const to = i + 1u == p.node_chunks ? &out[q * cs.k] : &keys[q * cs.k];
          for (uint32_t e = 0; e < cs.k; e++) to[e] = e < top.size() ? top[e] : ~0ull;
        }
      }
    }
    for (uint64_t q = 0; q < cs.nq; q++) {
      std::vector<uint64_t> want;
      for (uint64_t t = 0; t < cs.c; t++) want.push_back(((uint64_t)(uint32_t)dist[q * cs.c + t] << 32) | list[t]);
      std::sort(want.begin(), want.end());
      for (uint32_t e = 0; e < cs.k; e++) CHECK(out[q * cs.k + e] == (e < want.size() ? want[e] : ~0ull));
    }
  }
  CHECK(ph_dense_select_lds(1024) == (2u * 1024u + 64u) * 8u && ph_dense_select_lds(1024) <= 48u * 1024u);
}

int main() {
  test_knobs();
  test_plan_edges();
  test_list_model();
  test_select_model();
  printf("ALL OK\n");
  return 0;
}
