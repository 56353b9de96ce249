// Stand-alone host check of the rules behind the routed filtered search (parallel_hnsw_amd/csrc/filter_route.h, the
// header the entry points and the kernels include): compiled with -fsanitize=address,undefined and run without a GPU
// (tests/test_filter_route_cpp.py).  The route at its edges -- c * ef against k * N around 2^32, scan_below 0 and
// UINT64_MAX, c = 0 -- against a 128-bit restatement, the default thresholds, the length of a complete row, the
// argument checks, and a host model of the routing kernel's compaction over arrays of exactly the sizes the call
// allocates, so that an index out of bounds is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/filter_route.h"

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

// the rule of phnsw.h in arithmetic that cannot wrap for any argument
static uint32_t wide_route(uint64_t c, uint64_t scan_below, uint64_t ef, uint64_t k, uint64_t n_nodes) {
  if (c <= scan_below) return PH_ROUTE_SCAN;
  return (unsigned __int128)c * ef < (unsigned __int128)k * n_nodes ? PH_ROUTE_SCAN : PH_ROUTE_GRAPH;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// the routing kernel's walk over a batch: 256 queries at a time, four waves of 64, a ballot per wave and a scan over
// the waves' counts; returns through the two lists, which have ph_auto_list_words(nq) entries each
static void model_route(const std::vector<uint32_t> &counts, bool per_query, uint64_t nq, uint64_t scan_below, uint32_t ef,
                        uint32_t k, uint32_t n_nodes, std::vector<uint32_t> &glist, std::vector<uint32_t> &slist,
                        std::vector<uint32_t> &route, uint32_t head[PH_AUTO_HEAD_WORDS]) {
  CHECK(counts.size() == ph_auto_bitmaps(nq, per_query));
  glist.assign(ph_auto_list_words(nq), 0xFFFFFFFFu);
  slist.assign(ph_auto_list_words(nq), 0xFFFFFFFFu);
  route.assign(nq, 7u);
  uint32_t gbase = 0, sbase = 0;
  for (uint64_t base = 0; base < nq; base += 256u) {
    uint32_t wave_g[4] = {0, 0, 0, 0}, wave_s[4] = {0, 0, 0, 0}, r[256] = {};
    for (uint32_t t = 0; t < 256u; t++) {
      if (base + t >= nq) continue;
      r[t] = ph_auto_route(counts.at(per_query ? base + t : 0u), scan_below, ef, k, n_nodes);
      route.at(base + t) = r[t];
      if (r[t] == PH_ROUTE_GRAPH)
        wave_g[t >> 6]++;
      else
        wave_s[t >> 6]++;
    }
    uint32_t goff[4], soff[4], gtot = 0, stot = 0;
    for (uint32_t w = 0; w < 4u; w++) goff[w] = gbase + gtot, soff[w] = sbase + stot, gtot += wave_g[w], stot += wave_s[w];
    for (uint32_t t = 0; t < 256u; t++) {
      if (base + t >= nq) continue;
      if (r[t] == PH_ROUTE_GRAPH)
        glist.at(goff[t >> 6]++) = (uint32_t)(base + t);
      else
        slist.at(soff[t >> 6]++) = (uint32_t)(base + t);
    }
    gbase += gtot, sbase += stot;
  }
  head[0] = gbase, head[1] = sbase;
}

int main() {
  // ---- the route at its edges
  CHECK(ph_auto_route(0, 0, 1024, 1, 1) == PH_ROUTE_SCAN);   // c = 0: 0 <= scan_below whatever it is
  CHECK(ph_auto_route(0, 1, 1, 1, 0) == PH_ROUTE_SCAN);
  CHECK(ph_auto_route(1, 0, 1024, 1, 0) == PH_ROUTE_GRAPH);  // an empty bottom layer: k * N = 0, nothing is below it
  CHECK(ph_auto_route(100, 100, 1024, 1, 5000) == PH_ROUTE_SCAN);
  CHECK(ph_auto_route(101, 100, 1024, 1, 5000) == PH_ROUTE_GRAPH);
  CHECK(ph_auto_route(3124, 100, 16, 10, 5000) == PH_ROUTE_SCAN);   // 3124 * 16 = 49 984 < 50 000
  CHECK(ph_auto_route(3125, 100, 16, 10, 5000) == PH_ROUTE_GRAPH);  // 3125 * 16 = 50 000
  CHECK(ph_auto_route(0xFFFFFFFFu, UINT64_MAX, 1024, 1, 1) == PH_ROUTE_SCAN);  // UINT64_MAX: always scan
  // c * ef and k * N on either side of 2^32 and of each other
  const uint32_t two22 = 1u << 22;
  CHECK((uint64_t)two22 * 1024u == 1ull << 32);
  CHECK(ph_auto_route(two22, 1, 1024, 1024, two22) == PH_ROUTE_GRAPH);      // 2^32 against 2^32
  CHECK(ph_auto_route(two22, 1, 1024, 1024, two22 + 1u) == PH_ROUTE_SCAN);  // 2^32 against 2^32 + 1024
  CHECK(ph_auto_route(two22 - 1u, 1, 1024, 1024, two22) == PH_ROUTE_SCAN);  // 2^32 - 1024 against 2^32
  CHECK(ph_auto_route(two22 + 1u, 1, 1024, 1, 0xFFFFFFFFu) == PH_ROUTE_GRAPH);  // 2^32 + 1024 against 2^32 - 1: a 32-bit
                                                                                // product would read 1024
  CHECK(ph_auto_route(0xFFFFFFFFu, 1, 1024, 1024, 0xFFFFFFFFu) == PH_ROUTE_GRAPH);
  CHECK(ph_auto_route(0xFFFFFFFEu, 1, 1024, 1024, 0xFFFFFFFFu) == PH_ROUTE_SCAN);
  CHECK(ph_auto_route(0xFFFFFFFFu, 1, 1, 1024, 0xFFFFFFFFu) == PH_ROUTE_SCAN);
  for (int i = 0; i < 200000; i++) {
    const uint32_t ef = 1u + (uint32_t)(rnd() % 1024u), k = 1u + (uint32_t)(rnd() % ef);
    const uint32_t n_nodes = (uint32_t)(rnd() >> (32 + rnd() % 32)), span = (uint32_t)(rnd() % 5u);
    // counts near the crossover of the second rule, and anywhere
    const uint64_t edge = ((uint64_t)k * n_nodes + ef - 1u) / ef;
    uint64_t c64 = (i & 1) ? edge + span - 2u : rnd() >> 32;
    if (c64 > 0xFFFFFFFFull) c64 = 0xFFFFFFFFull;
    const uint64_t below = (i & 2) ? rnd() % 1000u : 0u;
    CHECK(ph_auto_route((uint32_t)c64, ph_auto_scan_below(below, i & 4), ef, k, n_nodes) ==
          wide_route(c64, below ? below : ((i & 4) ? 10000u : 13000u), ef, k, n_nodes));
  }

  // ---- the default thresholds
  CHECK(ph_auto_scan_below(0, false) == 13000u && ph_auto_scan_below(0, true) == 10000u);
  CHECK(ph_auto_scan_below(1, false) == 1u && ph_auto_scan_below(1, true) == 1u);
  CHECK(ph_auto_scan_below(UINT64_MAX, true) == UINT64_MAX);
  CHECK(ph_auto_route(13000, ph_auto_scan_below(0, false), 1024, 1, 1000000) == PH_ROUTE_SCAN);
  CHECK(ph_auto_route(13001, ph_auto_scan_below(0, false), 1024, 1, 1000000) == PH_ROUTE_GRAPH);
  CHECK(ph_auto_route(10000, ph_auto_scan_below(0, true), 1024, 1, 1000000) == PH_ROUTE_SCAN);
  CHECK(ph_auto_route(10001, ph_auto_scan_below(0, true), 1024, 1, 1000000) == PH_ROUTE_GRAPH);

  // ---- the length of a complete row
  CHECK(ph_auto_full_len(0, 0, 10) == 0 && ph_auto_full_len(0, 1, 10) == 0);
  CHECK(ph_auto_full_len(1, 1, 10) == 0 && ph_auto_full_len(1, 0, 10) == 1);
  CHECK(ph_auto_full_len(10, 0, 10) == 10 && ph_auto_full_len(10, 1, 10) == 9 && ph_auto_full_len(11, 1, 10) == 10);
  CHECK(ph_auto_full_len(0xFFFFFFFFu, 1, 1024) == 1024);

  // ---- the argument checks
  CHECK(!ph_auto_k_valid(0, 16) && ph_auto_k_valid(1, 16) && ph_auto_k_valid(16, 16) && !ph_auto_k_valid(17, 16));
  CHECK(ph_auto_k_valid(1024, 1024) && !ph_auto_k_valid(1025, 1025) && !ph_auto_k_valid(1, 0) && !ph_auto_k_valid(1, 1025));
  CHECK(!ph_auto_k_valid(UINT64_MAX, 1024) && !ph_auto_k_valid(1, UINT64_MAX));
  CHECK(ph_auto_queries_valid(true, false) && ph_auto_queries_valid(false, true));
  CHECK(!ph_auto_queries_valid(true, true) && !ph_auto_queries_valid(false, false));
  CHECK(ph_auto_stride_valid(0, 5000) && ph_auto_stride_valid(157, 5000) && ph_auto_stride_valid(160, 5000));
  CHECK(!ph_auto_stride_valid(156, 5000) && !ph_auto_stride_valid(1, 33) && ph_auto_stride_valid(1, 32));
  CHECK(ph_auto_nq_valid(0) && ph_auto_nq_valid(0xFFFFFFFFull) && !ph_auto_nq_valid(0x100000000ull));

  // ---- the scratch block holds what the call carves out of it
  for (uint64_t nq : {1ull, 70ull, 256ull, 257ull, 100000ull})
    for (int per_query = 0; per_query < 2; per_query++)
      for (uint64_t ef : {1ull, 16ull, 1024ull}) {
        const uint64_t nb = ph_auto_bitmaps(nq, per_query);
        CHECK(nb == (per_query ? nq : 1u));
        const uint64_t end = PH_AUTO_HEAD_WORDS + nb + 2u * ph_auto_list_words(nq) + nq + nq + nq * ef + nq * ef;
        CHECK(ph_auto_scratch_words(nq, per_query, ef) == end);
      }

  // ---- the compaction: both lists ascending, together every query once, nothing written past a list
  for (uint64_t nq : {1ull, 63ull, 64ull, 65ull, 70ull, 255ull, 256ull, 257ull, 1000ull}) {
    for (int per_query = 0; per_query < 2; per_query++) {
      for (int shape = 0; shape < 4; shape++) {  // all graph, all scan, mixed, mixed
        std::vector<uint32_t> counts(ph_auto_bitmaps(nq, per_query));
        for (uint32_t &c : counts) c = shape == 0 ? 5000u : (shape == 1 ? 0u : (uint32_t)(rnd() % 5001u));
        std::vector<uint32_t> glist, slist, route;
        uint32_t head[PH_AUTO_HEAD_WORDS] = {};
        model_route(counts, per_query, nq, 100, 16, 10, 5000, glist, slist, route, head);
        CHECK((uint64_t)head[0] + head[1] == nq);
        std::vector<int> seen(nq, 0);
        for (uint32_t i = 0; i < head[0]; i++) {
          CHECK(glist[i] < nq && route[glist[i]] == PH_ROUTE_GRAPH && (i == 0 || glist[i - 1] < glist[i]));
          seen[glist[i]]++;
        }
        for (uint32_t i = 0; i < head[1]; i++) {
          CHECK(slist[i] < nq && route[slist[i]] == PH_ROUTE_SCAN && (i == 0 || slist[i - 1] < slist[i]));
          seen[slist[i]]++;
        }
        for (uint64_t q = 0; q < nq; q++) CHECK(seen[q] == 1);
        if (!per_query) CHECK(head[0] == 0 || head[1] == 0);  // one bitmap: the whole batch goes one way
        // every short graph row moves over: the scan list never outgrows its nq entries
        CHECK((uint64_t)head[1] + head[0] <= ph_auto_list_words(nq));
      }
    }
  }
  std::printf("ALL OK\n");
  return 0;
}
