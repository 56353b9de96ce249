// The integer rules of the exact search over a table of allow-lists (parallel_hnsw_amd/csrc/group_plan.h) under the
// host sanitizers: keys, rounds under the byte budget and scratch sizes at their edges against a 128-bit restatement, and
// host models of the grouping pass, of the CSR list expansion and of the select's `order` indexing over arrays of EXACTLY
// the sizes the launcher allocates, so that an index past any of them is an AddressSanitizer report.  No GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/dense_plan.h"
#include "../../parallel_hnsw_amd/csrc/group_plan.h"

#define CHECK(x)                                                         \
  do {                                                                   \
    if (!(x)) {                                                          \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

typedef unsigned __int128 u128;

static void check_keys() {
  const uint64_t tables[] = {1, 2, 5, 257, 0xFFFFFFFEull};
  for (uint64_t nf : tables) {
    CHECK(ph_group_key(0, nf) == 0u);
    CHECK(ph_group_key((uint32_t)(nf - 1u), nf) == (uint32_t)(nf - 1u));
    CHECK(ph_group_key(PH_GROUP_SELECT_ALL, nf) == (uint32_t)nf);  // a key no bitmap has ...
    CHECK(!ph_group_key_has_bitmap((uint32_t)nf, nf) && (uint32_t)nf != PH_GROUP_KEY_REJECT);  // ... and not the reject key
    if (nf < 0xFFFFFFFEull) {
      CHECK(ph_group_key((uint32_t)nf, nf) == PH_GROUP_KEY_REJECT);  // selector == nfilters
      CHECK(ph_group_key(0xFFFFFFFEu, nf) == PH_GROUP_KEY_REJECT);
    }
    CHECK(!ph_group_key_has_bitmap(PH_GROUP_KEY_REJECT, nf));
    CHECK(ph_group_key_has_bitmap((uint32_t)(nf - 1u), nf));
    // the last word of the last bitmap, in 64 bits
    const uint32_t stride = 0xFFFFFFFFu;
    CHECK((u128)ph_group_bitmap_at((uint32_t)(nf - 1u), stride) == (u128)(nf - 1u) * stride);
  }
  CHECK(ph_group_max(10, 3) == 5u && ph_group_max(4, 3) == 4u && ph_group_max(1, 0xFFFFFFFEull) == 1u);
  CHECK(ph_group_max(0xFFFFFFFFull, 0xFFFFFFFEull) == 0xFFFFFFFFull);
  CHECK(ph_group_bytes_knob(0) == PH_GROUP_LIST_BYTES_DEFAULT && ph_group_bytes_knob(-5) == PH_GROUP_LIST_BYTES_DEFAULT);
  CHECK(ph_group_bytes_knob(1) == 1u && ph_group_bytes_knob(1ll << 60) == PH_GROUP_LIST_BYTES_MAX);
}

// rounds restated in 128 bits: they tile [0, ngroups), each fits the budget or is one group, none is needlessly short
static uint64_t check_rounds(const std::vector<uint32_t> &counts, uint64_t nwords, uint64_t budget) {
  const uint64_t ng = counts.size();
  uint64_t rounds = 0, g0 = 0;
  u128 most = 0;
  while (g0 < ng) {
    const uint64_t g1 = ph_group_round_end(counts.data(), ng, g0, nwords, budget);
    CHECK(g1 > g0 && g1 <= ng && g1 - g0 <= PH_GROUP_ROUND_GROUPS_MAX);
    u128 words = 0, lists = 0;
    for (uint64_t g = g0; g < g1; g++) words += (u128)counts[g] + nwords + 1, lists += counts[g];
    if (g1 - g0 > 1u) CHECK(words * 4 <= (u128)budget);
    if (g1 < ng && g1 - g0 < PH_GROUP_ROUND_GROUPS_MAX) CHECK((words + counts[g1] + nwords + 1) * 4 > (u128)budget);
    CHECK((u128)ph_group_round_off_words(g0, g1, nwords) == (u128)(g1 - g0) * (nwords + 1));
    CHECK((u128)ph_group_round_list_words(counts.data(), g0, g1) == lists);
    most = std::max(most, words);
    g0 = g1, rounds++;
  }
  uint64_t r = ~0ull;
  CHECK((u128)ph_group_list_bytes(counts.data(), ng, nwords, budget, &r) == most * 4);
  CHECK(r == rounds);
  return rounds;
}

static void check_pre(uint64_t nq, uint64_t nf) {
  const uint64_t G = ph_group_max(nq, nf);
  const PhGroupPre p = ph_group_pre(nq, G);
  // the areas in order, none overlapping, the 64-bit one aligned, the read the leading words
  struct Area { uint64_t at; u128 len; } areas[] = {
      {p.head, PH_GROUP_HEAD_WORDS}, {p.gfirst, (u128)G + 1}, {p.gkey, G}, {p.gcount, G}, {p.gcum, 2 * ((u128)G + 1)}, {p.gerr, G},
      {p.keys, nq}, {p.skeys, nq}, {p.iota, nq}, {p.order, nq}, {p.flags, (u128)nq + 1}, {p.slots, (u128)nq + 1}, {p.safe, nq},
      {p.why, nq}};
  u128 at = 0;
  for (const Area &a : areas) {
    CHECK((u128)a.at >= at);
    at = (u128)a.at + a.len;
  }
  CHECK((u128)p.words >= at && (u128)p.words <= at + 16);
  CHECK(p.head == 0u && p.gcum % 2u == 0u);
  CHECK((u128)p.read_words == (u128)PH_GROUP_HEAD_WORDS + 3 * (u128)G + 1 && p.gcount + G == p.read_words);
  CHECK((u128)ph_group_post_bytes(nq, 1024, 1ull << 40) == (u128)nq * 1024 * 8 + ((u128)1 << 42));
}

// ---- the grouping pass, the lists and the select's indexing as the kernels do them, over exact-size arrays
struct Model {
  uint64_t nq, nf, n, nwords;
  std::vector<uint32_t> table, sel, qids;  // table: nf bitmaps, nwords apart
};

static void run_model(const Model &m, uint64_t budget, uint32_t nodes_knob, uint64_t bytes_knob, uint64_t want_rounds_at_least) {
  const uint64_t nq = m.nq, G = ph_group_max(nq, m.nf);
  const PhGroupPre lay = ph_group_pre(nq, G);
  std::vector<uint32_t> pre(lay.words, 0xDEADBEEFu);
  uint32_t *keys = &pre[lay.keys], *skeys = &pre[lay.skeys], *order = &pre[lay.order], *flags = &pre[lay.flags];
  uint32_t *slots = &pre[lay.slots], *why = &pre[lay.why], *gfirst = &pre[lay.gfirst], *gkey = &pre[lay.gkey];
  uint32_t *gcount = &pre[lay.gcount];
  // keys kernel
  for (uint64_t q = 0; q < nq; q++) {
    uint32_t key = ph_group_key(m.sel[q], m.nf), st = key == PH_GROUP_KEY_REJECT ? PH_GROUP_ST_SELECTOR : PH_GROUP_ST_OK;
    if (!m.qids.empty() && m.qids[q] >= m.n) key = PH_GROUP_KEY_REJECT, st = PH_GROUP_ST_MISSING;
    keys[q] = key, why[q] = st;
  }
  // the stable sort of (key, query)
  std::vector<uint32_t> perm(nq);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  for (uint64_t p = 0; p < nq; p++) order[p] = perm[p], skeys[p] = keys[perm[p]];
  // flags, their exclusive sum, heads
  for (uint64_t p = 0; p <= nq; p++) flags[p] = p < nq && (p == 0 || skeys[p] != skeys[p - 1]) ? 1u : 0u;
  uint32_t run = 0;
  for (uint64_t p = 0; p <= nq; p++) slots[p] = run, run += flags[p];
  const uint32_t ng = slots[nq];
  CHECK(ng >= 1u && ng <= G);
  pre[lay.head] = ng;
  gfirst[ng] = (uint32_t)nq;
  for (uint64_t p = 0; p < nq; p++)
    if (flags[p]) {
      CHECK(slots[p] < G);
      gfirst[slots[p]] = (uint32_t)p, gkey[slots[p]] = skeys[p];
    }
  // counts per group
  auto word = [&](uint32_t key, uint64_t w) -> uint32_t {
    if (key == PH_GROUP_KEY_REJECT) return 0u;
    uint32_t v = ph_group_key_has_bitmap(key, m.nf) ? m.table.at(ph_group_bitmap_at(key, (uint32_t)m.nwords) + w) : 0xFFFFFFFFu;
    const uint64_t first = w * 32u;
    if (first >= m.n) return 0u;
    if (m.n - first < 32u) v &= (1u << (m.n - first)) - 1u;
    return v;
  };
  for (uint32_t g = 0; g < ng; g++) {
    uint32_t c = 0;
    for (uint64_t w = 0; w < m.nwords; w++) c += (uint32_t)__builtin_popcount(word(gkey[g], w));
    gcount[g] = c;
  }
  // groups: ascending keys, contiguous, sizes add up; every query sits in the group of its key, in query order
  uint64_t total = 0;
  for (uint32_t g = 0; g < ng; g++) {
    CHECK(gfirst[g] < gfirst[g + 1] && (g == 0 || gkey[g - 1] < gkey[g]));
    for (uint32_t p = gfirst[g]; p < gfirst[g + 1]; p++) {
      CHECK(keys[order[p]] == gkey[g]);
      if (p > gfirst[g]) CHECK(order[p - 1] < order[p]);
    }
    total += gfirst[g + 1] - gfirst[g];
  }
  CHECK(total == nq && gfirst[0] == 0u);
  // rounds and the CSR lists, then the select's reads and writes per group
  uint64_t rounds = 0;
  const uint64_t list_bytes = ph_group_list_bytes(gcount, ng, m.nwords, budget, &rounds);
  CHECK(rounds >= want_rounds_at_least);
  std::vector<uint32_t> lists(list_bytes / 4u, 0xDEADBEEFu);
  uint64_t table_floats = 0;
  for (uint32_t g = 0; g < ng; g++)
    if (gcount[g])
      table_floats = std::max(table_floats, ph_dense_plan(gcount[g], gfirst[g + 1] - gfirst[g], nodes_knob, bytes_knob).table_floats);
  const uint32_t k = 3;
  std::vector<uint64_t> keyscratch(ph_group_key_bytes(nq, k) / 8u, 0);
  std::vector<float> D(table_floats, 0.f);
  std::vector<uint32_t> written(nq, 0u);
  for (uint64_t g0 = 0; g0 < ng;) {
    const uint64_t g1 = ph_group_round_end(gcount, ng, g0, m.nwords, budget);
    uint32_t *const off = lists.data();
    const uint64_t off_words = ph_group_round_off_words(g0, g1, m.nwords);
    uint64_t list_at = 0;
    for (uint64_t g = g0; g < g1; g++) {
      uint32_t *const o = off + (g - g0) * ph_group_off_words(m.nwords);
      uint32_t sum = 0;
      for (uint64_t w = 0; w < m.nwords; w++) o[w] = sum, sum += (uint32_t)__builtin_popcount(word(gkey[g], w));
      o[m.nwords] = sum;
      CHECK(sum == gcount[g]);
      uint32_t *const list = lists.data() + off_words + list_at;
      for (uint64_t w = 0; w < m.nwords; w++) {
        uint32_t at = o[w];
        for (uint32_t t = word(gkey[g], w); t; t &= t - 1u) list[at++] = (uint32_t)w * 32u + (uint32_t)__builtin_ctz(t);
        CHECK(at == o[w + 1]);
      }
      for (uint32_t i = 0; i < gcount[g]; i++) CHECK(list[i] < m.n && (i == 0 || list[i - 1] < list[i]));
      // the tables and the select of this group
      const uint64_t first = gfirst[g], size = gfirst[g + 1] - first;
      if (!gcount[g]) {
        for (uint64_t p = 0; p < size; p++) written[order[first + p]]++;
      } else {
        const PhDensePlan plan = ph_dense_plan(gcount[g], size, nodes_knob, bytes_knob);
        for (uint32_t i = 0; i < plan.node_chunks; i++) {
          uint64_t nfirst;
          uint32_t tn, stride;
          ph_dense_node_chunk(plan, i, &nfirst, &tn, &stride);
          CHECK(nfirst + tn <= gcount[g]);
          for (uint64_t j = 0; j < plan.pos_chunks; j++) {
            uint64_t pfirst;
            uint32_t npos;
            ph_dense_pos_chunk(plan, j, &pfirst, &npos);
            const uint32_t *const ord = order + first + pfirst;
            for (uint32_t p = 0; p < npos; p++) {
              const uint32_t q = ord[p];
              CHECK(q < nq);
              D.at((uint64_t)p * stride + tn - 1u) += (float)list[nfirst + tn - 1u];  // the row's last entry, the chunk's last id
              keyscratch.at((uint64_t)q * k + k - 1u)++;
              if (i + 1u == plan.node_chunks) written[q]++;
            }
          }
        }
      }
      list_at += gcount[g];
    }
    CHECK((off_words + list_at) * 4u <= list_bytes);
    g0 = g1;
  }
  for (uint64_t q = 0; q < nq; q++) CHECK(written[q] == 1u);  // every row written exactly once, refused queries included
}

static Model make_model(uint64_t nq, uint64_t nf, uint64_t n, uint32_t seed, bool stored, bool bad) {
  std::mt19937 rng(seed);
  Model m;
  m.nq = nq, m.nf = nf, m.n = n, m.nwords = (n + 31u) / 32u;
  m.table.resize(nf * m.nwords);
  for (uint64_t f = 0; f < nf; f++) {
    const uint32_t dens = (uint32_t)(f % 5u);  // 0: empty, 4: full
    for (uint64_t w = 0; w < m.nwords; w++) {
      uint32_t v = dens == 0 ? 0u : dens == 4 ? 0xFFFFFFFFu : rng();
      if (dens == 1) v &= rng() & rng();
      m.table[f * m.nwords + w] = v;
    }
  }
  m.sel.resize(nq);
  for (uint64_t q = 0; q < nq; q++) {
    const uint32_t r = rng() % (uint32_t)(nf + 1u);
    m.sel[q] = r == nf ? PH_GROUP_SELECT_ALL : r;
    if (bad && q % 7u == 3u) m.sel[q] = q % 2u ? (uint32_t)nf : 0xFFFFFFFEu;
  }
  if (stored) {
    m.qids.resize(nq);
    for (uint64_t q = 0; q < nq; q++) m.qids[q] = bad && q % 11u == 5u ? (uint32_t)(n + q) : rng() % (uint32_t)n;
  }
  return m;
}

int main() {
  check_keys();
  // rounds: the tests' shapes, random counts, one group larger than the budget, the largest counts
  const uint64_t nw = 157;
  CHECK(check_rounds({0, 1, 65, 1500, 5000, 5000, 0}, nw, PH_GROUP_LIST_BYTES_DEFAULT) == 1u);
  CHECK(check_rounds({0, 1, 65, 1500, 5000}, nw, 4u * (5000u + nw + 1u)) >= 2u);
  CHECK(check_rounds({0, 1, 65, 1500, 5000}, nw, 1) == 5u);  // every group exceeds it: one each
  CHECK(check_rounds({700, 700}, nw, 4u * (700u + nw + 1u)) == 2u);
  CHECK(check_rounds({5000}, nw, 16) == 1u);
  CHECK(check_rounds({0x7FFFFFFFu, 0x7FFFFFFFu, 0x7FFFFFFFu}, 1ull << 26, PH_GROUP_LIST_BYTES_MAX) == 3u);
  CHECK(check_rounds({0x7FFFFFFFu, 0x7FFFFFFFu, 0x7FFFFFFFu}, 1ull << 26, ~0ull) == 1u);  // no wrap at a budget of 2^64 - 1
  CHECK(check_rounds(std::vector<uint32_t>(PH_GROUP_ROUND_GROUPS_MAX + 5u, 0u), 0, PH_GROUP_LIST_BYTES_DEFAULT) == 2u);  // the grid's limit
  std::mt19937 rng(12345);
  for (int it = 0; it < 300; it++) {
    std::vector<uint32_t> counts(1u + rng() % 40u);
    for (uint32_t &c : counts) c = rng() % 3u ? rng() % 6000u : 0u;
    check_rounds(counts, rng() % 300u, 1u + rng() % 60000u);
  }
  // scratch sizes at the edges of the argument ranges
  const uint64_t nqs[] = {1, 2, 65, 600, PH_GROUP_NQ_MAX, 0xFFFFFFFFull}, nfs[] = {1, 5, 257, 0xFFFFFFFEull};
  for (uint64_t nq : nqs)
    for (uint64_t nf : nfs) check_pre(nq, nf);
  // host models over exact-size arrays
  for (uint32_t seed = 0; seed < 6; seed++) {
    run_model(make_model(65, 5, 5000, seed, seed & 1u, false), PH_GROUP_LIST_BYTES_DEFAULT, 8192, PH_DENSE_TABLE_BYTES_DEFAULT, 1);
    run_model(make_model(65, 5, 5000, seed, seed & 1u, true), 4u * (5000u + 157u + 1u), 64, 64u * 4u * 11u, 3);
    run_model(make_model(600, 257, 1000, seed, true, true), 1, 128, 1, 100);
    run_model(make_model(1, 1, 33, seed, false, false), 1, 64, 1, 1);
    run_model(make_model(7, 300, 31, seed, false, true), 1000, 64, 1000, 1);
  }
  printf("ALL OK\n");
  return 0;
}
