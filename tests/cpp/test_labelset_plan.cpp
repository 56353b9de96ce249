// Stand-alone host check of the integer rules behind the exact search by label SETS (parallel_hnsw_amd/csrc/
// labelset_plan.h, the header the launcher and the kernels include): compiled with -fsanitize=address,undefined and run
// without a GPU (tests/test_labelset_plan_cpp.py).  Which query a pair belongs to, at range borders and with offsets
// that cannot be trusted; a host model of the call -- claim, slot, stable sort, duplicate flags, inverse, gather per
// query -- against a brute-force union; the scratch sizes at the largest batch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <set>
#include <vector>

#include "../../parallel_hnsw_amd/csrc/labelset_plan.h"

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

static const uint32_t NONE = 0xFFFFFFFFu;

// the claim kernel, one query after another in the given order (the device's order is not fixed: min is what makes the
// outcome independent of it)
static std::vector<uint32_t> claim_all(const std::vector<uint32_t> &first, uint64_t nwant, const std::vector<uint32_t> &order) {
  std::vector<uint32_t> owner(nwant, PH_LABELSET_OWNER_NONE);
  for (uint32_t q : order) {
    const uint32_t b = first[q], e = first[q + 1u];
    if (!ph_labelset_range_ok(b, e, nwant)) continue;
    for (uint32_t i = b; i < e; i++)
      if (!ph_labelset_claim(owner.data(), i, q)) break;
  }
  return owner;
}
static bool query_ok(const std::vector<uint32_t> &first, const std::vector<uint32_t> &owner, uint32_t q) {
  const uint32_t b = first[q], e = first[q + 1u];
  if (!ph_labelset_range_ok(b, e, owner.size())) return false;
  for (uint32_t i = b; i < e; i++)
    if (owner[i] != q) return false;
  return true;
}
static std::vector<uint32_t> iota(uint32_t n) {
  std::vector<uint32_t> v(n);
  std::iota(v.begin(), v.end(), 0u);
  return v;
}

static void test_pair_to_query() {
  // empty ranges at the front, in the middle and at the end; every border
  const std::vector<uint32_t> first = {0, 0, 0, 3, 3, 4, 9, 9, 9};
  const uint64_t nq = first.size() - 1u, nwant = 9;
  CHECK(ph_labelset_first_bad(first.data(), nq) == nq);
  const std::vector<uint32_t> owner = claim_all(first, nwant, iota((uint32_t)nq));
  const uint32_t expect[9] = {2, 2, 2, 4, 5, 5, 5, 5, 5};
  for (uint32_t i = 0; i < 9; i++) CHECK(owner[i] == expect[i]);
  for (uint32_t q = 0; q < nq; q++) CHECK(query_ok(first, owner, q));
  // any order of the queries gives the same owners
  std::vector<uint32_t> rev = iota((uint32_t)nq);
  std::reverse(rev.begin(), rev.end());
  CHECK(claim_all(first, nwant, rev) == owner);
  // nothing wanted at all
  const std::vector<uint32_t> none = {0, 0, 0};
  CHECK(claim_all(none, 0, iota(2)).empty());
  CHECK(ph_labelset_first_bad(none.data(), 2) == 2);
  const std::vector<uint32_t> zero = {0};
  CHECK(ph_labelset_first_bad(zero.data(), 0) == 0);  // nq == 0: none is bad
}

static void test_validity() {
  CHECK(ph_labelset_range_ok(0, 0, 0) && ph_labelset_range_ok(0, 5, 5) && ph_labelset_range_ok(5, 5, 5));
  CHECK(!ph_labelset_range_ok(3, 2, 5));                                     // backwards
  CHECK(!ph_labelset_range_ok(0, 6, 5) && !ph_labelset_range_ok(6, 6, 5));   // past nwant
  CHECK(!ph_labelset_range_ok(0xFFFFFFFFu, 0, 5) && !ph_labelset_range_ok(0, 0xFFFFFFFFu, 0x7FFFFFFEu));
  CHECK(ph_labelset_range_ok(0, 0x7FFFFFFEu, 0x7FFFFFFEu));
  // the host form's refusals name the first bad query
  const std::vector<uint32_t> a = {1, 2, 3}, b = {0, 2, 1, 3}, c = {0, 2, 2, 1}, d = {0, 1, 2, 3};
  CHECK(ph_labelset_first_bad(a.data(), 2) == 0);  // want_first[0] != 0
  CHECK(ph_labelset_first_bad(b.data(), 3) == 1);
  CHECK(ph_labelset_first_bad(c.data(), 3) == 2);
  CHECK(ph_labelset_first_bad(d.data(), 3) == 3);

  // the device form: one offset out of place spoils the two queries beside it and nobody else.  Honest offsets
  // {0,2,4,6,8,10}; want_first[3] = nwant + 7 makes query 2 run past nwant and query 3 run backwards
  std::vector<uint32_t> first = {0, 2, 4, 17, 8, 10};
  std::vector<uint32_t> owner = claim_all(first, 10, iota(5));
  const uint32_t expect[10] = {0, 0, 1, 1, NONE, NONE, NONE, NONE, 4, 4};
  for (uint32_t i = 0; i < 10; i++) CHECK(owner[i] == expect[i]);
  CHECK(query_ok(first, owner, 0) && query_ok(first, owner, 1) && query_ok(first, owner, 4));
  CHECK(!query_ok(first, owner, 2) && !query_ok(first, owner, 3));
  // want_first[0] != 0 on the device: query 0 is sound as a range, pairs below it belong to nobody
  first = {1, 2, 3};
  owner = claim_all(first, 3, iota(2));
  CHECK(owner[0] == NONE && owner[1] == 0 && owner[2] == 1);
  // sound ranges that overlap: the lowest query keeps the shared pairs, every other one is refused, in any order
  first = {0, 4, 2, 6};  // q0 [0,4), q1 backwards, q2 [2,6)
  for (int pass = 0; pass < 2; pass++) {
    std::vector<uint32_t> order = iota(3);
    if (pass) std::reverse(order.begin(), order.end());
    owner = claim_all(first, 6, order);
    CHECK(owner[0] == 0 && owner[1] == 0 && owner[2] == 0 && owner[3] == 0);
    CHECK(query_ok(first, owner, 0) && !query_ok(first, owner, 1) && !query_ok(first, owner, 2));
  }
  // a claim that meets a lower owner stops, one that meets a higher or none goes on
  CHECK(!ph_labelset_claim_goes_on(3, 5) && ph_labelset_claim_goes_on(7, 5) && ph_labelset_claim_goes_on(NONE, 5));
}

// steps 1, 2 and 4 on the host: the candidate ids of every query as the merge gathers them, against the union
static void test_model_against_a_union() {
  // posting lists: values ascending, list of label values[s] = ids first[s] .. first[s + 1)
  const std::vector<uint32_t> values = {3, 7, 8, 100, 0xFFFFFFFEu};
  const std::vector<uint32_t> lfirst = {0, 2, 2 + 5, 7 + 1, 8 + 4, 12 + 3};
  uint64_t state = 99;
  auto rnd = [&](uint32_t m) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((state >> 33) % m);
  };
  const uint32_t pool[] = {3, 7, 8, 100, 0xFFFFFFFEu, 5, 9, NONE, 0};  // carried labels, absent ones, NONE
  for (int round = 0; round < 200; round++) {
    const uint32_t nq = 1u + rnd(12);
    std::vector<uint32_t> first(nq + 1u, 0u), want;
    for (uint32_t q = 0; q < nq; q++) {
      const uint32_t len = rnd(4) ? rnd(7) : 0u;  // empty sets too
      for (uint32_t j = 0; j < len; j++) want.push_back(pool[rnd(9)]);  // duplicates happen
      first[q + 1u] = (uint32_t)want.size();
    }
    const uint64_t nwant = want.size();
    const PhLabelsetPre lay = ph_labelset_pre(nwant);
    std::vector<uint32_t> pre(lay.words, 0xDEADBEEFu);
    // 1: claim, slot
    const std::vector<uint32_t> owner = claim_all(first, nwant, iota(nq));
    for (uint64_t i = 0; i < nwant; i++) {
      pre[lay.owner + i] = owner[i];
      pre[lay.pos.slot + i] = ph_label_slot(values.data(), values.size(), want[i], NONE);
      pre[lay.pos.iota + i] = (uint32_t)i;
    }
    // 2: stable sort by slot, then per position its query, the inverse, the duplicate flag
    std::vector<uint32_t> perm = iota((uint32_t)nwant);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return pre[lay.pos.slot + x] < pre[lay.pos.slot + y]; });
    for (uint64_t p = 0; p < nwant; p++) {
      pre[lay.spair + p] = perm[p];
      pre[lay.pos.sslot + p] = pre[lay.pos.slot + perm[p]];
    }
    for (uint64_t p = 0; p < nwant; p++) {
      const uint32_t i = pre[lay.spair + p], q = pre[lay.owner + i];
      pre[lay.pos.order + p] = q;
      pre[lay.inv + i] = (uint32_t)p;
      pre[lay.dup + p] = p > 0 && ph_labelset_dup(pre[lay.pos.sslot + p], q, pre[lay.pos.sslot + p - 1u],
                                                  pre[lay.owner + pre[lay.spair + p - 1u]]);
    }
    for (uint64_t i = 0; i < nwant; i++) CHECK(pre[lay.spair + pre[lay.inv + i]] == i);
    // 4: per query the ids of its positions, duplicates and slot-less pairs left out
    for (uint32_t q = 0; q < nq; q++) {
      CHECK(query_ok(first, owner, q));
      std::vector<uint32_t> got;
      uint64_t count = 0;
      for (uint32_t i = first[q]; i < first[q + 1u]; i++) {
        const uint32_t pos = pre[lay.inv + i];
        CHECK(pre[lay.pos.order + pos] == q);
        const uint32_t s = pre[lay.pos.sslot + pos];
        if (pre[lay.dup + pos] || s == PH_LABEL_SLOT_NONE) continue;
        count += lfirst[s + 1u] - lfirst[s];
        for (uint32_t j = lfirst[s]; j < lfirst[s + 1u]; j++) got.push_back(j);
      }
      std::set<uint32_t> labels(want.begin() + first[q], want.begin() + first[q + 1u]);
      std::vector<uint32_t> expect;
      for (uint32_t w : labels)
        for (size_t s = 0; s < values.size(); s++)
          if (w != NONE && values[s] == w)
            for (uint32_t j = lfirst[s]; j < lfirst[s + 1u]; j++) expect.push_back(j);
      std::sort(got.begin(), got.end());
      std::sort(expect.begin(), expect.end());
      CHECK(got == expect);  // every candidate once
      CHECK(count == expect.size());
    }
  }
}

static void test_scratch_sizes() {
  const uint64_t big = PH_LABELSET_NWANT_MAX;  // 2^31 - 2
  CHECK(big == 0x7FFFFFFEull);
  const PhLabelsetPre lay = ph_labelset_pre(big);
  CHECK(lay.words == 4u + 5u * big + 2u * (big + 1u) + 4u * big);  // 44 bytes per pair: no wrap in 64 bits
  CHECK(lay.pos.words == lay.owner && lay.owner + big == lay.spair && lay.spair + big == lay.inv && lay.inv + big == lay.dup &&
        lay.dup + big == lay.words);
  const PhLabelsetPre none = ph_labelset_pre(0);
  CHECK(none.words == 6u && none.owner == 6u);
  uint64_t bytes = 0;
  CHECK(ph_labelset_key_bytes(big, 1, 1024, &bytes) && bytes == big * 1024u * 8u);
  CHECK(ph_labelset_key_bytes(big, 1ull << 20, 1024, &bytes) && bytes == big << 33);  // 2^64 - 2^34: the last that fits
  bytes = 12345;
  CHECK(!ph_labelset_key_bytes(big, (1ull << 20) + 1u, 1024, &bytes) && bytes == 12345);  // one slice more wraps: refused
  CHECK(ph_labelset_key_bytes(65, 3, 10, &bytes) && bytes == 65u * 3u * 10u * 8u);
  CHECK(ph_labelset_key_bytes(0, 7, 10, &bytes) && bytes == 0);
  bytes = 12345;
  CHECK(!ph_labelset_key_bytes(big, 0xFFFFFFFFull, 1024, &bytes) && bytes == 12345);  // 2^31 * 2^32 * 2^13: refused
  CHECK(!ph_labelset_key_bytes(big, 1ull << 22, 1024, &bytes) && bytes == 12345);     // 2^31 * 2^22 * 2^13 = 2^66
  CHECK(!ph_labelset_key_bytes(big + 1u, 1, 1, &bytes));
  CHECK(!ph_labelset_key_bytes(1, 1, 1025, &bytes));
  CHECK(!ph_labelset_key_bytes(1, 1ull << 32, 1, &bytes));
}

int main() {
  test_pair_to_query();
  test_validity();
  test_model_against_a_union();
  test_scratch_sizes();
  std::printf("ALL OK\n");
  return 0;
}
