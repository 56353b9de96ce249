// How the exact radius search over LISTS of row ids (filter_list_radius.hip: by row label, by numeric range) sizes its
// record pool and runs its staging buffer: pure integer rules, shared by the launcher, the kernel and
// tests/cpp/test_list_radius_plan.cpp (which runs them under the host sanitizers, no GPU).
//
// The records, the pool's layout and the sort are radius_plan.h's; there is no table block behind the pool.  What is
// new: the pool is sized from what the HANDLE knows on the host -- no candidate count is read back --, and a wave keeps
// its hits in a small LDS buffer and reserves pool space once per FLUSH, not once per batch of 64 rows.
#pragma once
#include <stdint.h>

#include "exact_slices.h"
#include "radius_plan.h"

#define PH_LIST_RADIUS_STAGE 256u  // keys a wave stages before it flushes: 2 KiB of LDS, four full batches
#define PH_LIST_RADIUS_BATCH 64u   // hits one batch adds at most (PH_LABEL_BATCH)

// Records the pool holds: min(cap, nq x longest), `longest` the longest list a query of the handle can have.  The
// product saturates: nq < 2^32 and longest < 2^32 in every call, but the rule holds for any pair.
static inline uint64_t ph_list_radius_pool_records(uint64_t cap, uint64_t nq, uint64_t longest) {
  if (!nq || !longest) return 0u;
  const uint64_t pairs = nq > UINT64_MAX / longest ? UINT64_MAX : nq * longest;
  return cap < pairs ? cap : pairs;
}

// the scratch behind the lookup arrays: radius_plan.h's layout with no table block
static inline PhRadiusLayout ph_list_radius_layout(uint64_t nq, uint64_t records) { return ph_radius_layout(nq, records, 0u); }

// The staging buffer.  `staged` keys wait in it (<= PH_LIST_RADIUS_STAGE); a batch brings `hits` more (<= 64).  The
// buffer is flushed BEFORE the batch's keys go in when they would not fit, and once more at the end of the item when
// anything is left; so every key is staged exactly once, and a flush never carries more than the buffer holds.
PH_EXACT_HD static inline bool ph_list_radius_flush_first(uint32_t staged, uint32_t hits) { return staged + hits > PH_LIST_RADIUS_STAGE; }

// what an item does over batches bringing hits[0 .. nb): the flushes it makes (atomics on the cursor) and the largest
// flush; *total = every key, each counted once
struct PhListRadiusFlushes {
  uint64_t flushes, total;
  uint32_t largest;
};
static inline PhListRadiusFlushes ph_list_radius_flushes(const uint32_t *hits, uint64_t nb) {
  PhListRadiusFlushes f = {0u, 0u, 0u};
  uint32_t staged = 0;
  for (uint64_t b = 0; b <= nb; b++) {
    const bool end = b == nb;
    const uint32_t h = end ? 0u : hits[b];
    if (end ? staged != 0u : ph_list_radius_flush_first(staged, h)) {
      f.flushes++, f.total += staged;
      if (staged > f.largest) f.largest = staged;
      staged = 0;
    }
    staged += h;
  }
  return f;
}
