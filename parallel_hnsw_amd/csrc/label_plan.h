// How the exact search by row label (filter_labeled.hip) is cut: pure integer rules, shared by the launcher, the
// kernels and tests/cpp/test_label_plan.cpp (which runs them under the host sanitizers, no GPU).
//
// Every vector carries one u32 label; the posting lists are the ascending VectorIds of every label in CSR form:
// values[nlabels] ascending, first[nlabels + 1], ids[listed].  A query wants one label; its SLOT is the index of that
// label in values[], or PH_LABEL_SLOT_NONE (a label nobody carries, PHNSW_LABEL_NONE, a Stored query id past n).
//
// A list of `len` ids is read in BATCHES of 64 (one id per lane of a wave64).  The batches are dealt to `slices` waves
// as exact_slices.h deals the passes of a bitmap.  The batch is sorted by slot; the positions of one slot are cut into
// TILES of at most T queries, and a wave of the tile kernel reads every row of its slice once for the whole tile.
#pragma once
#include <stdint.h>

#include "exact_slices.h"

#define PH_LABEL_SLOT_NONE 0xFFFFFFFFu
#define PH_LABEL_BATCH 64u
#define PH_LABEL_LDS_BYTES (160u * 1024u)  // a workgroup's LDS on gfx950
#define PH_LABEL_TILE_CAP 16u              // default cap on T (PHNSW_LABEL_TILE)
#define PH_LABEL_TILE_WAVES 4u             // tile waves a CU should hold: T is sized to a quarter of the LDS
#define PH_LABEL_NQ_MAX 0x7FFFFFFEull      // queries of one call (the sort counts in int)

PH_EXACT_HD static inline uint64_t ph_label_batches(uint64_t len) { return (len + PH_LABEL_BATCH - 1u) / PH_LABEL_BATCH; }

// partition_point: the first index whose value is not below `want`
PH_EXACT_HD static inline uint64_t ph_label_lower_bound(const uint32_t *values, uint64_t n, uint32_t want) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2u;
    if (values[mid] < want)
      lo = mid + 1u;
    else
      hi = mid;
  }
  return lo;
}

// the slot of a wanted label; none_label = PHNSW_LABEL_NONE
PH_EXACT_HD static inline uint32_t ph_label_slot(const uint32_t *values, uint64_t nlabels, uint32_t want, uint32_t none_label) {
  if (want == none_label) return PH_LABEL_SLOT_NONE;
  const uint64_t i = ph_label_lower_bound(values, nlabels, want);
  return i < nlabels && values[i] == want ? (uint32_t)i : PH_LABEL_SLOT_NONE;
}

// the query a lookup position stands for: the position itself, or -- the subset form of a call -- the entry of the
// caller's list; the sort then carries it and every later kernel addresses by order[pos]
PH_EXACT_HD static inline uint32_t ph_label_seed(const uint32_t *list, uint32_t p) { return list ? list[p] : p; }

// LDS of the per-query scan besides a PQ store's table: two key lists of k entries and 64 sorted survivor keys
PH_EXACT_HD static inline uint64_t ph_label_scan_lds(uint64_t k) { return 2u * k * 8u + 64u * 8u; }
// LDS one query of a tile takes: its row of ld f32 values, the scan's lists, 64 collected distances, four state words
PH_EXACT_HD static inline uint64_t ph_label_tile_query_lds(uint64_t k, uint64_t ld) {
  return ld * 4u + ph_label_scan_lds(k) + 64u * 4u + 16u;
}
PH_EXACT_HD static inline uint64_t ph_label_tile_lds(uint64_t T, uint64_t k, uint64_t ld) {
  return T * ph_label_tile_query_lds(k, ld);
}

// T: queries of one label a wave of the tile kernel serves.  As many as a quarter of the LDS holds, so that a CU keeps
// four tile waves, at most the cap (knob > 0: PHNSW_LABEL_TILE, else PH_LABEL_TILE_CAP), at least 1.  1 = the per-query
// scan.  Never grows with k or with the row length.
static inline uint32_t ph_label_tile(uint64_t k, uint64_t ld, uint64_t lds_bytes, long long knob) {
  const uint64_t cap = knob > 0 ? (uint64_t)knob : (uint64_t)PH_LABEL_TILE_CAP;
  uint64_t t = (lds_bytes / PH_LABEL_TILE_WAVES) / ph_label_tile_query_lds(k, ld);
  if (t > cap) t = cap;
  if (t > 0xFFFFu) t = 0xFFFFu;
  return t ? (uint32_t)t : 1u;
}

// slices per work item (a query, or a tile): ph_exact_slice_count over the batches of the longest list
static inline uint32_t ph_label_slice_count(uint64_t items, uint64_t resident, uint64_t longest, long long forced) {
  return ph_exact_slice_count(items, resident, ph_label_batches(longest), forced);
}
// batches of slice `slice` of a list of len ids: [*b0, *b1)
PH_EXACT_HD static inline void ph_label_slice_range(uint32_t slice, uint32_t slices, uint64_t len, uint64_t *b0, uint64_t *b1) {
  ph_exact_slice_range(slice, slices, ph_label_batches(len), b0, b1);
}

// ---- the tile cut over the sorted slots sslot[0 .. nq): position p belongs to the group of its slot, which starts at
// the first position holding that slot; every T-th position of a group heads a tile
PH_EXACT_HD static inline uint64_t ph_label_group_start(const uint32_t *sslot, uint64_t p) {
  return ph_label_lower_bound(sslot, p, sslot[p]);
}
PH_EXACT_HD static inline bool ph_label_tile_head(const uint32_t *sslot, uint64_t p, uint32_t T) {
  return (p - ph_label_group_start(sslot, p)) % T == 0u;
}
// queries of the tile that position p heads: <= T, all of p's slot
PH_EXACT_HD static inline uint32_t ph_label_tile_size(const uint32_t *sslot, uint64_t nq, uint64_t p, uint32_t T) {
  uint32_t c = 1;
  while (c < T && p + c < nq && sslot[p + c] == sslot[p]) c++;
  return c;
}

// ---- scratch of one call; every figure in 64 bits, false = it does not fit
// words of the grouping block: slot, sslot, iota, order, tile_first [nq] each, flags and tidx [nq + 1] each, head [4]
struct PhLabelPre {
  uint64_t slot, sslot, iota, order, tile_first, flags, tidx, head, words;
};
static inline PhLabelPre ph_label_pre(uint64_t nq) {
  PhLabelPre l;
  uint64_t at = 0;
  l.head = at, at += 4u;
  l.slot = at, at += nq;
  l.sslot = at, at += nq;
  l.iota = at, at += nq;
  l.order = at, at += nq;
  l.tile_first = at, at += nq;
  l.flags = at, at += nq + 1u;
  l.tidx = at, at += nq + 1u;
  l.words = at;
  return l;
}
// bytes of the per-slice key lists [nq][slices][k]
static inline bool ph_label_key_bytes(uint64_t nq, uint64_t slices, uint64_t k, uint64_t *bytes) {
  if (nq > PH_LABEL_NQ_MAX || k > PH_EXACT_KMAX || slices > 0xFFFFFFFFull) return false;
  const uint64_t per = slices * k * 8u;  // < 2^32 * 2^10 * 2^3
  if (per && nq > UINT64_MAX / per) return false;
  *bytes = nq * per;
  return true;
}
