// Exact top-k by ROW LABEL (phnsw_labels_*, phnsw_search_exact_labeled[_device]): the filter of a partition -- a tenant,
// a collection, an ACL class.  Every vector carries one u32 label and a query wants the rows of one label.  The
// candidate lists are a property of the data: posting lists in CSR form, built once per handle; a call derives nothing
// from a bitmap and reads nothing back.
//
//   listed under labels[v]  iff  v < n, labels[v] != PHNSW_LABEL_NONE, v a vector of the bottom layer
//   candidates of query q   =    the listed vectors of want[q], except exclude[q]
//   result                  =    the k candidates with the smallest (distance, id), ascending
//
//   construction  ph_label_key_kernel (the label, or NONE where the vector is not listed: label_of, kept with the
//                 handle for the label walk), stable radix sort of (label, id), ph_label_flags_kernel, exclusive sum,
//                 ph_label_heads_kernel: values, first, ids
//   a call     1. ph_labeled_lookup_kernel: per query the slot of its label (label_plan.h), radix sort of (slot, query):
//                 the queries of one label are adjacent positions; ph_labeled_tileflag_kernel, exclusive sum,
//                 ph_labeled_tiles_kernel: the tile table and its count, on the device
//              2. ph_labeled_scan_kernel: one wave64 per (position, slice of its list); ids 64 at a time from the
//                 posting list into dist.batch of the store's policy (ph_list_scan, list_scan.h: the loop the scan by
//                 range, filter_ranged.hip, runs over its spans) -- every store kind, and T = 1
//              3. ph_labeled_tile_kernel (f32 / f16 / i8 row stores, T > 1): one wave64 per (tile of up to T queries of
//                 ONE label, slice of that label's list); every candidate row is read once for the whole tile
//                 ph_list_merge_kernel (list_scan.h): the slices' lists of a position through the same running top-k
//
// Equality with phnsw_search_exact_filtered over the bitmap {v : labels[v] == want[q]}: the candidate sets are equal by
// the definition above, the keys are distinct, so the k smallest are one set in one order however the list is cut; the
// distances of path 2 are dist.batch's, and those of path 3 go through the same functions with the same operands in the
// same order (chain_partial with the row as x and the query as q, wave_sum4, finalize_metric), four rows at a time as
// batch_distances takes them.  The running top-k, what feeds it and what is written from it are exact_topk.h's, shared
// with filter_exact.hip and filter_dense.hip (profiles/exact_once/).
//
// A SET of labels per query (phnsw_search_exact_labelset[_device], phnsw_labels_count_set_device; labelset_plan.h): the
// lists of distinct labels are disjoint, so a set is more slices of the same scan.  A position of the sorted batch is a
// (query, wanted label) PAIR: ph_labelset_claim_kernel (which query owns a pair; the offsets are not trusted),
// ph_labelset_lookup_kernel, the same sort, ph_labelset_positions_kernel (the query of a position, the inverse
// permutation, duplicate flags), the tile table as above, the PAIRS instances of the scan and tile kernels -- every
// position writes its per-slice lists to scratch, none a row --, ph_labelset_merge_kernel: a wave per query merges the
// lists of its positions through the same running top-k.  Its subset form (PhLabelsetCall with c.list): the claim still
// runs over the whole batch -- which query owns a pair is a property of the batch --, ph_labelset_select_kernel marks the
// listed queries, the pairs of every other query get no slot and scan nothing, and the merge writes the listed rows alone.
//
// The graph walk by label (phnsw_search_batch_labeled[_device], at the end of this file) is the search kernels' own
// label mode (search_labeled.hip) over label_of, the walk by set (phnsw_search_batch_labelset[_device]) their set mode
// (search_labelset.hip); the routed calls (phnsw_search_labeled_auto, phnsw_search_labelset_auto) are filter_auto.hip's
// and take their scans from here through the subset forms (PhLabeledCall::list).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "exact_slices.h"
#include "exact_topk.h"
#include "filter_candidate.h"
#include "filter_route.h"
#include "host_call.h"
#include "label_plan.h"
#include "labelset_claim.h"
#include "labelset_plan.h"
#include "list_scan.h"
#include "phnsw_device.h"

struct phnsw_labels {
  const phnsw_index *ix = nullptr;  // the index the lists were made for, and what it looked like then
  uint64_t n = 0;
  uint32_t n_nodes = 0;
  int device = 0;
  uint64_t nlabels = 0, listed = 0, longest = 0;
  uint32_t *values = nullptr;  // [nlabels] ascending
  uint32_t *first = nullptr;   // [nlabels + 1]
  uint32_t *ids = nullptr;     // [listed] (allocated [n]): ascending within a label
  uint32_t *label_of = nullptr;  // [n]: the label of a listed vector, PHNSW_LABEL_NONE elsewhere (the label walk's column)
  PhCallPool pool;  // PhLabeledSet, handed out by set_acquire's policy
  PhResidentMemo resident;  // under pool.mutex
};

// ------------------------------------------------------------------ construction

// (ph_label_key_kernel: list_scan.h, shared with the attribute handle)

// flags [n + 1]: 1 where a label starts (NONE sorts last and starts nothing); head[1] = listed, the first NONE position
__global__ __launch_bounds__(256) void ph_label_flags_kernel(const uint32_t *skeys, uint32_t n, uint32_t *flags, uint32_t *head) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p <= n; p += (uint64_t)gridDim.x * 256u) {
    const bool none = p == n || skeys[p] == PHNSW_LABEL_NONE;
    const bool none_before = p > 0 && skeys[p - 1u] == PHNSW_LABEL_NONE;
    flags[p] = !none && (p == 0 || skeys[p] != skeys[p - 1u]) ? 1u : 0u;
    if (none && !none_before) head[1] = (uint32_t)p;
  }
}

__global__ __launch_bounds__(256) void ph_label_heads_kernel(const uint32_t *skeys, const uint32_t *flags, const uint32_t *slots,
                                                             uint32_t n, uint32_t nlabels, uint32_t listed, uint32_t *values,
                                                             uint32_t *first) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p <= n; p += (uint64_t)gridDim.x * 256u) {
    if (p == n) {
      first[nlabels] = listed;
    } else if (flags[p]) {
      const uint32_t s = slots[p];
      if (s < nlabels) values[s] = skeys[p], first[s] = (uint32_t)p;
    }
  }
}

// ------------------------------------------------------------------ a call: lookup, grouping, tiles

struct PhLabeledArgs {
  PhDistArgs dist;
  const float *queries;  // [nq][ldq] or nullptr
  uint32_t ldq;
  const uint32_t *qids, *exclude, *want;  // [nq]; qids, exclude nullable
  const uint32_t *list;                   // nullable: the subset form -- position p of the lookup is query list[p]
  uint32_t nq, n, k, slices, T;
  // the posting lists
  const uint32_t *values, *first, *ids;
  uint32_t nlabels;
  // the grouping (label_plan.h)
  uint32_t *slot, *iota;            // [nq] by lookup position: its slot, its query (the position itself without a list)
  const uint32_t *sslot, *order;    // [nq] by position: its slot, its query
  uint32_t *flags;                  // [nq + 1]
  const uint32_t *tidx;             // [nq + 1]: exclusive sum of flags
  uint32_t *tile_first, *head;      // [nq]; head[0] = tiles
  uint32_t pq_lds;                  // bytes of dynamic LDS in front of the scan's own: a PQ store's table
  uint64_t *scratch;                // slices > 1: [nq positions][slices][k] keys, each list ascending, KEY_NONE padded
  uint32_t *out_ids;                // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
};

__global__ __launch_bounds__(256) void ph_labeled_lookup_kernel(PhLabeledArgs a) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < a.nq; p += (uint64_t)gridDim.x * 256u) {
    const uint32_t q = ph_label_seed(a.list, (uint32_t)p);  // every kernel after the sort addresses by order[pos]
    const bool bad_query = !a.queries && a.qids[q] >= a.n;
    a.slot[p] = bad_query ? PH_LABEL_SLOT_NONE : ph_label_slot(a.values, a.nlabels, a.want[q], PHNSW_LABEL_NONE);
    a.iota[p] = q;
  }
}

__global__ __launch_bounds__(256) void ph_labeled_tileflag_kernel(PhLabeledArgs a) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p <= a.nq; p += (uint64_t)gridDim.x * 256u)
    a.flags[p] = p < a.nq && ph_label_tile_head(a.sslot, p, a.T) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void ph_labeled_tiles_kernel(PhLabeledArgs a) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p <= a.nq; p += (uint64_t)gridDim.x * 256u) {
    if (p == a.nq)
      a.head[0] = a.tidx[p];
    else if (a.flags[p])
      a.tile_first[a.tidx[p]] = (uint32_t)p;  // tidx[p] < tiles <= nq
  }
}

__global__ __launch_bounds__(256) void ph_labeled_count_kernel(const uint32_t *values, const uint32_t *first, uint32_t nlabels,
                                                               const uint32_t *want, uint64_t nq, uint32_t *out_count) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * 256u) {
    const uint32_t s = ph_label_slot(values, nlabels, want[q], PHNSW_LABEL_NONE);
    out_count[q] = s == PH_LABEL_SLOT_NONE ? 0u : first[s + 1u] - first[s];
  }
}

// ------------------------------------------------------------------ path 2: the per-query list scan

// One wave64 per (position, slice of its list); work item = slice * nq + position (slice-major, position-minor, the
// positions label-major): the waves resident together read the same rows.
// PAIRS: the form of phnsw_search_exact_labelset -- a position is a (query, wanted label) pair, order[pos] the pair's
// query; a position never writes a row, its lists go to the scratch at every slice count.
template <class Dist, bool PAIRS = false>
__global__ __launch_bounds__(64) void ph_labeled_scan_kernel(PhLabeledArgs a) {
  extern __shared__ float labeled_lds[];
  const uint32_t lane = threadIdx.x;
  uint64_t *const keys = (uint64_t *)((char *)labeled_lds + a.pq_lds);
  const uint64_t items = (uint64_t)a.nq * a.slices;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t pos = (uint32_t)(item % a.nq), slice = (uint32_t)(item / a.nq);
    const uint32_t q = a.order[pos], s = a.sslot[pos];
    __syncthreads();  // the previous item's LDS (table, lists) is done with
    const bool bad_query = !a.queries && a.qids[q] >= a.n;
    Dist dist;
    if (a.queries)
      dist.prepare_raw(a.dist, a.queries + (uint64_t)q * a.ldq, labeled_lds, lane);
    else if (!bad_query)
      dist.prepare_stored(a.dist, a.qids[q], labeled_lds, lane);
    const uint32_t at = s == PH_LABEL_SLOT_NONE ? 0u : a.first[s];
    const uint32_t len = s == PH_LABEL_SLOT_NONE ? 0u : a.first[s + 1u] - at;  // a bad query's slot is NONE
    ph_list_scan<PAIRS>(a, dist, keys, a.ids + at, len, q, pos, slice, bad_query, lane);  // list_scan.h
  }
}

// (the merge of the slices' lists: ph_list_merge_kernel, list_scan.h)

// ------------------------------------------------------------------ a SET of labels per query: pairs (labelset_plan.h)

// a = the block of the scan and tile kernels with nq = nwant POSITIONS; order[pos] is the query of the position's pair
struct PhLabelsetArgs {
  PhLabeledArgs a;
  const uint32_t *want_first, *want_values;  // [nq + 1], [nwant]: the caller's, untrusted
  uint32_t nq, nwant;
  uint32_t *owner;  // [nwant] by pair: the query that claimed it, PH_LABELSET_OWNER_NONE
  uint32_t *spair;  // [nwant] by position: its pair
  uint32_t *inv;    // [nwant] by pair: its position
  uint32_t *dup;    // [nwant] by position: 1 = the (slot, query) of the position before it
  // the subset form (a.list != nullptr): the rows of queries a.list[0 .. nlist) are made; sel [nq] = 1 for those
  const uint32_t *sel;
  uint32_t nlist;  // rows the merge writes: the list's length, nq without a list
};

// (which query owns a pair, the marks of the subset form: ph_labelset_claim_kernel, ph_labelset_select_kernel, labelset_claim.h)

// per pair: its slot (none for an unclaimed pair, for a bad Stored query id and for a query the list leaves out) and
// itself, the sort's value
__global__ __launch_bounds__(256) void ph_labelset_lookup_kernel(PhLabelsetArgs s) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < s.nwant; i += (uint64_t)gridDim.x * 256u) {
    const uint32_t q = s.owner[i];  // NONE or < nq
    const bool dead = q == PH_LABELSET_OWNER_NONE || (!s.a.queries && s.a.qids[q] >= s.a.n) || (s.sel && !s.sel[q]);
    s.a.slot[i] = dead ? PH_LABEL_SLOT_NONE : ph_label_slot(s.a.values, s.a.nlabels, s.want_values[i], PHNSW_LABEL_NONE);
    s.a.iota[i] = (uint32_t)i;
  }
}

// per position after the sort: its query (0 for an unclaimed pair, whose slot is none: it reads a row and scans
// nothing), the inverse permutation, the duplicate flag
__global__ __launch_bounds__(256) void ph_labelset_positions_kernel(PhLabelsetArgs s, uint32_t *order) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < s.nwant; p += (uint64_t)gridDim.x * 256u) {
    const uint32_t i = s.spair[p], q = s.owner[i];
    order[p] = q == PH_LABELSET_OWNER_NONE ? 0u : q;
    s.inv[i] = (uint32_t)p;
    s.dup[p] = p > 0 && ph_labelset_dup(s.a.sslot[p], q, s.a.sslot[p - 1u], s.owner[s.spair[p - 1u]]) ? 1u : 0u;
  }
}

// whether query q owns every pair of a sound range: what makes its row; wave-uniform
__device__ __forceinline__ bool ph_labelset_query_ok(const PhLabelsetArgs &s, uint32_t q, uint32_t b, uint32_t e, uint32_t lane) {
  return ph_labelset_owns_range(s.owner, s.nwant, q, b, e, lane);  // labelset_claim.h
}

// One wave per query: the lists of every position of its pairs -- duplicates and slot-less pairs left out -- through the
// same running top-k as ph_list_merge_kernel, so ties across lists fall in id order.  A refused query (labelset_plan.h)
// gets the empty row and status ST_LABELSET_RANGE.
#define ST_LABELSET_RANGE 8u
__global__ __launch_bounds__(64) void ph_labelset_merge_kernel(PhLabelsetArgs s) {
  extern __shared__ float labeled_lds[];
  const uint32_t lane = threadIdx.x;
  const PhLabeledArgs &a = s.a;
  uint64_t *const keys = (uint64_t *)labeled_lds;
  for (uint32_t at = blockIdx.x; at < s.nlist; at += gridDim.x) {
    const uint32_t q = a.list ? a.list[at] : at;
    if (q >= s.nq) continue;  // (a list holds query indices of the batch)
    const uint32_t b = s.want_first[q], e = s.want_first[q + 1u];
    const bool ok = ph_labelset_query_ok(s, q, b, e, lane);
    __syncthreads();
    PhExactTopK top;
    top.init(keys, a.k);
    for (uint32_t i = b; ok && i < e; i++) {
      const uint32_t pos = s.inv[i];  // < nwant: pair i is q's, so the sort placed it
      if (s.dup[pos] || a.sslot[pos] == PH_LABEL_SLOT_NONE) continue;
      for (uint32_t sl = 0; sl < a.slices; sl++)
        PH_EXACT_FEED(top, a.scratch + ((uint64_t)pos * a.slices + sl) * a.k, a.k, lane);
    }
    ph_exact_write_row(a, q, top.cur, top.len, !a.queries && a.qids[q] >= a.n, lane);
    if (!ok && lane == 0) a.status[q] = ST_LABELSET_RANGE;  // after the row's own status word, same lane
  }
}

// per query the list lengths of the distinct slots of its range; a refused range counts 0.  Distinct: no earlier pair
// of the range has the label -- sets are short, and the count needs no sort and no scratch.  One wave per query, a pair
// per lane.
__global__ __launch_bounds__(64) void ph_labelset_count_kernel(const uint32_t *values, const uint32_t *first, uint32_t nlabels,
                                                               const uint32_t *want_first, const uint32_t *want_values,
                                                               uint64_t nq, uint32_t nwant, uint32_t *out_count) {
  const uint32_t lane = threadIdx.x;
  for (uint64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    const uint32_t b = want_first[q], e = want_first[q + 1u];
    uint32_t c = 0;
    if (ph_labelset_range_ok(b, e, nwant))
      for (uint64_t i = (uint64_t)b + lane; i < e; i += 64u) {
        const uint32_t w = want_values[i];
        bool seen = false;
        for (uint32_t j = b; j < i && !seen; j++) seen = want_values[j] == w;
        if (seen) continue;
        const uint32_t sl = ph_label_slot(values, nlabels, w, PHNSW_LABEL_NONE);
        if (sl != PH_LABEL_SLOT_NONE) c += first[sl + 1u] - first[sl];
      }
    for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) out_count[q] = c;
  }
}

// the routed call by set: the count of a query that the scan would refuse (a range that is not sound, a pair a lower
// query holds) becomes 0, so that it is routed to the scan, which reports it.  owner[] as the claim kernel left it.
__global__ __launch_bounds__(64) void ph_labelset_refused_kernel(PhLabelsetArgs s, uint32_t *count) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t q = blockIdx.x; q < s.nq; q += gridDim.x) {
    const bool ok = ph_labelset_query_ok(s, q, s.want_first[q], s.want_first[q + 1u], lane);
    if (!ok && lane == 0) count[q] = 0u;
  }
}

// ------------------------------------------------------------------ path 3: the tile scan

// LDS of a tile wave: [T][ld] query values (what prepare_raw / prepare_stored would hold), then per query the scan's
// lists [2k + 64] keys, then [T][64] collected distances, then [T][4] state words {len, list in use, query, exclude}.
struct PhTileLds {
  float *qrow;
  uint64_t *keys;
  float *dbuf;
  uint32_t *state;
};

// Batches [b0, b1) of the list for the tsz queries of the tile.  The ids of a batch sit one per lane; with every lane
// below m a candidate, candidate g is lane g: batch_distances' compaction is the identity.  Four rows are in flight, as
// rows_partial loads them; each (row, query) pair then goes through chain_partial, wave_sum4 and finalize_metric with
// the operands batch_distances gives them.
template <int NV, class R, bool EXACT, bool L2>
__device__ __forceinline__ void ph_labeled_tile_batches(const PhLabeledArgs &a, const PhTileLds &l, uint32_t tsz,
                                                        const uint32_t *list, uint32_t len, uint64_t b0, uint64_t b1,
                                                        uint32_t lane) {
  const uint32_t nv4 = a.dist.nv4, keys_per = 2u * a.k + 64u;
  for (uint64_t b = b0; b < b1; b++) {
    const uint32_t j0 = (uint32_t)b * PH_LABEL_BATCH, j = j0 + lane;
    const uint32_t m = min(PH_LABEL_BATCH, len - j0);  // >= 1: b < batches of len
    const bool ok = lane < m;
    const uint32_t id = ok ? list[j] : 0u;  // a listed id: a row of the store
    const uint64_t off = (uint64_t)id * (uint64_t)a.dist.rows.stride;
    const uint32_t olo = (uint32_t)off, ohi = (uint32_t)(off >> 32);
    __syncthreads();  // the previous batch's distances have been taken
    for (uint32_t g = 0; g < m; g += 4u) {
      const typename R::chunk *r[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint32_t c = min(g + (uint32_t)u, m - 1u);  // short tail: the last row again (same value, unused)
        const uint64_t o = ((uint64_t)rl32(ohi, (int)c) << 32) | rl32(olo, (int)c);
        r[u] = (const typename R::chunk *)((const char *)a.dist.rows.base + o);
      }
      typename R::chunk raw[4][NV];
      typename R::aux ax[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        ax[u] = R::row_aux(r[u]);
#pragma unroll
        for (int k = 0; k < NV; k++) {
          uint32_t c = lane + 64u * k;
          if (!EXACT) c = c < nv4 ? c : nv4 - 1;
          raw[u][k] = R::load(r[u], c);
        }
      }
      float4 x[4][NV];
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int k = 0; k < NV; k++) x[u][k] = R::widen(raw[u][k], ax[u]);
      // where wave_sum4 leaves row u: lanes {0, 32, 16, 48}[u] + 0..15
      const uint32_t u_mine = (((lane >> 4) & 1u) << 1) | (lane >> 5);
      const bool writer = (lane & 15u) == 0u && g + u_mine < m;
      for (uint32_t t = 0; t < tsz; t++) {
        const float4 *const qr = (const float4 *)(l.qrow + (uint64_t)t * a.dist.ld);
        float4 qv[NV];
#pragma unroll
        for (int k = 0; k < NV; k++) {
          const uint32_t c = lane + 64u * k;
          qv[k] = (EXACT || c < nv4) ? qr[EXACT ? c : min(c, nv4 - 1u)] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float p[4];
#pragma unroll
        for (int u = 0; u < 4; u++) p[u] = chain_partial<NV, EXACT, L2>(x[u], qv, nv4, lane);
        const float d4 = finalize_metric(wave_sum4(p[0], p[1], p[2], p[3]), a.dist.metric);
        if (writer) l.dbuf[t * 64u + g + u_mine] = d4;
      }
    }
    __syncthreads();  // the batch's distances are there
    for (uint32_t t = 0; t < tsz; t++) {
      uint32_t *const st = l.state + 4u * t;
      uint64_t *const kb = l.keys + (uint64_t)t * keys_per;
      const uint32_t flip = rfl32(st[1]), ex = rfl32(st[3]);
      PhExactTopK top;
      top.init(kb, a.k);  // then as the state words left it: which list is in use, and its length
      if (flip) top.cur = kb + a.k, top.nxt = kb;
      top.len = rfl32(st[0]);
      const float d = l.dbuf[t * 64u + lane];
      top.insert(ok && id != ex ? mkkey(d, id) : KEY_NONE, lane);
      __syncthreads();
      if (lane == 0) st[0] = top.len, st[1] = top.cur == kb ? 0u : 1u;
    }
  }
}

// One wave64 per (tile, slice of the tile's list); work item = slice * nq + tile (nq bounds the tiles; the count is a
// device word), tiles label-major.
template <int NV, class R, bool PAIRS = false>
__global__ __launch_bounds__(64) void ph_labeled_tile_kernel(PhLabeledArgs a) {
  extern __shared__ float labeled_lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t keys_per = 2u * a.k + 64u;
  PhTileLds l;
  l.qrow = labeled_lds;
  l.keys = (uint64_t *)(l.qrow + (uint64_t)a.T * a.dist.ld);  // ld % 4 == 0: 16-byte aligned
  l.dbuf = (float *)(l.keys + (uint64_t)a.T * keys_per);
  l.state = (uint32_t *)(l.dbuf + a.T * 64u);
  const uint32_t ntiles = min(a.head[0], a.nq);
  const uint64_t items = (uint64_t)a.nq * a.slices;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t ti = (uint32_t)(item % a.nq), slice = (uint32_t)(item / a.nq);
    if (ti >= ntiles) continue;  // uniform over the wave
    const uint32_t p0 = a.tile_first[ti];  // < nq
    const uint32_t s = a.sslot[p0];
    const uint32_t tsz = ph_label_tile_size(a.sslot, a.nq, p0, a.T);
    __syncthreads();  // the previous item's LDS is done with
    for (uint32_t t = 0; t < tsz; t++) {
      const uint32_t q = a.order[p0 + t];
      float4 *const qr = (float4 *)(l.qrow + (uint64_t)t * a.dist.ld);
      const bool bad_query = !a.queries && a.qids[q] >= a.n;
      if (a.queries) {
        const float4 *const src = (const float4 *)(a.queries + (uint64_t)q * a.ldq);
        for (uint32_t c = lane; c < a.dist.nv4; c += 64u) qr[c] = src[c];
      } else if (!bad_query) {
        const typename R::chunk *row = R::row(a.dist.rows, a.qids[q]);
        const typename R::aux ax = R::row_aux(row);
        for (uint32_t c = lane; c < a.dist.nv4; c += 64u) qr[c] = R::widen(R::load(row, c), ax);
      }
      if (lane == 0) {
        uint32_t *const st = l.state + 4u * t;
        st[0] = 0u, st[1] = 0u, st[2] = q, st[3] = a.exclude ? a.exclude[q] : PH_EMPTY32;
      }
    }
    __syncthreads();
    const uint32_t at = s == PH_LABEL_SLOT_NONE ? 0u : a.first[s];
    const uint32_t len = s == PH_LABEL_SLOT_NONE ? 0u : a.first[s + 1u] - at;  // a bad query's slot is NONE
    const uint32_t *const list = a.ids + at;
    uint64_t b0, b1;
    ph_label_slice_range(slice, a.slices, len, &b0, &b1);
    const bool exact = a.dist.nv4 == 64u * NV, l2 = a.dist.metric == PHNSW_METRIC_L2;  // wave-uniform
    if (exact) {
      if (l2)
        ph_labeled_tile_batches<NV, R, true, true>(a, l, tsz, list, len, b0, b1, lane);
      else
        ph_labeled_tile_batches<NV, R, true, false>(a, l, tsz, list, len, b0, b1, lane);
    } else {
      if (l2)
        ph_labeled_tile_batches<NV, R, false, true>(a, l, tsz, list, len, b0, b1, lane);
      else
        ph_labeled_tile_batches<NV, R, false, false>(a, l, tsz, list, len, b0, b1, lane);
    }
    __syncthreads();
    for (uint32_t t = 0; t < tsz; t++) {
      const uint32_t *const st = l.state + 4u * t;
      const uint32_t tlen = rfl32(st[0]), q = rfl32(st[2]);
      const uint64_t *const cur = l.keys + (uint64_t)t * keys_per + (rfl32(st[1]) ? a.k : 0u);
      ph_exact_write_slice<PAIRS>(a, q, p0 + t, slice, cur, tlen, !a.queries && a.qids[q] >= a.n, lane);
    }
  }
}

// ------------------------------------------------------------------ launchers

typedef void (*PhLabeledFn)(PhLabeledArgs);
// pairs: the PAIRS instance, phnsw_search_exact_labelset's
template <template <int, int> class D>
static PhLabeledFn labeled_rows_fn(uint32_t nv4, bool pairs) {
  switch (ph_chunk_count(nv4)) {
    case 1: return pairs ? ph_labeled_scan_kernel<D<1, 4>, true> : ph_labeled_scan_kernel<D<1, 4>>;
    case 3: return pairs ? ph_labeled_scan_kernel<D<3, 4>, true> : ph_labeled_scan_kernel<D<3, 4>>;
    case 6: return pairs ? ph_labeled_scan_kernel<D<6, 4>, true> : ph_labeled_scan_kernel<D<6, 4>>;
    default: return nullptr;
  }
}
static PhLabeledFn labeled_scan_fn(const phnsw_store *s, bool pairs) {
  switch (s->kind) {
    case PH_ROWS_PQ: return pairs ? ph_labeled_scan_kernel<DistPQ, true> : ph_labeled_scan_kernel<DistPQ>;
    case PH_ROWS_F16: return labeled_rows_fn<DistF16>(s->ld / 4, pairs);
    case PH_ROWS_I8: return labeled_rows_fn<DistI8>(s->ld / 4, pairs);
    case PH_ROWS_I8Q: return labeled_rows_fn<DistI8Q>(s->ld / 4, pairs);
    default: return labeled_rows_fn<DistF32>(s->ld / 4, pairs);
  }
}
template <class R>
static PhLabeledFn labeled_tile_rows_fn(uint32_t nv4, bool pairs) {
  switch (ph_chunk_count(nv4)) {
    case 1: return pairs ? ph_labeled_tile_kernel<1, R, true> : ph_labeled_tile_kernel<1, R>;
    case 3: return pairs ? ph_labeled_tile_kernel<3, R, true> : ph_labeled_tile_kernel<3, R>;
    case 6: return pairs ? ph_labeled_tile_kernel<6, R, true> : ph_labeled_tile_kernel<6, R>;
    default: return nullptr;
  }
}
// the tile kernel of a store, nullptr where only the per-query scan serves it (i8q, PQ)
static PhLabeledFn labeled_tile_fn(const phnsw_store *s, bool pairs) {
  switch (s->kind) {
    case PH_ROWS_F32: return labeled_tile_rows_fn<RowF32>(s->ld / 4, pairs);
    case PH_ROWS_F16: return labeled_tile_rows_fn<RowF16>(s->ld / 4, pairs);
    case PH_ROWS_I8: return labeled_tile_rows_fn<RowI8>(s->ld / 4, pairs);
    default: return nullptr;
  }
}

// (PhLabeledSet, the scratch set kept with the handle, and its acquire: list_scan.h)
static PhLabeledSet *set_acquire(phnsw_labels *lb, hipStream_t stream, bool own_stream) {
  return ph_handle_set_acquire(lb->pool, stream, own_stream);
}

// the snapshot test of a handle, written once for phnsw_labels and phnsw_attr
int ph_snapshot_fresh(const phnsw_index *ix, bool present, const phnsw_index *h_ix, uint64_t h_n, uint32_t h_nodes, const char *what,
                      const char *call) {
  if (!present) {
    ph_set_error("%s: null %s", call, what);
    return PHNSW_E_INVALID;
  }
  if (h_ix != ix || h_n != ix->store->n || h_nodes != ix->layers.back().n_nodes) {
    ph_set_error("%s: the %s are stale: made for %s (%llu vectors, %u bottom-layer nodes then; %llu and %u now); make a "
                 "new handle", call, what, h_ix != ix ? "another index" : "this index before it changed", (unsigned long long)h_n,
                 h_nodes, (unsigned long long)ix->store->n, ix->layers.back().n_nodes);
    return PHNSW_E_INVALID;
  }
  return 0;
}

// the handle test every call by label makes (ix has layers)
int ph_labels_fresh(const phnsw_index *ix, const phnsw_labels *lb, const char *call) {
  return ph_snapshot_fresh(ix, lb != nullptr, lb ? lb->ix : nullptr, lb ? lb->n : 0u, lb ? lb->n_nodes : 0u, "labels", call);
}

// index, k, handle, store: the checks every exact form makes before it looks at another argument, in this order
int ph_labeled_check(const phnsw_index *ix, const phnsw_labels *lb, uint64_t k, const char *call) {
  if (ix) PH_TRY(ph_bits_unsupported(ix->store, call));  // a bits store has the plain walk alone
  if (!ix || ix->layers.empty()) {
    ph_set_error("%s: null index or index without layers", call);
    return PHNSW_E_INVALID;
  }
  if (!ph_exact_k_valid(k)) {
    ph_set_error("%s: k must be 1..1024 (got %llu)", call, (unsigned long long)k);
    return PHNSW_E_INVALID;
  }
  PH_TRY(ph_labels_fresh(ix, lb, call));
  if (ph_store_pq_shared(ix->store)) {  // as for the distance batch, whose arithmetic the scan runs
    ph_set_error("%s: not supported over a shared-codebook PQ store; use its reconstruction store", call);
    return PHNSW_E_UNSUPPORTED;
  }
  return ph_exact_supported(ix, (uint32_t)k);  // the row length, a PQ table beside the scan's LDS
}

const uint32_t *ph_labels_column(const phnsw_labels *lb) { return lb->label_of; }

PhListView ph_labels_view(const phnsw_labels *lb) {
  phnsw_labels *m = const_cast<phnsw_labels *>(lb);
  PhListView v = {};
  v.dev.values = lb->values, v.dev.first = lb->first, v.dev.nlabels = (uint32_t)lb->nlabels, v.dev.listed = (uint32_t)lb->listed;
  v.dev.ids = lb->ids, v.longest = lb->longest, v.pool = &m->pool, v.resident = &m->resident;
  return v;
}

namespace {

// What both runs fill alike of the argument block: the store, the request, the posting lists and the grouping arrays of
// a layout over `count` positions in `pre`.
void labeled_args(const phnsw_store *s, const phnsw_labels *lb, const PhLabeledCall &c, uint32_t *pre, const PhLabelPre &lay,
                  uint64_t count, PhLabeledArgs &a) {
  a.dist = ph_dist_args(s);
  a.queries = c.queries, a.ldq = c.ldq, a.qids = c.qids, a.exclude = c.exclude;
  a.nq = (uint32_t)count, a.n = (uint32_t)s->n, a.k = c.k;
  a.values = lb->values, a.first = lb->first, a.ids = lb->ids, a.nlabels = (uint32_t)lb->nlabels;
  a.slot = pre + lay.slot, a.iota = pre + lay.iota, a.sslot = pre + lay.sslot, a.order = pre + lay.order;
  a.flags = pre + lay.flags, a.tidx = pre + lay.tidx, a.tile_first = pre + lay.tile_first, a.head = pre + lay.head;
  a.out_ids = c.out_ids, a.out_d = c.out_d, a.out_len = c.out_len, a.status = c.status;
}

// the kernel of a call with its dynamic LDS, and what the sort and the tile scan write: the layout's arrays as outputs
// (the argument block holds them as the kernels' inputs)
struct PhLabeledLaunch {
  PhLabeledFn fn;
  size_t lds;
  uint32_t *sslot, *sorted_values, *tidx;  // sorted_values: the queries of labeled_run, the pairs of labelset_run
};

// Before anything is enqueued: T and the kernel of a call -- the tile kernel for T > 1 on a row store, else the per-query
// scan; pairs: the PAIRS instances of phnsw_search_exact_labelset --, its dynamic LDS, the slice count from the waves of
// it the device holds, and hipCUB's temporaries, which depend on the position count alone.  Fills a.T, a.pq_lds, a.slices.
int labeled_plan(const phnsw_labels *lb, const phnsw_store *s, PhLabeledSet &set, bool pairs, hipStream_t stream,
                 PhLabeledArgs &a, PhLabeledLaunch *ln) {
  const size_t pq_lds = (ph_pq_lds_bytes(s) + 15u) & ~(size_t)15u;
  ln->fn = labeled_scan_fn(s, pairs), ln->lds = pq_lds + (size_t)ph_label_scan_lds(a.k);
  a.T = 1u, a.pq_lds = (uint32_t)pq_lds;
  if (PhLabeledFn tile = labeled_tile_fn(s, pairs)) {
    const uint32_t T = ph_label_tile(a.k, s->ld, PH_LABEL_LDS_BYTES, env_ll("PHNSW_LABEL_TILE"));
    if (T > 1u && ph_label_tile_lds(T, a.k, s->ld) <= PH_LABEL_LDS_BYTES) {
      ln->fn = tile, a.T = T, ln->lds = (size_t)ph_label_tile_lds(T, a.k, s->ld);
    }
  }
  phnsw_labels *mlb = const_cast<phnsw_labels *>(lb);
  uint64_t resident = 0;
  PH_TRY(ph_resident_waves(mlb->resident, mlb->pool.mutex, s->device, (const void *)ln->fn, ln->lds, &resident));
  // work items the host can count on: the positions, or at least ceil(positions / T) tiles
  const uint64_t count = a.nq;
  a.slices = ph_label_slice_count((count + a.T - 1u) / a.T, resident, lb->longest, env_ll("PHNSW_LABEL_SLICES"));
  if (set.tmp_nq != count) {
    size_t sort_bytes = 0, scan_bytes = 0;
    PH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, a.slot, ln->sslot, a.iota, ln->sorted_values, (int)count, 0, 32,
                                              stream));
    PH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, a.flags, ln->tidx, (int)(count + 1u), stream));
    set.tmp_need = std::max<size_t>(std::max(sort_bytes, scan_bytes), 16), set.tmp_nq = count;
  }
  return set.block_ensure(&set.tmp, &set.tmp_bytes, set.tmp_need, stream);
}

// (slot, value) of the lookup positions sorted by slot: sslot and sorted_values
int labeled_sort(PhLabeledSet &set, const PhLabeledArgs &a, const PhLabeledLaunch &ln, hipStream_t stream) {
  size_t bytes = set.tmp_bytes;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(set.tmp, bytes, a.slot, ln.sslot, a.iota, ln.sorted_values, (int)a.nq, 0, 32, stream));
  return 0;
}

// After the lookup and the sort: the tile table for T > 1, then the scan or tile kernel over (positions, slices).
int labeled_scan(PhLabeledSet &set, const PhLabeledArgs &a, const PhLabeledLaunch &ln, hipStream_t stream) {
  const uint64_t count = a.nq;
  if (a.T > 1u) {
    hipLaunchKernelGGL(ph_labeled_tileflag_kernel, dim3(grid1(count + 1u)), dim3(256), 0, stream, a);
    PH_HIP(hipGetLastError());
    size_t bytes = set.tmp_bytes;
    PH_HIP(hipcub::DeviceScan::ExclusiveSum(set.tmp, bytes, a.flags, ln.tidx, (int)(count + 1u), stream));
    hipLaunchKernelGGL(ph_labeled_tiles_kernel, dim3(grid1(count + 1u)), dim3(256), 0, stream, a);
    PH_HIP(hipGetLastError());
  }
  const uint64_t items = count * (uint64_t)a.slices;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(items, 1u << 20);  // the kernels stride over what is left
  hipLaunchKernelGGL(ln.fn, dim3(grid), dim3(64), ln.lds, stream, a);
  PH_HIP(hipGetLastError());
  return 0;
}

// the orchestration on a set the caller holds; c is checked, 0 < nq <= PH_LABEL_NQ_MAX (with a list: its length).
// Enqueues and returns.
int labeled_run(const phnsw_index *ix, const phnsw_labels *lb, const PhLabeledCall &c, PhLabeledSet &set) {
  const phnsw_store *s = ix->store;
  const uint64_t nq = c.nq;
  const PhLabelPre lay = ph_label_pre(nq);
  PH_TRY(set.ready());
  PH_TRY(set.block_ensure(&set.pre, &set.pre_bytes, (size_t)lay.words * 4u, c.stream));
  uint32_t *const pre = (uint32_t *)set.pre;
  PhLabeledArgs a = {};
  labeled_args(s, lb, c, pre, lay, nq, a);
  a.want = c.want, a.list = c.list;
  PhLabeledLaunch ln = {nullptr, 0, pre + lay.sslot, pre + lay.order, pre + lay.tidx};
  PH_TRY(labeled_plan(lb, s, set, false, c.stream, a, &ln));
  if (a.slices > 1u) {
    uint64_t bytes = 0;
    if (!ph_label_key_bytes(nq, a.slices, c.k, &bytes)) {
      ph_set_error("exact labeled search: %llu queries in %u slices at k = %u need more scratch than can be addressed",
                   (unsigned long long)nq, a.slices, c.k);
      return PHNSW_E_INVALID;
    }
    PH_TRY(set.block_ensure(&set.keys, &set.keys_bytes, (size_t)bytes, c.stream));
    a.scratch = (uint64_t *)set.keys;
  }

  hipLaunchKernelGGL(ph_labeled_lookup_kernel, dim3(grid1(nq)), dim3(256), 0, c.stream, a);
  PH_HIP(hipGetLastError());
  PH_TRY(labeled_sort(set, a, ln, c.stream));
  PH_TRY(labeled_scan(set, a, ln, c.stream));
  if (a.slices > 1u) {
    hipLaunchKernelGGL(ph_list_merge_kernel<PhLabeledArgs>, dim3((uint32_t)std::min<uint64_t>(nq, 1u << 20)), dim3(64),
                       (size_t)ph_label_scan_lds(c.k), c.stream, a);
    PH_HIP(hipGetLastError());
  }
  return 0;
}

// labeled_run over pairs (labelset_plan.h; the request: PhLabelsetCall, phnsw_internal.h); c is checked, 0 < batch_nq,
// batch_nq and nwant <= PH_LABEL_NQ_MAX; with c.list, c.nq > 0 is its length.  Enqueues and returns.
int labelset_run(const phnsw_index *ix, const phnsw_labels *lb, const PhLabelsetCall &sc, PhLabeledSet &set) {
  const phnsw_store *s = ix->store;
  const PhLabeledCall &c = sc.c;
  const uint64_t nq = sc.batch_nq, np = sc.nwant;  // np positions
  const PhLabelsetPre lay = ph_labelset_pre(np);
  PH_TRY(set.ready());
  // (the subset form's marks [nq] behind the layout's words)
  PH_TRY(set.block_ensure(&set.pre, &set.pre_bytes, (size_t)(lay.words + (c.list ? nq : 0u)) * 4u, c.stream));
  uint32_t *const pre = (uint32_t *)set.pre;
  PhLabelsetArgs sa = {};
  PhLabeledArgs &a = sa.a;
  labeled_args(s, lb, c, pre, lay.pos, np, a);
  a.slices = 1u, a.T = 1u;
  sa.want_first = sc.want_first, sa.want_values = sc.want_values, sa.nq = (uint32_t)nq, sa.nwant = (uint32_t)np;
  sa.owner = pre + lay.owner, sa.spair = pre + lay.spair, sa.inv = pre + lay.inv, sa.dup = pre + lay.dup;
  a.list = c.list, sa.nlist = (uint32_t)(c.list ? c.nq : nq);

  if (np) {
    PhLabeledLaunch ln = {nullptr, 0, pre + lay.pos.sslot, sa.spair, pre + lay.pos.tidx};
    PH_TRY(labeled_plan(lb, s, set, true, c.stream, a, &ln));
    uint64_t bytes = 0;
    if (!ph_labelset_key_bytes(np, a.slices, c.k, &bytes)) {
      ph_set_error("exact labelset search: %llu wanted labels in %u slices at k = %u need more scratch than can be addressed",
                   (unsigned long long)np, a.slices, c.k);
      return PHNSW_E_INVALID;
    }
    PH_TRY(set.block_ensure(&set.keys, &set.keys_bytes, (size_t)bytes, c.stream));
    a.scratch = (uint64_t *)set.keys;

    PH_HIP(hipMemsetAsync(sa.owner, 0xFF, (size_t)np * 4u, c.stream));  // PH_LABELSET_OWNER_NONE
    hipLaunchKernelGGL(ph_labelset_claim_kernel, dim3(grid1(nq)), dim3(256), 0, c.stream, sa.want_first, sa.nq, sa.nwant, sa.owner);
    PH_HIP(hipGetLastError());
    if (c.list) {
      uint32_t *const sel = pre + lay.words;
      PH_HIP(hipMemsetAsync(sel, 0, (size_t)nq * 4u, c.stream));
      hipLaunchKernelGGL(ph_labelset_select_kernel, dim3(grid1(sa.nlist)), dim3(256), 0, c.stream, c.list, sa.nlist, (uint32_t)nq, sel);
      PH_HIP(hipGetLastError());
      sa.sel = sel;
    }
    hipLaunchKernelGGL(ph_labelset_lookup_kernel, dim3(grid1(np)), dim3(256), 0, c.stream, sa);
    PH_HIP(hipGetLastError());
    PH_TRY(labeled_sort(set, a, ln, c.stream));
    hipLaunchKernelGGL(ph_labelset_positions_kernel, dim3(grid1(np)), dim3(256), 0, c.stream, sa, pre + lay.pos.order);
    PH_HIP(hipGetLastError());
    PH_TRY(labeled_scan(set, a, ln, c.stream));
  }
  // no pair at all: every sound range is empty, and the merge alone writes the rows
  hipLaunchKernelGGL(ph_labelset_merge_kernel, dim3((uint32_t)std::min<uint64_t>(sa.nlist, 1u << 20)), dim3(64),
                     (size_t)ph_label_scan_lds(c.k), c.stream, sa);
  PH_HIP(hipGetLastError());
  return 0;
}

void labels_free(phnsw_labels *lb) {
  ph_handle_sets_free(lb->pool);
  if (lb->values) hipFree(lb->values);
  if (lb->first) hipFree(lb->first);
  if (lb->ids) hipFree(lb->ids);
  if (lb->label_of) hipFree(lb->label_of);
  delete lb;
}

// the lists of labels_dev [n] on `stream`; synchronises it
int labels_build(const phnsw_index *ix, const uint32_t *labels_dev, uint64_t n, hipStream_t stream, const char *call,
                 phnsw_labels **out) {
  const phnsw_store *s = ix->store;
  phnsw_labels *lb = new phnsw_labels();
  lb->ix = ix, lb->n = n, lb->n_nodes = ix->layers.back().n_nodes, lb->device = s->device;
  struct Drop {
    phnsw_labels *lb;
    ~Drop() {
      if (lb) labels_free(lb);
    }
  } drop{lb};
  if (n == 0) {
    PH_HIP(hipMalloc(&lb->first, 4));
    PH_HIP(hipMemsetAsync(lb->first, 0, 4, stream));
    PH_HIP(hipMalloc(&lb->label_of, 4));  // never null: a null column would read as "no label filter"
    PH_HIP(hipMemsetAsync(lb->label_of, 0xFF, 4, stream));
    PH_HIP(hipStreamSynchronize(stream));
    *out = lb, drop.lb = nullptr;
    return 0;
  }
  uint32_t n_nodes;
  const uint32_t *nodes, *vec2node;
  ph_exact_bottom_layer(ix, &n_nodes, &nodes, &vec2node);
  HostBlocks hb{stream, {}};
  uint32_t *skeys = nullptr, *iota = nullptr, *flags = nullptr, *slots = nullptr, *head = nullptr;
  void *tmp = nullptr;
  PH_HIP(hipMalloc(&lb->label_of, (size_t)n * 4u));  // the sort's keys, which it leaves as they are: kept
  uint32_t *const keys = lb->label_of;
  PH_TRY(hb.alloc(&skeys, (size_t)n * 4u));
  PH_TRY(hb.alloc(&iota, (size_t)n * 4u));
  PH_TRY(hb.alloc(&flags, (size_t)(n + 1u) * 4u));
  PH_TRY(hb.alloc(&slots, (size_t)(n + 1u) * 4u));
  PH_TRY(hb.alloc(&head, 16));
  PH_HIP(hipMalloc(&lb->ids, (size_t)n * 4u));
  size_t sort_bytes = 0, scan_bytes = 0;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys, skeys, iota, lb->ids, (int)n, 0, 32, stream));
  PH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, flags, slots, (int)(n + 1u), stream));
  size_t tmp_bytes = std::max<size_t>(std::max(sort_bytes, scan_bytes), 16);
  PH_TRY(hb.alloc(&tmp, tmp_bytes));
  hipLaunchKernelGGL(ph_label_key_kernel, dim3(grid1(n)), dim3(256), 0, stream, labels_dev, (uint32_t)n, n_nodes, nodes, vec2node,
                     keys, iota);
  PH_HIP(hipGetLastError());
  size_t bytes = tmp_bytes;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys, skeys, iota, lb->ids, (int)n, 0, 32, stream));
  hipLaunchKernelGGL(ph_label_flags_kernel, dim3(grid1(n + 1u)), dim3(256), 0, stream, skeys, (uint32_t)n, flags, head);
  PH_HIP(hipGetLastError());
  bytes = tmp_bytes;
  PH_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, flags, slots, (int)(n + 1u), stream));
  uint32_t h[2] = {0, 0};
  PH_HIP(hipMemcpyAsync(&h[0], slots + n, 4, hipMemcpyDeviceToHost, stream));
  PH_HIP(hipMemcpyAsync(&h[1], head + 1, 4, hipMemcpyDeviceToHost, stream));
  PH_HIP(hipStreamSynchronize(stream));
  lb->nlabels = h[0], lb->listed = h[1];
  if (lb->listed > n || lb->nlabels > lb->listed) {
    ph_set_error("%s: the labels changed while the lists were made", call);
    return PHNSW_E_INVALID;
  }
  PH_HIP(hipMalloc(&lb->values, std::max<size_t>((size_t)lb->nlabels * 4u, 4)));
  PH_HIP(hipMalloc(&lb->first, (size_t)(lb->nlabels + 1u) * 4u));
  hipLaunchKernelGGL(ph_label_heads_kernel, dim3(grid1(n + 1u)), dim3(256), 0, stream, skeys, flags, slots, (uint32_t)n,
                     (uint32_t)lb->nlabels, (uint32_t)lb->listed, lb->values, lb->first);
  PH_HIP(hipGetLastError());
  std::vector<uint32_t> hfirst(lb->nlabels + 1u);
  PH_HIP(hipMemcpyAsync(hfirst.data(), lb->first, hfirst.size() * 4u, hipMemcpyDeviceToHost, stream));
  PH_HIP(hipStreamSynchronize(stream));
  for (uint64_t i = 0; i < lb->nlabels; i++) {
    if (hfirst[i + 1u] <= hfirst[i] || hfirst[i + 1u] > lb->listed) {
      ph_set_error("%s: the labels changed while the lists were made", call);
      return PHNSW_E_INVALID;
    }
    lb->longest = std::max<uint64_t>(lb->longest, hfirst[i + 1u] - hfirst[i]);
  }
  *out = lb, drop.lb = nullptr;
  return 0;
}

int labels_create_check(const phnsw_index *ix, const void *labels, uint64_t n, phnsw_labels **out, const char *call) {
  if (!ix || ix->layers.empty()) {
    ph_set_error("%s: null index or index without layers", call);
    return PHNSW_E_INVALID;
  }
  if (!out || (!labels && n)) {
    ph_set_error("%s: null labels or null output", call);
    return PHNSW_E_INVALID;
  }
  if (n != ix->store->n) {
    ph_set_error("%s: %llu labels for a store of %llu vectors (one label per vector)", call, (unsigned long long)n,
                 (unsigned long long)ix->store->n);
    return PHNSW_E_INVALID;
  }
  return 0;
}

}  // namespace

int ph_labels_count(const phnsw_labels *lb, const uint32_t *want_dev, uint64_t nq, uint32_t *out_count_dev, hipStream_t stream) {
  hipLaunchKernelGGL(ph_labeled_count_kernel, dim3(grid1(nq)), dim3(256), 0, stream, lb->values, lb->first, (uint32_t)lb->nlabels,
                     want_dev, nq, out_count_dev);
  PH_HIP(hipGetLastError());
  return 0;
}

int ph_labeled_device(const phnsw_index *ix, const phnsw_labels *lb, const PhLabeledCall &c) {
  if (c.nq == 0) return 0;
  phnsw_labels *mlb = const_cast<phnsw_labels *>(lb);
  PhLabeledSet *set = set_acquire(mlb, c.stream, false);
  PhSetGuard guard{mlb->pool, set, c.stream};
  return labeled_run(ix, lb, c, *set);
}

int ph_labelset_device(const phnsw_index *ix, const phnsw_labels *lb, const PhLabelsetCall &sc) {
  if (sc.c.nq == 0 || sc.batch_nq == 0) return 0;
  phnsw_labels *mlb = const_cast<phnsw_labels *>(lb);
  PhLabeledSet *set = set_acquire(mlb, sc.c.stream, false);
  PhSetGuard guard{mlb->pool, set, sc.c.stream};
  return labelset_run(ix, lb, sc, *set);
}

int ph_labels_count_set(const phnsw_labels *lb, const uint32_t *want_first_dev, const uint32_t *want_values_dev, uint64_t nq,
                        uint64_t nwant, uint32_t *out_count_dev, uint32_t *owner_scratch, hipStream_t stream) {
  hipLaunchKernelGGL(ph_labelset_count_kernel, dim3((uint32_t)std::min<uint64_t>(nq, 1u << 20)), dim3(64), 0, stream, lb->values,
                     lb->first, (uint32_t)lb->nlabels, want_first_dev, want_values_dev, nq, (uint32_t)nwant, out_count_dev);
  PH_HIP(hipGetLastError());
  if (!owner_scratch || !nwant) return 0;  // without a pair no range overlaps another, and a bad range counts 0 already
  PhLabelsetArgs sa = {};
  sa.want_first = want_first_dev, sa.want_values = want_values_dev, sa.nq = (uint32_t)nq, sa.nwant = (uint32_t)nwant;
  sa.owner = owner_scratch;
  PH_HIP(hipMemsetAsync(sa.owner, 0xFF, (size_t)nwant * 4u, stream));  // PH_LABELSET_OWNER_NONE
  hipLaunchKernelGGL(ph_labelset_claim_kernel, dim3(grid1(nq)), dim3(256), 0, stream, sa.want_first, sa.nq, sa.nwant, sa.owner);
  PH_HIP(hipGetLastError());
  hipLaunchKernelGGL(ph_labelset_refused_kernel, dim3((uint32_t)std::min<uint64_t>(nq, 1u << 20)), dim3(64), 0, stream, sa,
                     out_count_dev);
  PH_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ C ABI

extern "C" int phnsw_labels_create_device(const phnsw_index *ix, const uint32_t *labels_dev, uint64_t n, void *stream,
                                          phnsw_labels **out) try {
  const char *const call = "phnsw_labels_create_device";
  PH_TRY(labels_create_check(ix, labels_dev, n, out, call));
  PH_HIP(hipSetDevice(ix->store->device));
  return labels_build(ix, labels_dev, n, (hipStream_t)stream, call, out);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_labels_create(const phnsw_index *ix, const uint32_t *labels, uint64_t n, phnsw_labels **out) try {
  const char *const call = "phnsw_labels_create";
  PH_TRY(labels_create_check(ix, labels, n, out, call));
  PH_HIP(hipSetDevice(ix->store->device));
  HostBlocks hb{nullptr, {}};
  uint32_t *dev = nullptr;
  PH_TRY(hb.alloc(&dev, (size_t)n * 4u));
  if (n) PH_HIP(hipMemcpy(dev, labels, (size_t)n * 4u, hipMemcpyHostToDevice));
  return labels_build(ix, dev, n, nullptr, call, out);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_labels_info(const phnsw_labels *lb, uint64_t *n, uint64_t *nlabels, uint64_t *listed, uint64_t *longest) try {
  if (!lb) {
    ph_set_error("phnsw_labels_info: null labels");
    return PHNSW_E_INVALID;
  }
  if (n) *n = lb->n;
  if (nlabels) *nlabels = lb->nlabels;
  if (listed) *listed = lb->listed;
  if (longest) *longest = lb->longest;
  return 0;
} catch (...) { return ph_caught(); }

extern "C" int phnsw_labels_count_device(const phnsw_labels *lb, const uint32_t *want_dev, uint64_t nq, uint32_t *out_count_dev,
                                         void *stream) try {
  const char *const call = "phnsw_labels_count_device";
  if (!lb) {
    ph_set_error("%s: null labels", call);
    return PHNSW_E_INVALID;
  }
  if (nq == 0) return 0;
  if (!want_dev || !out_count_dev) {
    ph_set_error("%s: null want or null output", call);
    return PHNSW_E_INVALID;
  }
  PH_HIP(hipSetDevice(lb->device));
  return ph_labels_count(lb, want_dev, nq, out_count_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" void phnsw_labels_destroy(phnsw_labels *lb) {
  if (!lb) return;
  try {
    hipSetDevice(lb->device);
    labels_free(lb);  // waits for the events that close the calls in flight
  } catch (...) {
  }
}

extern "C" int phnsw_search_exact_labeled_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev,
                                                 uint32_t ldq, const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                                 const uint32_t *want_dev, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                                 uint32_t *out_len_dev, uint32_t *status_dev, void *stream) try {
  const char *const call = "phnsw_search_exact_labeled_device";
  PH_TRY(ph_labeled_check(ix, lb, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !want_dev || nq > PH_LABEL_NQ_MAX) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; want; nq < 2^31 - 1; queries need ldq >= store "
                 "ld, multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhLabeledCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.want = want_dev, c.nq = nq;
  c.k = (uint32_t)k;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_labeled_device(ix, lb, c);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_labeled(const phnsw_index *ix, const phnsw_labels *lb, const float *queries, const uint64_t *qids,
                                          uint64_t nq, const uint64_t *exclude, const uint32_t *want, uint64_t k,
                                          uint64_t *out_ids, float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_search_exact_labeled";
  PH_TRY(ph_labeled_check(ix, lb, k, call));
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!out_ids || !out_d || !out_len || !want || nq > PH_LABEL_NQ_MAX) {
    ph_set_error("%s: invalid argument (outputs; want; nq < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, call));
  phnsw_labels *mlb = const_cast<phnsw_labels *>(lb);
  PhLabeledSet *set = set_acquire(mlb, nullptr, true);
  PhHostCall h(mlb->pool, set);
  PH_TRY(h.stage_in(s, queries, qids, exclude, nq, (size_t)nq, 0, (uint32_t)k, (uint32_t)k));  // extras: want
  PhLabeledCall c = {};
  h.fill(c);
  PH_HIP(hipMemcpyAsync(h.extra(), want, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
  c.want = h.extra(), c.k = (uint32_t)k;
  PH_TRY(labeled_run(ix, lb, c, *set));
  return h.finish(out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }

// ------------------------------------------------------------------ C ABI: a set of labels per query

extern "C" int phnsw_labels_count_set_device(const phnsw_labels *lb, const uint32_t *want_first_dev,
                                             const uint32_t *want_values_dev, uint64_t nq, uint64_t nwant,
                                             uint32_t *out_count_dev, void *stream) try {
  const char *const call = "phnsw_labels_count_set_device";
  if (!lb) {
    ph_set_error("%s: null labels", call);
    return PHNSW_E_INVALID;
  }
  if (nq == 0) return 0;
  if (!want_first_dev || !out_count_dev || (!want_values_dev && nwant)) {
    ph_set_error("%s: null want_first, null want_values with nwant > 0, or null output", call);
    return PHNSW_E_INVALID;
  }
  if (nq > PH_LABEL_NQ_MAX || nwant > PH_LABELSET_NWANT_MAX) {
    ph_set_error("%s: nq and nwant must be below 2^31 - 1", call);
    return PHNSW_E_INVALID;
  }
  PH_HIP(hipSetDevice(lb->device));
  return ph_labels_count_set(lb, want_first_dev, want_values_dev, nq, nwant, out_count_dev, nullptr, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_labelset_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev,
                                                  uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                  const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                                  const uint32_t *want_values_dev, uint64_t nwant, uint64_t k,
                                                  uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                  uint32_t *status_dev, void *stream) try {
  const char *const call = "phnsw_search_exact_labelset_device";
  PH_TRY(ph_labeled_check(ix, lb, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !want_first_dev || (!want_values_dev && nwant)) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; want_first; want_values unless nwant is 0; "
                 "queries need ldq >= store ld, multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  if (nq > PH_LABEL_NQ_MAX || nwant > PH_LABELSET_NWANT_MAX) {
    ph_set_error("%s: nq and nwant must be below 2^31 - 1", call);
    return PHNSW_E_INVALID;
  }
  PhLabelsetCall sc = {};
  PhLabeledCall &c = sc.c;
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq, c.k = (uint32_t)k;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  sc.want_first = want_first_dev, sc.want_values = want_values_dev, sc.nwant = nwant, sc.batch_nq = nq;
  PH_HIP(hipSetDevice(ix->store->device));
  phnsw_labels *mlb = const_cast<phnsw_labels *>(lb);
  PhLabeledSet *set = set_acquire(mlb, c.stream, false);
  PhSetGuard guard{mlb->pool, set, c.stream};
  return labelset_run(ix, lb, sc, *set);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_labelset(const phnsw_index *ix, const phnsw_labels *lb, const float *queries,
                                           const uint64_t *qids, uint64_t nq, const uint64_t *exclude,
                                           const uint32_t *want_first, const uint32_t *want_values, uint64_t k,
                                           uint64_t *out_ids, float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_search_exact_labelset";
  PH_TRY(ph_labeled_check(ix, lb, k, call));
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!out_ids || !out_d || !out_len || !want_first || nq > PH_LABEL_NQ_MAX) {
    ph_set_error("%s: invalid argument (outputs; want_first; nq < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  const uint64_t nwant = want_first[nq];
  if ((!want_values && nwant) || nwant > PH_LABELSET_NWANT_MAX) {
    ph_set_error("%s: invalid argument (want_values unless want_first[nq] is 0; want_first[nq] < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, call, true));
  if (const uint64_t bad = ph_labelset_first_bad(want_first, nq); bad < nq) {
    ph_set_error("%s: query %llu: want_first must start at 0 and never run backwards (want_first[%llu] = %u, want_first[%llu] "
                 "= %u)", call, (unsigned long long)bad, (unsigned long long)bad, want_first[bad], (unsigned long long)bad + 1u,
                 want_first[bad + 1u]);
    return PHNSW_E_INVALID;
  }
  phnsw_labels *mlb = const_cast<phnsw_labels *>(lb);
  PhLabeledSet *set = set_acquire(mlb, nullptr, true);
  PhHostCall h(mlb->pool, set);
  // extras: want_first [nq + 1] | want_values [nwant]
  PH_TRY(h.stage_in(s, queries, qids, exclude, nq, (size_t)nq + 1u + (size_t)nwant, 0, (uint32_t)k, (uint32_t)k));
  PhLabelsetCall sc = {};
  h.fill(sc.c);
  uint32_t *const first_dev = h.extra(), *const values_dev = first_dev + nq + 1u;
  PH_HIP(hipMemcpyAsync(first_dev, want_first, (size_t)(nq + 1u) * 4u, hipMemcpyHostToDevice, h.st));
  if (nwant) PH_HIP(hipMemcpyAsync(values_dev, want_values, (size_t)nwant * 4u, hipMemcpyHostToDevice, h.st));
  sc.want_first = first_dev, sc.want_values = values_dev, sc.nwant = nwant, sc.batch_nq = nq;
  sc.c.k = (uint32_t)k;
  PH_TRY(labelset_run(ix, lb, sc, *set));
  return h.finish(out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }

// ------------------------------------------------------------------ the graph walk by label

namespace {

// what both forms of the walk check before they look at a pointer: index and parameters, the handle, the flags
int walk_check(const phnsw_index *ix, const phnsw_labels *lb, const phnsw_search_params *sp, uint32_t flags, const char *call) {
  if (ix) PH_TRY(ph_bits_unsupported(ix->store, call));  // a bits store has the plain walk alone
  PH_TRY(ph_check_sp(ix, sp));
  PH_TRY(ph_labels_fresh(ix, lb, call));
  if (flags & ~(uint32_t)PHNSW_FILTER_STRICT) {
    ph_set_error("%s: unknown flag bits 0x%x", call, flags);
    return PHNSW_E_INVALID;
  }
  return 0;
}

}  // namespace

// The run of the host walks (by label, by set, by range: list_scan.h) once everything is staged: the launch, the words back, and the queries
// whose frontier spill overflowed (status 5) again from a device list with 8x the room, as ph_search_host re-runs them;
// then the rows and the stats (the first two extra words of `small`).  redo_dev: nq words of the staging.
int ph_walk_host_run(const phnsw_index *ix, PhHostCall &h, PhSearchCall &c, uint32_t *redo_dev, uint32_t ef, uint64_t *out_ids,
                  float *out_d, uint64_t *out_len, uint64_t *out_stats) {
  const uint64_t nq = h.nq;
  std::vector<uint32_t> &redo = h.h_list;  // read by a copy: kept by h, changed only behind the next sync
  uint32_t ovf_cap = ph_default_ovf_cap(ef);
  for (int attempt = 0;; attempt++) {
    PH_TRY(ph_search_device(ix, c));
    PH_TRY(h.download_words());
    PH_TRY(h.sync());
    redo.clear();
    for (uint64_t i = 0; i < nq; i++) {
      if (h.status(i) == 4u) {
        ph_set_error("search: a candidate vector is missing from a lower layer (layers not nested, lib.rs:261)");
        return PHNSW_E_MISSING_NODE;
      }
      if (h.status(i) == 5u) redo.push_back((uint32_t)i);
    }
    if (redo.empty()) break;
    if (attempt == 3) {
      ph_set_error("search: frontier spill exceeded %u entries for %zu queries", ovf_cap, redo.size());
      return PHNSW_E_OVERFLOW;
    }
    // the overflowed queries alone, from a device list, with 8x the room: everything stays addressed by the query index
    ovf_cap *= 8;
    PH_TRY(h.upload_list(redo_dev));
    c.order = redo_dev, c.nq = redo.size(), c.ovf_cap = ovf_cap;
  }
  PH_TRY(h.finish(out_ids, out_d, out_len));
  if (out_stats)
    for (uint64_t i = 0; i < 2u * nq; i++) out_stats[i] = h.read_extra(0, i);
  return 0;
}

extern "C" int phnsw_search_batch_labeled_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev,
                                                 uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                 const phnsw_search_params *sp, uint32_t upto_layers, const uint32_t *exclude_dev,
                                                 const uint32_t *want_dev, uint32_t flags, uint32_t *out_ids_dev, float *out_d_dev,
                                                 uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev,
                                                 void *stream) try {
  const char *const call = "phnsw_search_batch_labeled_device";
  PH_TRY(walk_check(ix, lb, sp, flags, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !want_dev || nq > 0xFFFFFFFFull) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; want; queries need ldq >= store ld, multiple of "
                 "4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhSearchCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq;
  c.sp = sp, c.upto = upto_layers;
  c.filter.label_of = lb->label_of, c.filter.want = want_dev, c.filter.flags = flags;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.status = status_dev, c.out_stats = out_stats_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_search_device(ix, c);
} catch (...) { return ph_caught(); }

// The host form stages everything once, on the stream of a scratch set of the handle: query rows, the id words, want.
// Queries whose frontier spill overflowed (status 5) are re-run from a device list with 8x the room, as ph_search_host
// re-runs them.
extern "C" int phnsw_search_batch_labeled(const phnsw_index *ix, const phnsw_labels *lb, const float *queries,
                                          const uint64_t *qids, uint64_t nq, const phnsw_search_params *sp, uint32_t upto_layers,
                                          const uint64_t *exclude, const uint32_t *want, uint32_t flags, uint64_t k,
                                          uint64_t *out_ids, float *out_d, uint64_t *out_len, uint64_t *out_stats) try {
  const char *const call = "phnsw_search_batch_labeled";
  PH_TRY(walk_check(ix, lb, sp, flags, call));
  const uint32_t ef = (uint32_t)sp->number_of_candidates;
  if (k > ef) {
    ph_set_error("%s: k must be 0 (the whole queue) or 1..number_of_candidates (got %llu, number_of_candidates %u)", call,
                 (unsigned long long)k, ef);
    return PHNSW_E_INVALID;
  }
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!out_ids || !out_d || !out_len || !want || nq > 0xFFFFFFFFull) {
    ph_set_error("%s: invalid argument (outputs; want; nq < 2^32)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, call));
  phnsw_labels *mlb = const_cast<phnsw_labels *>(lb);
  PhLabeledSet *set = set_acquire(mlb, nullptr, true);
  PhHostCall h(mlb->pool, set);
  // extras: stats(2), which the host reads back with len and status | want | the redo list
  PH_TRY(h.stage_in(s, queries, qids, exclude, nq, (size_t)nq * 4u, 2, ef, k ? (uint32_t)k : ef));
  uint32_t *const want_dev = h.extra() + 2u * nq, *const redo_dev = want_dev + nq;
  PhSearchCall c = {};
  h.fill(c);
  PH_HIP(hipMemcpyAsync(want_dev, want, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
  c.filter.label_of = lb->label_of, c.filter.want = want_dev, c.filter.flags = flags;
  c.sp = sp, c.upto = upto_layers, c.out_stats = h.extra();
  return ph_walk_host_run(ix, h, c, redo_dev, ef, out_ids, out_d, out_len, out_stats);
} catch (...) { return ph_caught(); }

// ------------------------------------------------------------------ the graph walk by a set of labels

// The search kernels' set mode (search_labelset.hip) over label_of and the caller's table.  The device form hands the
// table to the kernels as it is: they refuse a range that is not sound per query (status 8) and read nothing outside
// want_values[0 .. nwant); ranges that OVERLAP are harmless to a walk -- every query reads its own range -- and are not
// detected here (the exact scan and the routed call do detect them).
extern "C" int phnsw_search_batch_labelset_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev,
                                                  uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                  const phnsw_search_params *sp, uint32_t upto_layers,
                                                  const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                                  const uint32_t *want_values_dev, uint64_t nwant, uint32_t flags,
                                                  uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                  uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) try {
  const char *const call = "phnsw_search_batch_labelset_device";
  PH_TRY(walk_check(ix, lb, sp, flags, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !want_first_dev || (!want_values_dev && nwant)) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; want_first; want_values unless nwant is 0; "
                 "queries need ldq >= store ld, multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  if (nq > PH_LABEL_NQ_MAX || nwant > PH_LABELSET_NWANT_MAX) {
    ph_set_error("%s: nq and nwant must be below 2^31 - 1", call);
    return PHNSW_E_INVALID;
  }
  PhSearchCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq;
  c.sp = sp, c.upto = upto_layers;
  c.filter.label_of = lb->label_of, c.filter.flags = flags;
  c.filter.set_first = want_first_dev, c.filter.set_values = want_values_dev, c.filter.set_nwant = (uint32_t)nwant;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.status = status_dev, c.out_stats = out_stats_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_search_device(ix, c);
} catch (...) { return ph_caught(); }

// The host form stages everything once, as phnsw_search_batch_labeled does: query rows, the id words, and the filter's
// 4 * (nq + 1) + 4 * nwant bytes.  The offsets are checked here, so no query can come back with status 8.
extern "C" int phnsw_search_batch_labelset(const phnsw_index *ix, const phnsw_labels *lb, const float *queries,
                                           const uint64_t *qids, uint64_t nq, const phnsw_search_params *sp, uint32_t upto_layers,
                                           const uint64_t *exclude, const uint32_t *want_first, const uint32_t *want_values,
                                           uint32_t flags, uint64_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len,
                                           uint64_t *out_stats) try {
  const char *const call = "phnsw_search_batch_labelset";
  PH_TRY(walk_check(ix, lb, sp, flags, call));
  const uint32_t ef = (uint32_t)sp->number_of_candidates;
  if (k > ef) {
    ph_set_error("%s: k must be 0 (the whole queue) or 1..number_of_candidates (got %llu, number_of_candidates %u)", call,
                 (unsigned long long)k, ef);
    return PHNSW_E_INVALID;
  }
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!out_ids || !out_d || !out_len || !want_first || nq > PH_LABEL_NQ_MAX) {
    ph_set_error("%s: invalid argument (outputs; want_first; nq < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  const uint64_t nwant = want_first[nq];
  if ((!want_values && nwant) || nwant > PH_LABELSET_NWANT_MAX) {
    ph_set_error("%s: invalid argument (want_values unless want_first[nq] is 0; want_first[nq] < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, call, true));
  if (const uint64_t bad = ph_labelset_first_bad(want_first, nq); bad < nq) {
    ph_set_error("%s: query %llu: want_first must start at 0 and never run backwards (want_first[%llu] = %u, want_first[%llu] "
                 "= %u)", call, (unsigned long long)bad, (unsigned long long)bad, want_first[bad], (unsigned long long)bad + 1u,
                 want_first[bad + 1u]);
    return PHNSW_E_INVALID;
  }
  phnsw_labels *mlb = const_cast<phnsw_labels *>(lb);
  PhLabeledSet *set = set_acquire(mlb, nullptr, true);
  PhHostCall h(mlb->pool, set);
  // extras: stats(2), which the host reads back with len and status | want_first [nq + 1] | want_values [nwant] | the redo list
  PH_TRY(h.stage_in(s, queries, qids, exclude, nq, (size_t)nq * 4u + 1u + (size_t)nwant, 2, ef, k ? (uint32_t)k : ef));
  uint32_t *const first_dev = h.extra() + 2u * nq, *const values_dev = first_dev + nq + 1u, *const redo_dev = values_dev + nwant;
  PhSearchCall c = {};
  h.fill(c);
  PH_HIP(hipMemcpyAsync(first_dev, want_first, (size_t)(nq + 1u) * 4u, hipMemcpyHostToDevice, h.st));
  if (nwant) PH_HIP(hipMemcpyAsync(values_dev, want_values, (size_t)nwant * 4u, hipMemcpyHostToDevice, h.st));
  c.filter.label_of = lb->label_of, c.filter.flags = flags;
  c.filter.set_first = first_dev, c.filter.set_values = values_dev, c.filter.set_nwant = (uint32_t)nwant;
  c.sp = sp, c.upto = upto_layers, c.out_stats = h.extra();
  return ph_walk_host_run(ix, h, c, redo_dev, ef, out_ids, out_d, out_len, out_stats);
} catch (...) { return ph_caught(); }
