// Search by a ROW LABEL AND A NUMERIC RANGE of a row attribute (phnsw_label_attr_*,
// phnsw_search_exact_label_ranged[_device], phnsw_search_batch_label_ranged[_device]): `label == want AND lo <= attribute
// <= hi` over a u32 label column and a u32 key column -- this tenant's rows of the last week.  The candidate lists are a
// property of the data once more: the listed rows sorted ONCE by the composite (label << 32) | key, then by id, so that
// every (label, range) pair is one contiguous span of that order.
//
//   listed                iff  v < n, labels[v] != PHNSW_LABEL_NONE, keys[v] != PHNSW_ATTR_NONE, v a vector of the bottom layer
//   candidates of query q  =   the listed vectors with label want[q] and lo[q] <= key <= hi[q], except exclude[q]
//   result                 =   the k candidates with the smallest (distance, id), ascending
//
//   construction  ph_label_pair_kernel (the composite, or UINT64_MAX where the vector is not listed: pair_of, kept with
//                 the handle for the walk), stable radix sort of (composite, id) over all 64 key bits: spairs, ids;
//                 ph_label_attr_head_kernel: listed = the first UINT64_MAX position, the distinct labels, the longest
//                 run of one label
//   a call     1. ph_label_ranged_lookup_kernel: per lookup position its query and the span (at, len) of its pair
//                 (label_range_plan.h; a bad Stored id and an empty span: length 0); radix sort of (span start, position)
//              2. ph_label_ranged_scan_kernel: one wave64 per (position, slice of its span): ph_list_scan (list_scan.h),
//                 the scan loop of the label scan -- every store kind
//              3. ph_list_merge_kernel when the spans were cut into more than one slice
//
// Equality with phnsw_search_exact_filtered over the bitmap {v : v listed, labels[v] == want, lo <= keys[v] <= hi}: spairs
// holds exactly the composites of the listed vectors, so the span IS that set; the ids of a span are not ascending, but
// the keys of the running top-k are (distance, id), distinct, so the k smallest are one set in one order however the span
// is ordered or cut (exact_topk.h); the distances are dist.batch's.  There is no tile path.
//
// A SET of labels and one range per query (phnsw_label_attr_count_set_device,
// phnsw_search_exact_labelset_ranged[_device]; labelset_range_plan.h): `label IN S_q AND lo <= attribute <= hi`.  The
// kernel sequence of the scan by set (filter_labeled.hip) with spans in place of posting lists: a lookup position is a
// (query, wanted label) PAIR --
//   a call     1. ph_labelset_claim_kernel (labelset_claim.h: which query owns a pair; the offsets are not trusted)
//              2. ph_labelset_ranged_lookup_kernel: per pair the span of (its label, its owner's range); the same sort
//              3. ph_labelset_ranged_dup_kernel: a position that repeats the (query, span) of the position before it
//              4. ph_label_ranged_scan_kernel<Dist, PAIRS>: every pair writes its per-slice lists to scratch, none a row
//              5. ph_labelset_ranged_merge_kernel: a wave per query merges the lists of its pairs, duplicates left out
// The subset form (PhLabelsetRangedCall with a list) makes the rows of the listed queries only; its claim runs over the
// whole batch.  No tile path.
//
// The graph walk (at the end of this file) is the search kernels' label-range mode (search_label_ranged.hip) over
// pair_of; the routed call (phnsw_search_label_ranged_auto) is filter_auto.hip's and takes its scan from here through the
// subset form (PhLabelRangedCall::list).
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
#include "label_range_plan.h"
#include "labelset_claim.h"
#include "labelset_range_plan.h"
#include "list_scan.h"
#include "phnsw_device.h"

static_assert(PHNSW_ATTR_NONE == PH_LABEL_RANGE_NONE && PHNSW_LABEL_NONE == PH_LABEL_RANGE_NONE, "label_range_plan.h knows one NONE");

struct phnsw_label_attr {
  const phnsw_index *ix = nullptr;  // the index the columns were sorted for, and what it looked like then
  uint64_t n = 0;
  uint32_t n_nodes = 0;
  int device = 0;
  uint64_t listed = 0, nlabels = 0, longest = 0;
  uint64_t *spairs = nullptr;   // [listed] (allocated [n]) ascending
  uint32_t *ids = nullptr;      // [listed] (allocated [n]): ascending within equal composites
  uint64_t *pair_of = nullptr;  // [n]: the composite of a listed vector, UINT64_MAX elsewhere (the walk's column)
  PhCallPool pool;              // PhLabeledSet, handed out by ph_handle_set_acquire's policy
  PhResidentMemo resident;      // under pool.mutex
};

// ------------------------------------------------------------------ construction

// the composite of a vector as the handle lists it, or UINT64_MAX where the vector is not listed, and the values of the
// construction's sort
__global__ __launch_bounds__(256) void ph_label_pair_kernel(const uint32_t *labels, const uint32_t *keys, uint32_t n, uint32_t n_nodes,
                                                            const uint32_t *nodes, const uint32_t *vec2node, uint64_t *pair_of,
                                                            uint32_t *iota) {
  const uint32_t nlim = ph_exact_id_limit(n, n_nodes, nodes, vec2node);
  for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < n; v += (uint64_t)gridDim.x * 256u) {
    const uint32_t lbl = labels[v], key = keys[v];
    const bool listed = v < nlim && (!vec2node || vec2node[v] != PH_EMPTY32) && lbl != PHNSW_LABEL_NONE && key != PHNSW_ATTR_NONE;
    pair_of[v] = listed ? ph_label_range_pair(lbl, key) : PH_LABEL_RANGE_PAIR_NONE;
    iota[v] = (uint32_t)v;
  }
}

// head[0] = listed, the first UINT64_MAX position of spairs [n]; head[1] = the distinct labels of the listed rows;
// head[2] = the most rows under one label (all preset to 0: nothing listed).  A row that opens a label finds the end of
// the label's run with one binary search over the whole sorted column: UINT64_MAX sorts behind every listed composite.
__global__ __launch_bounds__(256) void ph_label_attr_head_kernel(const uint64_t *spairs, uint32_t n, uint32_t *head) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p <= n; p += (uint64_t)gridDim.x * 256u) {
    const bool none = p == n || spairs[p] == PH_LABEL_RANGE_PAIR_NONE;
    const bool none_before = p > 0 && spairs[p - 1u] == PH_LABEL_RANGE_PAIR_NONE;
    if (none && !none_before) head[0] = (uint32_t)p;
    if (none) continue;
    const uint32_t lbl = (uint32_t)(spairs[p] >> 32);
    if (p > 0 && (uint32_t)(spairs[p - 1u] >> 32) == lbl) continue;
    const uint64_t e = ph_label_range_upper_bound(spairs, n, ph_label_range_pair(lbl, 0xFFFFFFFFu));
    atomicAdd(&head[1], 1u);
    atomicMax(&head[2], (uint32_t)(e - p));
  }
}

// ------------------------------------------------------------------ a call: spans, grouping, the scan

struct PhLabelRangedArgs {
  PhDistArgs dist;
  const float *queries;  // [nq][ldq] or nullptr
  uint32_t ldq;
  const uint32_t *qids, *exclude, *want, *lo, *hi;  // [nq]; qids, exclude nullable
  const uint32_t *list;                             // nullable: the subset form -- lookup position p is query list[p]
  uint32_t nq, n, k, slices;
  const uint64_t *spairs;  // the sorted column
  const uint32_t *ids;
  uint32_t listed;
  // the grouping (range_plan.h), by lookup position: key and iota feed the sort; order = the query of a position
  uint32_t *key, *iota, *order, *at, *len;
  const uint32_t *sorted;  // [nq] by position of the sorted batch: its lookup position
  const uint32_t *dup;     // the PAIRS form: [nq] by lookup position, 1 = scans nothing (labelset_range_plan.h); else nullptr
  uint32_t pq_lds;         // bytes of dynamic LDS in front of the scan's own: a PQ store's table
  uint64_t *scratch;       // slices > 1: [nq lookup positions][slices][k] keys, each list ascending, KEY_NONE padded
  uint32_t *out_ids;       // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
};

__global__ __launch_bounds__(256) void ph_label_ranged_lookup_kernel(PhLabelRangedArgs a) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < a.nq; p += (uint64_t)gridDim.x * 256u) {
    const uint32_t q = ph_label_seed(a.list, (uint32_t)p);
    const bool bad_query = !a.queries && a.qids[q] >= a.n;
    uint32_t at = 0u, len = 0u;
    if (!bad_query) ph_label_range_span(a.spairs, a.listed, a.want[q], a.lo[q], a.hi[q], &at, &len);  // at + len <= listed
    a.order[p] = q, a.at[p] = at, a.len[p] = len;
    a.key[p] = ph_label_range_sort_key(at, len), a.iota[p] = (uint32_t)p;
  }
}

__global__ __launch_bounds__(256) void ph_label_ranged_count_kernel(const uint64_t *spairs, uint32_t listed, const uint32_t *want,
                                                                    const uint32_t *lo, const uint32_t *hi, uint64_t nq,
                                                                    uint32_t *out_count) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * 256u)
    out_count[q] = ph_label_range_count(spairs, listed, want[q], lo[q], hi[q]);
}

// One wave64 per (position of the sorted batch, slice of its span); work item = slice * nq + position (slice-major,
// the positions by span start): the waves resident together read neighbouring rows.  What a wave leaves is addressed by
// the LOOKUP position, which the merge walks.
// PAIRS: the form of phnsw_search_exact_labelset_ranged -- a lookup position is a (query, wanted label) pair, order[p]
// the pair's query; a position never writes a row, its lists go to the scratch at every slice count, and a duplicate
// scans nothing.
template <class Dist, bool PAIRS = false>
__global__ __launch_bounds__(64) void ph_label_ranged_scan_kernel(PhLabelRangedArgs a) {
  extern __shared__ float label_ranged_lds[];
  const uint32_t lane = threadIdx.x;
  uint64_t *const keys = (uint64_t *)((char *)label_ranged_lds + a.pq_lds);
  const uint64_t items = (uint64_t)a.nq * a.slices;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t pos = (uint32_t)(item % a.nq), slice = (uint32_t)(item / a.nq);
    const uint32_t p = min(a.sorted[pos], a.nq - 1u);  // (the sort's value: a lookup position)
    const uint32_t q = a.order[p];
    __syncthreads();  // the previous item's LDS (table, lists) is done with
    const bool bad_query = !a.queries && a.qids[q] >= a.n;
    Dist dist;
    if (a.queries)
      dist.prepare_raw(a.dist, a.queries + (uint64_t)q * a.ldq, label_ranged_lds, lane);
    else if (!bad_query)
      dist.prepare_stored(a.dist, a.qids[q], label_ranged_lds, lane);
    const uint32_t at = a.at[p], len = PAIRS && a.dup[p] ? 0u : a.len[p];  // a bad query's span is empty
    ph_list_scan<PAIRS>(a, dist, keys, a.ids + at, len, q, p, slice, bad_query, lane);  // list_scan.h
  }
}

typedef void (*PhLabelRangedFn)(PhLabelRangedArgs);
// pairs: the PAIRS instance, phnsw_search_exact_labelset_ranged's
template <template <int, int> class D>
static PhLabelRangedFn label_ranged_rows_fn(uint32_t nv4, bool pairs) {
  switch (ph_chunk_count(nv4)) {
    case 1: return pairs ? ph_label_ranged_scan_kernel<D<1, 4>, true> : ph_label_ranged_scan_kernel<D<1, 4>>;
    case 3: return pairs ? ph_label_ranged_scan_kernel<D<3, 4>, true> : ph_label_ranged_scan_kernel<D<3, 4>>;
    case 6: return pairs ? ph_label_ranged_scan_kernel<D<6, 4>, true> : ph_label_ranged_scan_kernel<D<6, 4>>;
    default: return nullptr;
  }
}
static PhLabelRangedFn label_ranged_scan_fn(const phnsw_store *s, bool pairs = false) {
  switch (s->kind) {
    case PH_ROWS_PQ: return pairs ? ph_label_ranged_scan_kernel<DistPQ, true> : ph_label_ranged_scan_kernel<DistPQ>;
    case PH_ROWS_F16: return label_ranged_rows_fn<DistF16>(s->ld / 4, pairs);
    case PH_ROWS_I8: return label_ranged_rows_fn<DistI8>(s->ld / 4, pairs);
    case PH_ROWS_I8Q: return label_ranged_rows_fn<DistI8Q>(s->ld / 4, pairs);
    default: return label_ranged_rows_fn<DistF32>(s->ld / 4, pairs);
  }
}

// ------------------------------------------------------------------ a SET of labels and a range per query: pairs

// a = the block of the scan kernel with nq = nwant lookup positions, the PAIRS: order[i] is the query of pair i (0 for a
// pair that scans nothing), at[i] and len[i] its span, dup[i] the duplicate mark; lo and hi are indexed by QUERY
struct PhLabelsetRangedArgs {
  PhLabelRangedArgs a;
  const uint32_t *want_first, *want_values;  // [nq + 1], [nwant]: the caller's, untrusted
  uint32_t nq, nwant;
  uint32_t *owner;  // [nwant] by pair: the query that claimed it, PH_LABELSET_OWNER_NONE
  uint32_t *dup;    // [nwant] by pair (a.dup, writable)
  // the subset form (a.list != nullptr): the rows of queries a.list[0 .. nlist) are made; sel [nq] = 1 for those
  const uint32_t *sel;
  uint32_t nlist;  // rows the merge writes: the list's length, nq without a list
};

// per pair: its span (empty for an unclaimed pair, for a bad Stored query id and for a query the list leaves out), the
// sort key of the span and the pair itself, the sort's value
__global__ __launch_bounds__(256) void ph_labelset_ranged_lookup_kernel(PhLabelsetRangedArgs s) {
  const PhLabelRangedArgs &a = s.a;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < s.nwant; i += (uint64_t)gridDim.x * 256u) {
    const uint32_t q = s.owner[i];  // NONE or < nq
    const bool dead = q == PH_LABELSET_OWNER_NONE || (!a.queries && a.qids[q] >= a.n) || (s.sel && !s.sel[q]);
    uint32_t at = 0u, len = 0u;
    if (!dead) ph_label_range_span(a.spairs, a.listed, s.want_values[i], a.lo[q], a.hi[q], &at, &len);  // at + len <= listed
    a.order[i] = dead ? 0u : q, a.at[i] = at, a.len[i] = len;
    a.key[i] = ph_label_range_sort_key(at, len), a.iota[i] = (uint32_t)i;
  }
}

// per position after the sort: whether its pair repeats the (query, span) of the pair before it (labelset_range_plan.h)
__global__ __launch_bounds__(256) void ph_labelset_ranged_dup_kernel(PhLabelsetRangedArgs s) {
  const PhLabelRangedArgs &a = s.a;
  for (uint64_t pos = (uint64_t)blockIdx.x * 256u + threadIdx.x; pos < s.nwant; pos += (uint64_t)gridDim.x * 256u) {
    const uint32_t i = min(a.sorted[pos], s.nwant - 1u);
    bool dup = false;
    if (pos > 0) {
      const uint32_t j = min(a.sorted[pos - 1u], s.nwant - 1u);
      dup = ph_labelset_range_dup(a.at[i], a.len[i], s.owner[i], a.at[j], a.len[j], s.owner[j]);
    }
    s.dup[i] = dup ? 1u : 0u;
  }
}

// One wave per query: the lists of every pair of its range -- duplicates and empty spans left out -- through the same
// running top-k as ph_list_merge_kernel, so ties across spans fall in id order.  A refused query (labelset_plan.h)
// gets the empty row and status ST_LABELSET_RANGE.
#define ST_LABELSET_RANGE 8u
__global__ __launch_bounds__(64) void ph_labelset_ranged_merge_kernel(PhLabelsetRangedArgs s) {
  extern __shared__ float label_ranged_lds[];
  const uint32_t lane = threadIdx.x;
  const PhLabelRangedArgs &a = s.a;
  uint64_t *const keys = (uint64_t *)label_ranged_lds;
  for (uint32_t at = blockIdx.x; at < s.nlist; at += gridDim.x) {
    const uint32_t q = a.list ? a.list[at] : at;
    if (q >= s.nq) continue;  // (a list holds query indices of the batch)
    const uint32_t b = s.want_first[q], e = s.want_first[q + 1u];
    const bool ok = ph_labelset_owns_range(s.owner, s.nwant, q, b, e, lane);  // labelset_claim.h
    __syncthreads();
    PhExactTopK top;
    top.init(keys, a.k);
    for (uint32_t i = b; ok && i < e; i++) {  // i < nwant: the range is sound, and every pair of it is q's
      if (s.dup[i] || a.len[i] == 0u) continue;
      for (uint32_t sl = 0; sl < a.slices; sl++)
        PH_EXACT_FEED(top, a.scratch + ((uint64_t)i * a.slices + sl) * a.k, a.k, lane);
    }
    ph_exact_write_row(a, q, top.cur, top.len, !a.queries && a.qids[q] >= a.n, lane);
    if (!ok && lane == 0) a.status[q] = ST_LABELSET_RANGE;  // after the row's own status word, same lane
  }
}

// per query the span lengths of the distinct labels of its range (labelset_range_plan.h); a refused query counts 0: a
// range that is not sound and, with owner[] as the claim kernel left it (nullable), a pair a lower query holds.  One
// wave per query, a pair per lane.
__global__ __launch_bounds__(64) void ph_labelset_ranged_count_kernel(const uint64_t *spairs, uint32_t listed,
                                                                      const uint32_t *want_first, const uint32_t *want_values,
                                                                      const uint32_t *lo, const uint32_t *hi, uint64_t nq,
                                                                      uint32_t nwant, const uint32_t *owner, uint32_t *out_count) {
  const uint32_t lane = threadIdx.x;
  for (uint64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    const uint32_t b = want_first[q], e = want_first[q + 1u];
    uint32_t c = 0;
    bool ok = ph_labelset_range_ok(b, e, nwant);
    if (ok && owner) ok = ph_labelset_owns_range(owner, nwant, (uint32_t)q, b, e, lane);
    if (ok) {
      const uint32_t l = lo[q], h = hi[q];
      for (uint64_t i = (uint64_t)b + lane; i < e; i += 64u)
        c += ph_labelset_range_count_pair(spairs, listed, want_values, b, (uint32_t)i, l, h);
    }
    for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) out_count[q] = c;
  }
}

int ph_label_attr_fresh(const phnsw_index *ix, const phnsw_label_attr *h, const char *call) {
  return ph_snapshot_fresh(ix, h != nullptr, h ? h->ix : nullptr, h ? h->n : 0u, h ? h->n_nodes : 0u, "label and attribute keys", call);
}

// index, k, handle, store: ph_ranged_check's checks in its order
int ph_label_ranged_check(const phnsw_index *ix, const phnsw_label_attr *h, uint64_t k, const char *call) {
  if (ix) PH_TRY(ph_bits_unsupported(ix->store, call));  // a bits store has the plain walk alone
  if (!ix || ix->layers.empty()) {
    ph_set_error("%s: null index or index without layers", call);
    return PHNSW_E_INVALID;
  }
  if (!ph_exact_k_valid(k)) {
    ph_set_error("%s: k must be 1..1024 (got %llu)", call, (unsigned long long)k);
    return PHNSW_E_INVALID;
  }
  PH_TRY(ph_label_attr_fresh(ix, h, call));
  if (ph_store_pq_shared(ix->store)) {  // as for the distance batch, whose arithmetic the scan runs
    ph_set_error("%s: not supported over a shared-codebook PQ store; use its reconstruction store", call);
    return PHNSW_E_UNSUPPORTED;
  }
  return ph_exact_supported(ix, (uint32_t)k);  // the row length, a PQ table beside the scan's LDS
}

const uint64_t *ph_label_attr_column(const phnsw_label_attr *h) { return h->pair_of; }

namespace {

// the orchestration on a set the caller holds; c is checked, 0 < nq <= PH_LABEL_NQ_MAX (with a list: its length).
// Enqueues and returns.
int label_ranged_run(const phnsw_index *ix, const phnsw_label_attr *h, const PhLabelRangedCall &c, PhLabeledSet &set) {
  const phnsw_store *s = ix->store;
  const uint64_t nq = c.nq;
  const PhRangePre lay = ph_range_pre(nq);
  PH_TRY(set.ready());
  PH_TRY(set.block_ensure(&set.pre, &set.pre_bytes, (size_t)lay.words * 4u, c.stream));
  uint32_t *const pre = (uint32_t *)set.pre;
  PhLabelRangedArgs a = {};
  a.dist = ph_dist_args(s);
  a.queries = c.queries, a.ldq = c.ldq, a.qids = c.qids, a.exclude = c.exclude, a.want = c.want, a.lo = c.lo, a.hi = c.hi;
  a.list = c.list;
  a.nq = (uint32_t)nq, a.n = (uint32_t)s->n, a.k = c.k;
  a.spairs = h->spairs, a.ids = h->ids, a.listed = (uint32_t)h->listed;
  a.key = pre + lay.key, a.iota = pre + lay.iota, a.order = pre + lay.query, a.at = pre + lay.at, a.len = pre + lay.len;
  uint32_t *const skey = pre + lay.skey, *const sorted = pre + lay.sorted;
  a.sorted = sorted;
  a.out_ids = c.out_ids, a.out_d = c.out_d, a.out_len = c.out_len, a.status = c.status;

  // before anything is enqueued: the kernel with its dynamic LDS, the slice count from the waves of it the device
  // holds -- `longest` is the longest span a call can ask for; nothing is read back --, hipCUB's temporaries
  const size_t pq_lds = (ph_pq_lds_bytes(s) + 15u) & ~(size_t)15u;
  const PhLabelRangedFn fn = label_ranged_scan_fn(s);
  const size_t lds = pq_lds + (size_t)ph_label_scan_lds(a.k);
  a.pq_lds = (uint32_t)pq_lds;
  phnsw_label_attr *mh = const_cast<phnsw_label_attr *>(h);
  uint64_t resident = 0;
  PH_TRY(ph_resident_waves(mh->resident, mh->pool.mutex, s->device, (const void *)fn, lds, &resident));
  a.slices = ph_label_slice_count(nq, resident, h->longest, env_ll("PHNSW_LABEL_RANGE_SLICES"));
  if (set.tmp_nq != nq) {
    size_t sort_bytes = 0;
    PH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, a.key, skey, a.iota, sorted, (int)nq, 0, 32, c.stream));
    set.tmp_need = std::max<size_t>(sort_bytes, 16), set.tmp_nq = nq;
  }
  PH_TRY(set.block_ensure(&set.tmp, &set.tmp_bytes, set.tmp_need, c.stream));
  if (a.slices > 1u) {
    uint64_t bytes = 0;
    if (!ph_label_key_bytes(nq, a.slices, c.k, &bytes)) {
      ph_set_error("exact label-ranged search: %llu queries in %u slices at k = %u need more scratch than can be addressed",
                   (unsigned long long)nq, a.slices, c.k);
      return PHNSW_E_INVALID;
    }
    PH_TRY(set.block_ensure(&set.keys, &set.keys_bytes, (size_t)bytes, c.stream));
    a.scratch = (uint64_t *)set.keys;
  }

  hipLaunchKernelGGL(ph_label_ranged_lookup_kernel, dim3(grid1(nq)), dim3(256), 0, c.stream, a);
  PH_HIP(hipGetLastError());
  size_t bytes = set.tmp_bytes;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(set.tmp, bytes, a.key, skey, a.iota, sorted, (int)nq, 0, 32, c.stream));
  const uint64_t items = nq * (uint64_t)a.slices;
  hipLaunchKernelGGL(fn, dim3((uint32_t)std::min<uint64_t>(items, 1u << 20)), dim3(64), lds, c.stream, a);
  PH_HIP(hipGetLastError());
  if (a.slices > 1u) {
    hipLaunchKernelGGL(ph_list_merge_kernel<PhLabelRangedArgs>, dim3((uint32_t)std::min<uint64_t>(nq, 1u << 20)), dim3(64),
                       (size_t)ph_label_scan_lds(c.k), c.stream, a);
    PH_HIP(hipGetLastError());
  }
  return 0;
}

// label_ranged_run over pairs (labelset_range_plan.h; the request: PhLabelsetRangedCall, phnsw_internal.h); sc is checked,
// 0 < batch_nq, batch_nq and nwant <= PH_LABEL_NQ_MAX; with c.list, c.nq > 0 is its length.  Enqueues and returns.
int labelset_ranged_run(const phnsw_index *ix, const phnsw_label_attr *h, const PhLabelsetRangedCall &sc, PhLabeledSet &set) {
  const phnsw_store *s = ix->store;
  const PhLabelRangedCall &c = sc.c;
  const uint64_t nq = sc.batch_nq, np = sc.nwant;  // np lookup positions
  const PhLabelsetPre lay = ph_labelset_pre(np);
  PH_TRY(set.ready());
  // (the subset form's marks [nq] behind the layout's words)
  PH_TRY(set.block_ensure(&set.pre, &set.pre_bytes, (size_t)(lay.words + (c.list ? nq : 0u)) * 4u, c.stream));
  uint32_t *const pre = (uint32_t *)set.pre;
  PhLabelsetRangedArgs sa = {};
  PhLabelRangedArgs &a = sa.a;
  a.dist = ph_dist_args(s);
  a.queries = c.queries, a.ldq = c.ldq, a.qids = c.qids, a.exclude = c.exclude, a.lo = c.lo, a.hi = c.hi;
  a.list = c.list;
  a.nq = (uint32_t)np, a.n = (uint32_t)s->n, a.k = c.k, a.slices = 1u;
  a.spairs = h->spairs, a.ids = h->ids, a.listed = (uint32_t)h->listed;
  // the arrays of ph_labelset_pre as labelset_range_plan.h reads them
  a.key = pre + lay.pos.slot, a.iota = pre + lay.pos.iota, a.order = pre + lay.pos.order;
  a.at = pre + lay.pos.tile_first, a.len = pre + lay.pos.flags;
  uint32_t *const skey = pre + lay.pos.sslot, *const sorted = pre + lay.spair;
  a.sorted = sorted;
  sa.owner = pre + lay.owner, sa.dup = pre + lay.dup, a.dup = sa.dup;
  a.out_ids = c.out_ids, a.out_d = c.out_d, a.out_len = c.out_len, a.status = c.status;
  sa.want_first = sc.want_first, sa.want_values = sc.want_values, sa.nq = (uint32_t)nq, sa.nwant = (uint32_t)np;
  sa.nlist = (uint32_t)(c.list ? c.nq : nq);

  if (np) {
    // before anything is enqueued: the kernel with its dynamic LDS, the slice count, hipCUB's temporaries
    const size_t pq_lds = (ph_pq_lds_bytes(s) + 15u) & ~(size_t)15u;
    const PhLabelRangedFn fn = label_ranged_scan_fn(s, true);
    const size_t lds = pq_lds + (size_t)ph_label_scan_lds(a.k);
    a.pq_lds = (uint32_t)pq_lds;
    phnsw_label_attr *mh = const_cast<phnsw_label_attr *>(h);
    uint64_t resident = 0;
    PH_TRY(ph_resident_waves(mh->resident, mh->pool.mutex, s->device, (const void *)fn, lds, &resident));
    a.slices = ph_label_slice_count(np, resident, h->longest, env_ll("PHNSW_LABELSET_RANGE_SLICES"));
    if (set.tmp_nq != np) {
      size_t sort_bytes = 0;
      PH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, a.key, skey, a.iota, sorted, (int)np, 0, 32, c.stream));
      set.tmp_need = std::max<size_t>(sort_bytes, 16), set.tmp_nq = np;
    }
    PH_TRY(set.block_ensure(&set.tmp, &set.tmp_bytes, set.tmp_need, c.stream));
    uint64_t bytes = 0;
    if (!ph_labelset_key_bytes(np, a.slices, c.k, &bytes)) {
      ph_set_error("exact labelset-ranged search: %llu wanted labels in %u slices at k = %u need more scratch than can be addressed",
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
    hipLaunchKernelGGL(ph_labelset_ranged_lookup_kernel, dim3(grid1(np)), dim3(256), 0, c.stream, sa);
    PH_HIP(hipGetLastError());
    size_t tmp_bytes = set.tmp_bytes;
    PH_HIP(hipcub::DeviceRadixSort::SortPairs(set.tmp, tmp_bytes, a.key, skey, a.iota, sorted, (int)np, 0, 32, c.stream));
    hipLaunchKernelGGL(ph_labelset_ranged_dup_kernel, dim3(grid1(np)), dim3(256), 0, c.stream, sa);
    PH_HIP(hipGetLastError());
    const uint64_t items = np * (uint64_t)a.slices;
    hipLaunchKernelGGL(fn, dim3((uint32_t)std::min<uint64_t>(items, 1u << 20)), dim3(64), lds, c.stream, a);
    PH_HIP(hipGetLastError());
  }
  // no pair at all: every sound range is empty, and the merge alone writes the rows
  hipLaunchKernelGGL(ph_labelset_ranged_merge_kernel, dim3((uint32_t)std::min<uint64_t>(sa.nlist, 1u << 20)), dim3(64),
                     (size_t)ph_label_scan_lds(c.k), c.stream, sa);
  PH_HIP(hipGetLastError());
  return 0;
}

void label_attr_free(phnsw_label_attr *h) {
  ph_handle_sets_free(h->pool);
  if (h->spairs) hipFree(h->spairs);
  if (h->ids) hipFree(h->ids);
  if (h->pair_of) hipFree(h->pair_of);
  delete h;
}

// the sorted column of (labels_dev, keys_dev) [n] on `stream`; synchronises it
int label_attr_build(const phnsw_index *ix, const uint32_t *labels_dev, const uint32_t *keys_dev, uint64_t n, hipStream_t stream,
                     const char *call, phnsw_label_attr **out) {
  const phnsw_store *s = ix->store;
  phnsw_label_attr *h = new phnsw_label_attr();
  h->ix = ix, h->n = n, h->n_nodes = ix->layers.back().n_nodes, h->device = s->device;
  struct Drop {
    phnsw_label_attr *h;
    ~Drop() {
      if (h) label_attr_free(h);
    }
  } drop{h};
  if (n == 0) {
    PH_HIP(hipMalloc(&h->pair_of, 8));  // never null: a null column would read as "no label-range filter"
    PH_HIP(hipMemsetAsync(h->pair_of, 0xFF, 8, stream));
    PH_HIP(hipMalloc(&h->spairs, 8));
    PH_HIP(hipMalloc(&h->ids, 4));
    PH_HIP(hipStreamSynchronize(stream));
    *out = h, drop.h = nullptr;
    return 0;
  }
  uint32_t n_nodes;
  const uint32_t *nodes, *vec2node;
  ph_exact_bottom_layer(ix, &n_nodes, &nodes, &vec2node);
  HostBlocks hb{stream, {}};
  uint32_t *iota = nullptr, *head = nullptr;
  void *tmp = nullptr;
  PH_HIP(hipMalloc(&h->pair_of, (size_t)n * 8u));  // the sort's keys, which it leaves as they are: kept
  PH_HIP(hipMalloc(&h->spairs, (size_t)n * 8u));
  PH_HIP(hipMalloc(&h->ids, (size_t)n * 4u));
  PH_TRY(hb.alloc(&iota, (size_t)n * 4u));
  PH_TRY(hb.alloc(&head, 16));
  size_t tmp_bytes = 0;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, h->pair_of, h->spairs, iota, h->ids, (int)n, 0, 64, stream));
  tmp_bytes = std::max<size_t>(tmp_bytes, 16);
  PH_TRY(hb.alloc(&tmp, tmp_bytes));
  hipLaunchKernelGGL(ph_label_pair_kernel, dim3(grid1(n)), dim3(256), 0, stream, labels_dev, keys_dev, (uint32_t)n, n_nodes, nodes,
                     vec2node, h->pair_of, iota);
  PH_HIP(hipGetLastError());
  size_t bytes = tmp_bytes;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, h->pair_of, h->spairs, iota, h->ids, (int)n, 0, 64, stream));
  PH_HIP(hipMemsetAsync(head, 0, 16, stream));
  hipLaunchKernelGGL(ph_label_attr_head_kernel, dim3(grid1(n + 1u)), dim3(256), 0, stream, h->spairs, (uint32_t)n, head);
  PH_HIP(hipGetLastError());
  uint32_t hd[4] = {0, 0, 0, 0};
  PH_HIP(hipMemcpyAsync(hd, head, 16, hipMemcpyDeviceToHost, stream));
  PH_HIP(hipStreamSynchronize(stream));
  h->listed = hd[0], h->nlabels = hd[1], h->longest = hd[2];
  if (h->listed > n || h->longest > h->listed) {
    ph_set_error("%s: the labels or the keys changed while the column was sorted", call);
    return PHNSW_E_INVALID;
  }
  *out = h, drop.h = nullptr;
  return 0;
}

int label_attr_create_check(const phnsw_index *ix, const void *labels, const void *keys, uint64_t n, phnsw_label_attr **out,
                            const char *call) {
  if (!ix || ix->layers.empty()) {
    ph_set_error("%s: null index or index without layers", call);
    return PHNSW_E_INVALID;
  }
  if (!out || ((!labels || !keys) && n)) {
    ph_set_error("%s: null labels, null keys or null output", call);
    return PHNSW_E_INVALID;
  }
  if (n != ix->store->n) {
    ph_set_error("%s: %llu labels and keys for a store of %llu vectors (one of each per vector)", call, (unsigned long long)n,
                 (unsigned long long)ix->store->n);
    return PHNSW_E_INVALID;
  }
  return 0;
}

// what both forms of the walk check before they look at a pointer: index and parameters, the handle, the flags
int walk_check(const phnsw_index *ix, const phnsw_label_attr *h, const phnsw_search_params *sp, uint32_t flags, const char *call) {
  if (ix) PH_TRY(ph_bits_unsupported(ix->store, call));  // a bits store has the plain walk alone
  PH_TRY(ph_check_sp(ix, sp));
  PH_TRY(ph_label_attr_fresh(ix, h, call));
  if (flags & ~(uint32_t)PHNSW_FILTER_STRICT) {
    ph_set_error("%s: unknown flag bits 0x%x", call, flags);
    return PHNSW_E_INVALID;
  }
  return 0;
}

}  // namespace

int ph_label_attr_count(const phnsw_label_attr *h, const uint32_t *want_dev, const uint32_t *lo_dev, const uint32_t *hi_dev,
                        uint64_t nq, uint32_t *out_count_dev, hipStream_t stream) {
  hipLaunchKernelGGL(ph_label_ranged_count_kernel, dim3(grid1(nq)), dim3(256), 0, stream, h->spairs, (uint32_t)h->listed, want_dev,
                     lo_dev, hi_dev, nq, out_count_dev);
  PH_HIP(hipGetLastError());
  return 0;
}

int ph_label_attr_count_set(const phnsw_label_attr *h, const uint32_t *want_first_dev, const uint32_t *want_values_dev,
                            const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t nq, uint64_t nwant, uint32_t *out_count_dev,
                            uint32_t *owner_scratch, hipStream_t stream) {
  uint32_t *const owner = nwant ? owner_scratch : nullptr;  // without a pair no range overlaps another
  if (owner) {
    PH_HIP(hipMemsetAsync(owner, 0xFF, (size_t)nwant * 4u, stream));  // PH_LABELSET_OWNER_NONE
    hipLaunchKernelGGL(ph_labelset_claim_kernel, dim3(grid1(nq)), dim3(256), 0, stream, want_first_dev, (uint32_t)nq, (uint32_t)nwant, owner);
    PH_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(ph_labelset_ranged_count_kernel, dim3((uint32_t)std::min<uint64_t>(nq, 1u << 20)), dim3(64), 0, stream, h->spairs,
                     (uint32_t)h->listed, want_first_dev, want_values_dev, lo_dev, hi_dev, nq, (uint32_t)nwant, owner, out_count_dev);
  PH_HIP(hipGetLastError());
  return 0;
}

int ph_labelset_ranged_device(const phnsw_index *ix, const phnsw_label_attr *h, const PhLabelsetRangedCall &sc) {
  if (sc.c.nq == 0 || sc.batch_nq == 0) return 0;
  phnsw_label_attr *mh = const_cast<phnsw_label_attr *>(h);
  PhLabeledSet *set = ph_handle_set_acquire(mh->pool, sc.c.stream, false);
  PhSetGuard guard{mh->pool, set, sc.c.stream};
  return labelset_ranged_run(ix, h, sc, *set);
}

int ph_label_ranged_device(const phnsw_index *ix, const phnsw_label_attr *h, const PhLabelRangedCall &c) {
  if (c.nq == 0) return 0;
  phnsw_label_attr *mh = const_cast<phnsw_label_attr *>(h);
  PhLabeledSet *set = ph_handle_set_acquire(mh->pool, c.stream, false);
  PhSetGuard guard{mh->pool, set, c.stream};
  return label_ranged_run(ix, h, c, *set);
}

// ------------------------------------------------------------------ C ABI: the handle

extern "C" int phnsw_label_attr_create_device(const phnsw_index *ix, const uint32_t *labels_dev, const uint32_t *keys_dev, uint64_t n,
                                              void *stream, phnsw_label_attr **out) try {
  const char *const call = "phnsw_label_attr_create_device";
  PH_TRY(label_attr_create_check(ix, labels_dev, keys_dev, n, out, call));
  PH_HIP(hipSetDevice(ix->store->device));
  return label_attr_build(ix, labels_dev, keys_dev, n, (hipStream_t)stream, call, out);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_label_attr_create(const phnsw_index *ix, const uint32_t *labels, const uint32_t *keys, uint64_t n,
                                       phnsw_label_attr **out) try {
  const char *const call = "phnsw_label_attr_create";
  PH_TRY(label_attr_create_check(ix, labels, keys, n, out, call));
  PH_HIP(hipSetDevice(ix->store->device));
  HostBlocks hb{nullptr, {}};
  uint32_t *dev = nullptr;
  PH_TRY(hb.alloc(&dev, (size_t)n * 8u));  // labels | keys
  if (n) {
    PH_HIP(hipMemcpy(dev, labels, (size_t)n * 4u, hipMemcpyHostToDevice));
    PH_HIP(hipMemcpy(dev + n, keys, (size_t)n * 4u, hipMemcpyHostToDevice));
  }
  return label_attr_build(ix, dev, dev + n, n, nullptr, call, out);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_label_attr_info(const phnsw_label_attr *h, uint64_t *n, uint64_t *listed, uint64_t *nlabels,
                                     uint64_t *longest) try {
  if (!h) {
    ph_set_error("phnsw_label_attr_info: null label and attribute keys");
    return PHNSW_E_INVALID;
  }
  if (n) *n = h->n;
  if (listed) *listed = h->listed;
  if (nlabels) *nlabels = h->nlabels;
  if (longest) *longest = h->longest;
  return 0;
} catch (...) { return ph_caught(); }

extern "C" int phnsw_label_attr_count_device(const phnsw_label_attr *h, const uint32_t *want_dev, const uint32_t *lo_dev,
                                             const uint32_t *hi_dev, uint64_t nq, uint32_t *out_count_dev, void *stream) try {
  const char *const call = "phnsw_label_attr_count_device";
  if (!h) {
    ph_set_error("%s: null label and attribute keys", call);
    return PHNSW_E_INVALID;
  }
  if (nq == 0) return 0;
  if (!want_dev || !lo_dev || !hi_dev || !out_count_dev) {
    ph_set_error("%s: null want, null lo, null hi or null output", call);
    return PHNSW_E_INVALID;
  }
  PH_HIP(hipSetDevice(h->device));
  return ph_label_attr_count(h, want_dev, lo_dev, hi_dev, nq, out_count_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" void phnsw_label_attr_destroy(phnsw_label_attr *h) {
  if (!h) return;
  try {
    hipSetDevice(h->device);
    label_attr_free(h);  // waits for the events that close the calls in flight
  } catch (...) {
  }
}

// ------------------------------------------------------------------ C ABI: exact top-k over a label and a range

extern "C" int phnsw_search_exact_label_ranged_device(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries_dev,
                                                      uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                      const uint32_t *exclude_dev, const uint32_t *want_dev, const uint32_t *lo_dev,
                                                      const uint32_t *hi_dev, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                                      uint32_t *out_len_dev, uint32_t *status_dev, void *stream) try {
  const char *const call = "phnsw_search_exact_label_ranged_device";
  PH_TRY(ph_label_ranged_check(ix, h, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !want_dev || !lo_dev || !hi_dev || nq > PH_LABEL_NQ_MAX) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; want, lo and hi; nq < 2^31 - 1; queries need "
                 "ldq >= store ld, multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhLabelRangedCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq;
  c.want = want_dev, c.lo = lo_dev, c.hi = hi_dev;
  c.k = (uint32_t)k;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_label_ranged_device(ix, h, c);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_label_ranged(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries,
                                               const uint64_t *qids, uint64_t nq, const uint64_t *exclude, const uint32_t *want,
                                               const uint32_t *lo, const uint32_t *hi, uint64_t k, uint64_t *out_ids, float *out_d,
                                               uint64_t *out_len) try {
  const char *const call = "phnsw_search_exact_label_ranged";
  PH_TRY(ph_label_ranged_check(ix, h, k, call));
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!out_ids || !out_d || !out_len || !want || !lo || !hi || nq > PH_LABEL_NQ_MAX) {
    ph_set_error("%s: invalid argument (outputs; want, lo and hi; nq < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, call));
  phnsw_label_attr *mh = const_cast<phnsw_label_attr *>(h);
  PhLabeledSet *set = ph_handle_set_acquire(mh->pool, nullptr, true);
  PhHostCall hc(mh->pool, set);
  PH_TRY(hc.stage_in(s, queries, qids, exclude, nq, (size_t)nq * 3u, 0, (uint32_t)k, (uint32_t)k));  // extras: want | lo | hi
  PhLabelRangedCall c = {};
  hc.fill(c);
  uint32_t *const want_dev = hc.extra(), *const lo_dev = want_dev + nq, *const hi_dev = lo_dev + nq;
  PH_HIP(hipMemcpyAsync(want_dev, want, (size_t)nq * 4u, hipMemcpyHostToDevice, hc.st));
  PH_HIP(hipMemcpyAsync(lo_dev, lo, (size_t)nq * 4u, hipMemcpyHostToDevice, hc.st));
  PH_HIP(hipMemcpyAsync(hi_dev, hi, (size_t)nq * 4u, hipMemcpyHostToDevice, hc.st));
  c.want = want_dev, c.lo = lo_dev, c.hi = hi_dev, c.k = (uint32_t)k;
  PH_TRY(label_ranged_run(ix, h, c, *set));
  return hc.finish(out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }

// ------------------------------------------------------------------ C ABI: a set of labels and a range per query

extern "C" int phnsw_label_attr_count_set_device(const phnsw_label_attr *h, const uint32_t *want_first_dev,
                                                 const uint32_t *want_values_dev, const uint32_t *lo_dev, const uint32_t *hi_dev,
                                                 uint64_t nq, uint64_t nwant, uint32_t *out_count_dev, void *stream) try {
  const char *const call = "phnsw_label_attr_count_set_device";
  if (!h) {
    ph_set_error("%s: null label and attribute keys", call);
    return PHNSW_E_INVALID;
  }
  if (nq == 0) return 0;
  if (!want_first_dev || !lo_dev || !hi_dev || !out_count_dev || (!want_values_dev && nwant)) {
    ph_set_error("%s: null want_first, null want_values with nwant > 0, null lo, null hi or null output", call);
    return PHNSW_E_INVALID;
  }
  if (nq > PH_LABEL_NQ_MAX || nwant > PH_LABELSET_NWANT_MAX) {
    ph_set_error("%s: nq and nwant must be below 2^31 - 1", call);
    return PHNSW_E_INVALID;
  }
  PH_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  if (!nwant) return ph_label_attr_count_set(h, want_first_dev, want_values_dev, lo_dev, hi_dev, nq, 0u, out_count_dev, nullptr, st);
  // the claim's owner words [nwant]: a scratch set of the handle, as the scan takes one
  phnsw_label_attr *mh = const_cast<phnsw_label_attr *>(h);
  PhLabeledSet *set = ph_handle_set_acquire(mh->pool, st, false);
  PhSetGuard guard{mh->pool, set, st};
  PH_TRY(set->ready());
  PH_TRY(set->block_ensure(&set->pre, &set->pre_bytes, (size_t)nwant * 4u, st));
  return ph_label_attr_count_set(h, want_first_dev, want_values_dev, lo_dev, hi_dev, nq, nwant, out_count_dev, (uint32_t *)set->pre, st);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_labelset_ranged_device(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries_dev,
                                                         uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                         const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                                         const uint32_t *want_values_dev, uint64_t nwant, const uint32_t *lo_dev,
                                                         const uint32_t *hi_dev, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                                         uint32_t *out_len_dev, uint32_t *status_dev, void *stream) try {
  const char *const call = "phnsw_search_exact_labelset_ranged_device";
  PH_TRY(ph_label_ranged_check(ix, h, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !want_first_dev || (!want_values_dev && nwant) || !lo_dev || !hi_dev) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; want_first; want_values unless nwant is 0; lo and "
                 "hi; queries need ldq >= store ld, multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  if (nq > PH_LABEL_NQ_MAX || nwant > PH_LABELSET_NWANT_MAX) {
    ph_set_error("%s: nq and nwant must be below 2^31 - 1", call);
    return PHNSW_E_INVALID;
  }
  PhLabelsetRangedCall sc = {};
  PhLabelRangedCall &c = sc.c;
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq, c.k = (uint32_t)k;
  c.lo = lo_dev, c.hi = hi_dev;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  sc.want_first = want_first_dev, sc.want_values = want_values_dev, sc.nwant = nwant, sc.batch_nq = nq;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_labelset_ranged_device(ix, h, sc);
} catch (...) { return ph_caught(); }

// the offset and size checks the host forms by set and range make once outputs and pointers are known to be there:
// want_values against want_first[nq], the Stored ids, the offsets, each naming the call and the query
static int labelset_ranged_host_check(const char *call, const phnsw_store *s, const uint64_t *qids, uint64_t nq,
                                      const uint32_t *want_first, const uint32_t *want_values, uint64_t *nwant) {
  *nwant = want_first[nq];
  if ((!want_values && *nwant) || *nwant > PH_LABELSET_NWANT_MAX) {
    ph_set_error("%s: invalid argument (want_values unless want_first[nq] is 0; want_first[nq] < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, call, true));
  if (const uint64_t bad = ph_labelset_first_bad(want_first, nq); bad < nq) {
    ph_set_error("%s: query %llu: want_first must start at 0 and never run backwards (want_first[%llu] = %u, want_first[%llu] "
                 "= %u)", call, (unsigned long long)bad, (unsigned long long)bad, want_first[bad], (unsigned long long)bad + 1u,
                 want_first[bad + 1u]);
    return PHNSW_E_INVALID;
  }
  return 0;
}

extern "C" int phnsw_search_exact_labelset_ranged(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries,
                                                  const uint64_t *qids, uint64_t nq, const uint64_t *exclude,
                                                  const uint32_t *want_first, const uint32_t *want_values, const uint32_t *lo,
                                                  const uint32_t *hi, uint64_t k, uint64_t *out_ids, float *out_d,
                                                  uint64_t *out_len) try {
  const char *const call = "phnsw_search_exact_labelset_ranged";
  PH_TRY(ph_label_ranged_check(ix, h, k, call));
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!out_ids || !out_d || !out_len || !want_first || !lo || !hi || nq > PH_LABEL_NQ_MAX) {
    ph_set_error("%s: invalid argument (outputs; want_first, lo and hi; nq < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  uint64_t nwant = 0;
  PH_TRY(labelset_ranged_host_check(call, s, qids, nq, want_first, want_values, &nwant));
  phnsw_label_attr *mh = const_cast<phnsw_label_attr *>(h);
  PhLabeledSet *set = ph_handle_set_acquire(mh->pool, nullptr, true);
  PhHostCall hc(mh->pool, set);
  // extras: want_first [nq + 1] | want_values [nwant] | lo | hi
  PH_TRY(hc.stage_in(s, queries, qids, exclude, nq, (size_t)nq * 3u + 1u + (size_t)nwant, 0, (uint32_t)k, (uint32_t)k));
  PhLabelsetRangedCall sc = {};
  hc.fill(sc.c);
  uint32_t *const first_dev = hc.extra(), *const values_dev = first_dev + nq + 1u, *const lo_dev = values_dev + nwant;
  uint32_t *const hi_dev = lo_dev + nq;
  PH_HIP(hipMemcpyAsync(first_dev, want_first, (size_t)(nq + 1u) * 4u, hipMemcpyHostToDevice, hc.st));
  if (nwant) PH_HIP(hipMemcpyAsync(values_dev, want_values, (size_t)nwant * 4u, hipMemcpyHostToDevice, hc.st));
  PH_HIP(hipMemcpyAsync(lo_dev, lo, (size_t)nq * 4u, hipMemcpyHostToDevice, hc.st));
  PH_HIP(hipMemcpyAsync(hi_dev, hi, (size_t)nq * 4u, hipMemcpyHostToDevice, hc.st));
  sc.want_first = first_dev, sc.want_values = values_dev, sc.nwant = nwant, sc.batch_nq = nq;
  sc.c.lo = lo_dev, sc.c.hi = hi_dev, sc.c.k = (uint32_t)k;
  PH_TRY(labelset_ranged_run(ix, h, sc, *set));
  return hc.finish(out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }

// ------------------------------------------------------------------ the graph walk by label and range

extern "C" int phnsw_search_batch_label_ranged_device(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries_dev,
                                                      uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                      const phnsw_search_params *sp, uint32_t upto_layers,
                                                      const uint32_t *exclude_dev, const uint32_t *want_dev, const uint32_t *lo_dev,
                                                      const uint32_t *hi_dev, uint32_t flags, uint32_t *out_ids_dev, float *out_d_dev,
                                                      uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev,
                                                      void *stream) try {
  const char *const call = "phnsw_search_batch_label_ranged_device";
  PH_TRY(walk_check(ix, h, sp, flags, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !want_dev || !lo_dev || !hi_dev || nq > 0xFFFFFFFFull) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; want, lo and hi; queries need ldq >= store ld, "
                 "multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhSearchCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq;
  c.sp = sp, c.upto = upto_layers;
  c.filter.pair_of = h->pair_of, c.filter.pair_want = want_dev, c.filter.pair_lo = lo_dev, c.filter.pair_hi = hi_dev;
  c.filter.flags = flags;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.status = status_dev, c.out_stats = out_stats_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_search_device(ix, c);
} catch (...) { return ph_caught(); }

// The host form stages everything once, on the stream of a scratch set of the handle, as phnsw_search_batch_ranged does.
extern "C" int phnsw_search_batch_label_ranged(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries,
                                               const uint64_t *qids, uint64_t nq, const phnsw_search_params *sp,
                                               uint32_t upto_layers, const uint64_t *exclude, const uint32_t *want,
                                               const uint32_t *lo, const uint32_t *hi, uint32_t flags, uint64_t k, uint64_t *out_ids,
                                               float *out_d, uint64_t *out_len, uint64_t *out_stats) try {
  const char *const call = "phnsw_search_batch_label_ranged";
  PH_TRY(walk_check(ix, h, sp, flags, call));
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
  if (!out_ids || !out_d || !out_len || !want || !lo || !hi || nq > 0xFFFFFFFFull) {
    ph_set_error("%s: invalid argument (outputs; want, lo and hi; nq < 2^32)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, call));
  phnsw_label_attr *mh = const_cast<phnsw_label_attr *>(h);
  PhLabeledSet *set = ph_handle_set_acquire(mh->pool, nullptr, true);
  PhHostCall hc(mh->pool, set);
  // extras: stats(2), which the host reads back with len and status | want | lo | hi | the redo list
  PH_TRY(hc.stage_in(s, queries, qids, exclude, nq, (size_t)nq * 6u, 2, ef, k ? (uint32_t)k : ef));
  uint32_t *const want_dev = hc.extra() + 2u * nq, *const lo_dev = want_dev + nq, *const hi_dev = lo_dev + nq;
  uint32_t *const redo_dev = hi_dev + nq;
  PhSearchCall c = {};
  hc.fill(c);
  PH_HIP(hipMemcpyAsync(want_dev, want, (size_t)nq * 4u, hipMemcpyHostToDevice, hc.st));
  PH_HIP(hipMemcpyAsync(lo_dev, lo, (size_t)nq * 4u, hipMemcpyHostToDevice, hc.st));
  PH_HIP(hipMemcpyAsync(hi_dev, hi, (size_t)nq * 4u, hipMemcpyHostToDevice, hc.st));
  c.filter.pair_of = h->pair_of, c.filter.pair_want = want_dev, c.filter.pair_lo = lo_dev, c.filter.pair_hi = hi_dev;
  c.filter.flags = flags;
  c.sp = sp, c.upto = upto_layers, c.out_stats = hc.extra();
  return ph_walk_host_run(ix, hc, c, redo_dev, ef, out_ids, out_d, out_len, out_stats);
} catch (...) { return ph_caught(); }

// ------------------------------------------------------------------ the graph walk by a set of labels and a range

// The search kernels' set-range mode (search_labelset_ranged.hip) over pair_of, the caller's table and the bounds.  The
// device form hands the table to the kernels as it is: they refuse a range that is not sound per query (status 8) and
// read nothing outside want_values[0 .. nwant); ranges that OVERLAP are harmless to a walk and are not detected here.
extern "C" int phnsw_search_batch_labelset_ranged_device(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries_dev,
                                                         uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                         const phnsw_search_params *sp, uint32_t upto_layers,
                                                         const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                                         const uint32_t *want_values_dev, uint64_t nwant, const uint32_t *lo_dev,
                                                         const uint32_t *hi_dev, uint32_t flags, uint32_t *out_ids_dev,
                                                         float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_stats_dev,
                                                         uint32_t *status_dev, void *stream) try {
  const char *const call = "phnsw_search_batch_labelset_ranged_device";
  PH_TRY(walk_check(ix, h, sp, flags, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !want_first_dev || (!want_values_dev && nwant) || !lo_dev || !hi_dev) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; want_first; want_values unless nwant is 0; lo and "
                 "hi; queries need ldq >= store ld, multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  if (nq > PH_LABEL_NQ_MAX || nwant > PH_LABELSET_NWANT_MAX) {
    ph_set_error("%s: nq and nwant must be below 2^31 - 1", call);
    return PHNSW_E_INVALID;
  }
  PhSearchCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq;
  c.sp = sp, c.upto = upto_layers;
  c.filter.pair_of = h->pair_of, c.filter.pair_lo = lo_dev, c.filter.pair_hi = hi_dev, c.filter.flags = flags;
  c.filter.set_first = want_first_dev, c.filter.set_values = want_values_dev, c.filter.set_nwant = (uint32_t)nwant;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.status = status_dev, c.out_stats = out_stats_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_search_device(ix, c);
} catch (...) { return ph_caught(); }

// The host form stages everything once, as phnsw_search_batch_labelset does, with the bounds behind the table.  The
// offsets are checked here, so no query can come back with status 8.
extern "C" int phnsw_search_batch_labelset_ranged(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries,
                                                  const uint64_t *qids, uint64_t nq, const phnsw_search_params *sp,
                                                  uint32_t upto_layers, const uint64_t *exclude, const uint32_t *want_first,
                                                  const uint32_t *want_values, const uint32_t *lo, const uint32_t *hi,
                                                  uint32_t flags, uint64_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len,
                                                  uint64_t *out_stats) try {
  const char *const call = "phnsw_search_batch_labelset_ranged";
  PH_TRY(walk_check(ix, h, sp, flags, call));
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
  if (!out_ids || !out_d || !out_len || !want_first || !lo || !hi || nq > PH_LABEL_NQ_MAX) {
    ph_set_error("%s: invalid argument (outputs; want_first, lo and hi; nq < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  uint64_t nwant = 0;
  PH_TRY(labelset_ranged_host_check(call, s, qids, nq, want_first, want_values, &nwant));
  phnsw_label_attr *mh = const_cast<phnsw_label_attr *>(h);
  PhLabeledSet *set = ph_handle_set_acquire(mh->pool, nullptr, true);
  PhHostCall hc(mh->pool, set);
  // extras: stats(2), which the host reads back with len and status | want_first [nq + 1] | want_values [nwant] | lo | hi |
  // the redo list
  PH_TRY(hc.stage_in(s, queries, qids, exclude, nq, (size_t)nq * 6u + 1u + (size_t)nwant, 2, ef, k ? (uint32_t)k : ef));
  uint32_t *const first_dev = hc.extra() + 2u * nq, *const values_dev = first_dev + nq + 1u, *const lo_dev = values_dev + nwant;
  uint32_t *const hi_dev = lo_dev + nq, *const redo_dev = hi_dev + nq;
  PhSearchCall c = {};
  hc.fill(c);
  PH_HIP(hipMemcpyAsync(first_dev, want_first, (size_t)(nq + 1u) * 4u, hipMemcpyHostToDevice, hc.st));
  if (nwant) PH_HIP(hipMemcpyAsync(values_dev, want_values, (size_t)nwant * 4u, hipMemcpyHostToDevice, hc.st));
  PH_HIP(hipMemcpyAsync(lo_dev, lo, (size_t)nq * 4u, hipMemcpyHostToDevice, hc.st));
  PH_HIP(hipMemcpyAsync(hi_dev, hi, (size_t)nq * 4u, hipMemcpyHostToDevice, hc.st));
  c.filter.pair_of = h->pair_of, c.filter.pair_lo = lo_dev, c.filter.pair_hi = hi_dev, c.filter.flags = flags;
  c.filter.set_first = first_dev, c.filter.set_values = values_dev, c.filter.set_nwant = (uint32_t)nwant;
  c.sp = sp, c.upto = upto_layers, c.out_stats = hc.extra();
  return ph_walk_host_run(ix, hc, c, redo_dev, ef, out_ids, out_d, out_len, out_stats);
} catch (...) { return ph_caught(); }
