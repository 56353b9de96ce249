// Search by a NUMERIC RANGE of a row attribute (phnsw_attr_*, phnsw_search_exact_ranged[_device],
// phnsw_search_batch_ranged[_device]): `lo <= attribute <= hi` over a u32 key column -- timestamps, prices, versions.
// The candidate lists are a property of the data once more: the listed rows sorted ONCE by (key, id), so that every
// range is one contiguous span of that order.
//
//   listed                iff  v < n, keys[v] != PHNSW_ATTR_NONE, v a vector of the bottom layer
//   candidates of query q  =   the listed vectors with lo[q] <= key <= hi[q], except exclude[q]
//   result                 =   the k candidates with the smallest (distance, id), ascending
//
//   construction  ph_label_key_kernel (the key, or NONE where the vector is not listed: attr_of, kept with the handle
//                 for the range walk), stable radix sort of (key, id): skeys, ids; ph_attr_head_kernel: listed = the
//                 first NONE position, the smallest and the largest key
//   a call     1. ph_ranged_lookup_kernel: per lookup position its query and the span (at, len) of its range
//                 (range_plan.h; a bad Stored id and an empty range: length 0); radix sort of (span start, position)
//              2. ph_ranged_scan_kernel: one wave64 per (position, slice of its span): ph_list_scan (list_scan.h), the
//                 scan loop of the label scan -- every store kind
//              3. ph_list_merge_kernel when the spans were cut into more than one slice
//
// Equality with phnsw_search_exact_filtered over the bitmap {v : v listed, lo <= keys[v] <= hi}: skeys holds exactly the
// keys of the listed vectors, so the span IS that set; the ids of a span are not ascending, but the keys of the running
// top-k are (distance, id), distinct, so the k smallest are one set in one order however the span is ordered or cut
// (exact_topk.h); the distances are dist.batch's.  There is no tile path: tiles share rows between the queries of ONE
// list, and overlapping spans are not one list.
//
// The graph walk by range (at the end of this file) is the search kernels' range mode (search_ranged.hip) over attr_of;
// the routed call (phnsw_search_ranged_auto) is filter_auto.hip's and takes its scan from here through the subset form
// (PhRangedCall::list).
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
#include "list_scan.h"
#include "phnsw_device.h"
#include "range_plan.h"

static_assert(PHNSW_ATTR_NONE == PHNSW_LABEL_NONE && PHNSW_ATTR_NONE == PH_RANGE_KEY_NONE, "ph_label_key_kernel writes one NONE");

struct phnsw_attr {
  const phnsw_index *ix = nullptr;  // the index the column was sorted for, and what it looked like then
  uint64_t n = 0;
  uint32_t n_nodes = 0;
  int device = 0;
  uint64_t listed = 0;
  uint32_t key_min = 0xFFFFFFFFu, key_max = 0u;
  uint32_t *skeys = nullptr;    // [listed] (allocated [n]) ascending
  uint32_t *ids = nullptr;      // [listed] (allocated [n]): ascending within equal keys
  uint32_t *attr_of = nullptr;  // [n]: the key of a listed vector, PHNSW_ATTR_NONE elsewhere (the range walk's column)
  PhCallPool pool;              // PhLabeledSet, handed out by ph_handle_set_acquire's policy
  PhResidentMemo resident;      // under pool.mutex
};

// ------------------------------------------------------------------ construction

// head[0] = listed, the first NONE position of skeys [n]; head[1], head[2] = the smallest and the largest key (preset
// to NONE and 0: nothing listed)
__global__ __launch_bounds__(256) void ph_attr_head_kernel(const uint32_t *skeys, uint32_t n, uint32_t *head) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p <= n; p += (uint64_t)gridDim.x * 256u) {
    const bool none = p == n || skeys[p] == PHNSW_ATTR_NONE;
    const bool none_before = p > 0 && skeys[p - 1u] == PHNSW_ATTR_NONE;
    if (none && !none_before) {
      head[0] = (uint32_t)p;
      if (p > 0) head[1] = skeys[0], head[2] = skeys[p - 1u];
    }
  }
}

// ------------------------------------------------------------------ a call: spans, grouping, the scan

struct PhRangedArgs {
  PhDistArgs dist;
  const float *queries;  // [nq][ldq] or nullptr
  uint32_t ldq;
  const uint32_t *qids, *exclude, *lo, *hi;  // [nq]; qids, exclude nullable
  const uint32_t *list;                      // nullable: the subset form -- lookup position p is query list[p]
  uint32_t nq, n, k, slices;
  const uint32_t *skeys, *ids;  // the sorted column
  uint32_t listed;
  // the grouping (range_plan.h), by lookup position: key and iota feed the sort; order = the query of a position
  uint32_t *key, *iota, *order, *at, *len;
  const uint32_t *sorted;  // [nq] by position of the sorted batch: its lookup position
  uint32_t pq_lds;         // bytes of dynamic LDS in front of the scan's own: a PQ store's table
  uint64_t *scratch;       // slices > 1: [nq lookup positions][slices][k] keys, each list ascending, KEY_NONE padded
  uint32_t *out_ids;       // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
};

__global__ __launch_bounds__(256) void ph_ranged_lookup_kernel(PhRangedArgs a) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < a.nq; p += (uint64_t)gridDim.x * 256u) {
    const uint32_t q = ph_label_seed(a.list, (uint32_t)p);
    const bool bad_query = !a.queries && a.qids[q] >= a.n;
    uint32_t at = 0u, len = 0u;
    if (!bad_query) ph_range_span(a.skeys, a.listed, a.lo[q], a.hi[q], &at, &len);  // at + len <= listed
    a.order[p] = q, a.at[p] = at, a.len[p] = len;
    a.key[p] = ph_range_sort_key(at, len), a.iota[p] = (uint32_t)p;
  }
}

__global__ __launch_bounds__(256) void ph_ranged_count_kernel(const uint32_t *skeys, uint32_t listed, const uint32_t *lo,
                                                              const uint32_t *hi, uint64_t nq, uint32_t *out_count) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * 256u)
    out_count[q] = ph_range_count(skeys, listed, lo[q], hi[q]);
}

// One wave64 per (position of the sorted batch, slice of its span); work item = slice * nq + position (slice-major,
// the positions by span start): the waves resident together read neighbouring rows.  What a wave leaves is addressed by
// the LOOKUP position, which the merge walks.
template <class Dist>
__global__ __launch_bounds__(64) void ph_ranged_scan_kernel(PhRangedArgs a) {
  extern __shared__ float ranged_lds[];
  const uint32_t lane = threadIdx.x;
  uint64_t *const keys = (uint64_t *)((char *)ranged_lds + a.pq_lds);
  const uint64_t items = (uint64_t)a.nq * a.slices;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t pos = (uint32_t)(item % a.nq), slice = (uint32_t)(item / a.nq);
    const uint32_t p = min(a.sorted[pos], a.nq - 1u);  // (the sort's value: a lookup position)
    const uint32_t q = a.order[p];
    __syncthreads();  // the previous item's LDS (table, lists) is done with
    const bool bad_query = !a.queries && a.qids[q] >= a.n;
    Dist dist;
    if (a.queries)
      dist.prepare_raw(a.dist, a.queries + (uint64_t)q * a.ldq, ranged_lds, lane);
    else if (!bad_query)
      dist.prepare_stored(a.dist, a.qids[q], ranged_lds, lane);
    const uint32_t at = a.at[p], len = a.len[p];  // a bad query's span is empty
    ph_list_scan<false>(a, dist, keys, a.ids + at, len, q, p, slice, bad_query, lane);  // list_scan.h
  }
}

typedef void (*PhRangedFn)(PhRangedArgs);
template <template <int, int> class D>
static PhRangedFn ranged_rows_fn(uint32_t nv4) {
  switch (ph_chunk_count(nv4)) {
    case 1: return ph_ranged_scan_kernel<D<1, 4>>;
    case 3: return ph_ranged_scan_kernel<D<3, 4>>;
    case 6: return ph_ranged_scan_kernel<D<6, 4>>;
    default: return nullptr;
  }
}
static PhRangedFn ranged_scan_fn(const phnsw_store *s) {
  switch (s->kind) {
    case PH_ROWS_PQ: return ph_ranged_scan_kernel<DistPQ>;
    case PH_ROWS_F16: return ranged_rows_fn<DistF16>(s->ld / 4);
    case PH_ROWS_I8: return ranged_rows_fn<DistI8>(s->ld / 4);
    case PH_ROWS_I8Q: return ranged_rows_fn<DistI8Q>(s->ld / 4);
    default: return ranged_rows_fn<DistF32>(s->ld / 4);
  }
}

int ph_attr_fresh(const phnsw_index *ix, const phnsw_attr *at, const char *call) {
  return ph_snapshot_fresh(ix, at != nullptr, at ? at->ix : nullptr, at ? at->n : 0u, at ? at->n_nodes : 0u, "attribute keys", call);
}

// index, k, handle, store: ph_labeled_check's checks in its order
int ph_ranged_check(const phnsw_index *ix, const phnsw_attr *at, uint64_t k, const char *call) {
  if (ix) PH_TRY(ph_bits_unsupported(ix->store, call));  // a bits store has the plain walk alone
  if (!ix || ix->layers.empty()) {
    ph_set_error("%s: null index or index without layers", call);
    return PHNSW_E_INVALID;
  }
  if (!ph_exact_k_valid(k)) {
    ph_set_error("%s: k must be 1..1024 (got %llu)", call, (unsigned long long)k);
    return PHNSW_E_INVALID;
  }
  PH_TRY(ph_attr_fresh(ix, at, call));
  if (ph_store_pq_shared(ix->store)) {  // as for the distance batch, whose arithmetic the scan runs
    ph_set_error("%s: not supported over a shared-codebook PQ store; use its reconstruction store", call);
    return PHNSW_E_UNSUPPORTED;
  }
  return ph_exact_supported(ix, (uint32_t)k);  // the row length, a PQ table beside the scan's LDS
}

const uint32_t *ph_attr_column(const phnsw_attr *at) { return at->attr_of; }

PhListView ph_attr_view(const phnsw_attr *at) {
  phnsw_attr *m = const_cast<phnsw_attr *>(at);
  PhListView v = {};
  v.dev.skeys = at->skeys, v.dev.listed = (uint32_t)at->listed;
  v.dev.ids = at->ids, v.longest = at->listed, v.pool = &m->pool, v.resident = &m->resident;
  return v;
}

namespace {

// the orchestration on a set the caller holds; c is checked, 0 < nq <= PH_LABEL_NQ_MAX (with a list: its length).
// Enqueues and returns.
int ranged_run(const phnsw_index *ix, const phnsw_attr *at, const PhRangedCall &c, PhLabeledSet &set) {
  const phnsw_store *s = ix->store;
  const uint64_t nq = c.nq;
  const PhRangePre lay = ph_range_pre(nq);
  PH_TRY(set.ready());
  PH_TRY(set.block_ensure(&set.pre, &set.pre_bytes, (size_t)lay.words * 4u, c.stream));
  uint32_t *const pre = (uint32_t *)set.pre;
  PhRangedArgs a = {};
  a.dist = ph_dist_args(s);
  a.queries = c.queries, a.ldq = c.ldq, a.qids = c.qids, a.exclude = c.exclude, a.lo = c.lo, a.hi = c.hi, a.list = c.list;
  a.nq = (uint32_t)nq, a.n = (uint32_t)s->n, a.k = c.k;
  a.skeys = at->skeys, a.ids = at->ids, a.listed = (uint32_t)at->listed;
  a.key = pre + lay.key, a.iota = pre + lay.iota, a.order = pre + lay.query, a.at = pre + lay.at, a.len = pre + lay.len;
  uint32_t *const skey = pre + lay.skey, *const sorted = pre + lay.sorted;
  a.sorted = sorted;
  a.out_ids = c.out_ids, a.out_d = c.out_d, a.out_len = c.out_len, a.status = c.status;

  // before anything is enqueued: the kernel with its dynamic LDS, the slice count from the waves of it the device
  // holds -- `listed` is the longest span a call can ask for; nothing is read back --, hipCUB's temporaries
  const size_t pq_lds = (ph_pq_lds_bytes(s) + 15u) & ~(size_t)15u;
  const PhRangedFn fn = ranged_scan_fn(s);
  const size_t lds = pq_lds + (size_t)ph_label_scan_lds(a.k);
  a.pq_lds = (uint32_t)pq_lds;
  phnsw_attr *mat = const_cast<phnsw_attr *>(at);
  uint64_t resident = 0;
  PH_TRY(ph_resident_waves(mat->resident, mat->pool.mutex, s->device, (const void *)fn, lds, &resident));
  a.slices = ph_label_slice_count(nq, resident, at->listed, env_ll("PHNSW_RANGE_SLICES"));
  if (set.tmp_nq != nq) {
    size_t sort_bytes = 0;
    PH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, a.key, skey, a.iota, sorted, (int)nq, 0, 32, c.stream));
    set.tmp_need = std::max<size_t>(sort_bytes, 16), set.tmp_nq = nq;
  }
  PH_TRY(set.block_ensure(&set.tmp, &set.tmp_bytes, set.tmp_need, c.stream));
  if (a.slices > 1u) {
    uint64_t bytes = 0;
    if (!ph_label_key_bytes(nq, a.slices, c.k, &bytes)) {
      ph_set_error("exact ranged search: %llu queries in %u slices at k = %u need more scratch than can be addressed",
                   (unsigned long long)nq, a.slices, c.k);
      return PHNSW_E_INVALID;
    }
    PH_TRY(set.block_ensure(&set.keys, &set.keys_bytes, (size_t)bytes, c.stream));
    a.scratch = (uint64_t *)set.keys;
  }

  hipLaunchKernelGGL(ph_ranged_lookup_kernel, dim3(grid1(nq)), dim3(256), 0, c.stream, a);
  PH_HIP(hipGetLastError());
  size_t bytes = set.tmp_bytes;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(set.tmp, bytes, a.key, skey, a.iota, sorted, (int)nq, 0, 32, c.stream));
  const uint64_t items = nq * (uint64_t)a.slices;
  hipLaunchKernelGGL(fn, dim3((uint32_t)std::min<uint64_t>(items, 1u << 20)), dim3(64), lds, c.stream, a);
  PH_HIP(hipGetLastError());
  if (a.slices > 1u) {
    hipLaunchKernelGGL(ph_list_merge_kernel<PhRangedArgs>, dim3((uint32_t)std::min<uint64_t>(nq, 1u << 20)), dim3(64),
                       (size_t)ph_label_scan_lds(c.k), c.stream, a);
    PH_HIP(hipGetLastError());
  }
  return 0;
}

void attr_free(phnsw_attr *at) {
  ph_handle_sets_free(at->pool);
  if (at->skeys) hipFree(at->skeys);
  if (at->ids) hipFree(at->ids);
  if (at->attr_of) hipFree(at->attr_of);
  delete at;
}

// the sorted column of keys_dev [n] on `stream`; synchronises it
int attr_build(const phnsw_index *ix, const uint32_t *keys_dev, uint64_t n, hipStream_t stream, const char *call, phnsw_attr **out) {
  const phnsw_store *s = ix->store;
  phnsw_attr *at = new phnsw_attr();
  at->ix = ix, at->n = n, at->n_nodes = ix->layers.back().n_nodes, at->device = s->device;
  struct Drop {
    phnsw_attr *at;
    ~Drop() {
      if (at) attr_free(at);
    }
  } drop{at};
  if (n == 0) {
    PH_HIP(hipMalloc(&at->attr_of, 4));  // never null: a null column would read as "no range filter"
    PH_HIP(hipMemsetAsync(at->attr_of, 0xFF, 4, stream));
    PH_HIP(hipMalloc(&at->skeys, 4));
    PH_HIP(hipMalloc(&at->ids, 4));
    PH_HIP(hipStreamSynchronize(stream));
    *out = at, drop.at = nullptr;
    return 0;
  }
  uint32_t n_nodes;
  const uint32_t *nodes, *vec2node;
  ph_exact_bottom_layer(ix, &n_nodes, &nodes, &vec2node);
  HostBlocks hb{stream, {}};
  uint32_t *iota = nullptr, *head = nullptr;
  void *tmp = nullptr;
  PH_HIP(hipMalloc(&at->attr_of, (size_t)n * 4u));  // the sort's keys, which it leaves as they are: kept
  PH_HIP(hipMalloc(&at->skeys, (size_t)n * 4u));
  PH_HIP(hipMalloc(&at->ids, (size_t)n * 4u));
  PH_TRY(hb.alloc(&iota, (size_t)n * 4u));
  PH_TRY(hb.alloc(&head, 16));
  size_t tmp_bytes = 0;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, at->attr_of, at->skeys, iota, at->ids, (int)n, 0, 32, stream));
  tmp_bytes = std::max<size_t>(tmp_bytes, 16);
  PH_TRY(hb.alloc(&tmp, tmp_bytes));
  hipLaunchKernelGGL(ph_label_key_kernel, dim3(grid1(n)), dim3(256), 0, stream, keys_dev, (uint32_t)n, n_nodes, nodes, vec2node,
                     at->attr_of, iota);
  PH_HIP(hipGetLastError());
  size_t bytes = tmp_bytes;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, at->attr_of, at->skeys, iota, at->ids, (int)n, 0, 32, stream));
  PH_HIP(hipMemsetAsync(head, 0, 16, stream));
  PH_HIP(hipMemsetAsync(head + 1, 0xFF, 4, stream));  // the smallest key of nothing
  hipLaunchKernelGGL(ph_attr_head_kernel, dim3(grid1(n + 1u)), dim3(256), 0, stream, at->skeys, (uint32_t)n, head);
  PH_HIP(hipGetLastError());
  uint32_t h[4] = {0, 0, 0, 0};
  PH_HIP(hipMemcpyAsync(h, head, 16, hipMemcpyDeviceToHost, stream));
  PH_HIP(hipStreamSynchronize(stream));
  at->listed = h[0], at->key_min = h[1], at->key_max = h[2];
  if (at->listed > n) {
    ph_set_error("%s: the keys changed while the column was sorted", call);
    return PHNSW_E_INVALID;
  }
  *out = at, drop.at = nullptr;
  return 0;
}

int attr_create_check(const phnsw_index *ix, const void *keys, uint64_t n, phnsw_attr **out, const char *call) {
  if (!ix || ix->layers.empty()) {
    ph_set_error("%s: null index or index without layers", call);
    return PHNSW_E_INVALID;
  }
  if (!out || (!keys && n)) {
    ph_set_error("%s: null keys or null output", call);
    return PHNSW_E_INVALID;
  }
  if (n != ix->store->n) {
    ph_set_error("%s: %llu keys for a store of %llu vectors (one key per vector)", call, (unsigned long long)n,
                 (unsigned long long)ix->store->n);
    return PHNSW_E_INVALID;
  }
  return 0;
}

// what both forms of the walk check before they look at a pointer: index and parameters, the handle, the flags
int walk_check(const phnsw_index *ix, const phnsw_attr *at, const phnsw_search_params *sp, uint32_t flags, const char *call) {
  if (ix) PH_TRY(ph_bits_unsupported(ix->store, call));  // a bits store has the plain walk alone
  PH_TRY(ph_check_sp(ix, sp));
  PH_TRY(ph_attr_fresh(ix, at, call));
  if (flags & ~(uint32_t)PHNSW_FILTER_STRICT) {
    ph_set_error("%s: unknown flag bits 0x%x", call, flags);
    return PHNSW_E_INVALID;
  }
  return 0;
}

}  // namespace

int ph_attr_count(const phnsw_attr *at, const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t nq, uint32_t *out_count_dev,
                  hipStream_t stream) {
  hipLaunchKernelGGL(ph_ranged_count_kernel, dim3(grid1(nq)), dim3(256), 0, stream, at->skeys, (uint32_t)at->listed, lo_dev, hi_dev,
                     nq, out_count_dev);
  PH_HIP(hipGetLastError());
  return 0;
}

int ph_ranged_device(const phnsw_index *ix, const phnsw_attr *at, const PhRangedCall &c) {
  if (c.nq == 0) return 0;
  phnsw_attr *mat = const_cast<phnsw_attr *>(at);
  PhLabeledSet *set = ph_handle_set_acquire(mat->pool, c.stream, false);
  PhSetGuard guard{mat->pool, set, c.stream};
  return ranged_run(ix, at, c, *set);
}

// ------------------------------------------------------------------ C ABI: the handle

extern "C" int phnsw_attr_create_device(const phnsw_index *ix, const uint32_t *keys_dev, uint64_t n, void *stream,
                                        phnsw_attr **out) try {
  const char *const call = "phnsw_attr_create_device";
  PH_TRY(attr_create_check(ix, keys_dev, n, out, call));
  PH_HIP(hipSetDevice(ix->store->device));
  return attr_build(ix, keys_dev, n, (hipStream_t)stream, call, out);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_attr_create(const phnsw_index *ix, const uint32_t *keys, uint64_t n, phnsw_attr **out) try {
  const char *const call = "phnsw_attr_create";
  PH_TRY(attr_create_check(ix, keys, n, out, call));
  PH_HIP(hipSetDevice(ix->store->device));
  HostBlocks hb{nullptr, {}};
  uint32_t *dev = nullptr;
  PH_TRY(hb.alloc(&dev, (size_t)n * 4u));
  if (n) PH_HIP(hipMemcpy(dev, keys, (size_t)n * 4u, hipMemcpyHostToDevice));
  return attr_build(ix, dev, n, nullptr, call, out);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_attr_info(const phnsw_attr *at, uint64_t *n, uint64_t *listed, uint32_t *key_min, uint32_t *key_max) try {
  if (!at) {
    ph_set_error("phnsw_attr_info: null attribute keys");
    return PHNSW_E_INVALID;
  }
  if (n) *n = at->n;
  if (listed) *listed = at->listed;
  if (key_min) *key_min = at->key_min;
  if (key_max) *key_max = at->key_max;
  return 0;
} catch (...) { return ph_caught(); }

extern "C" int phnsw_attr_count_device(const phnsw_attr *at, const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t nq,
                                       uint32_t *out_count_dev, void *stream) try {
  const char *const call = "phnsw_attr_count_device";
  if (!at) {
    ph_set_error("%s: null attribute keys", call);
    return PHNSW_E_INVALID;
  }
  if (nq == 0) return 0;
  if (!lo_dev || !hi_dev || !out_count_dev) {
    ph_set_error("%s: null lo, null hi or null output", call);
    return PHNSW_E_INVALID;
  }
  PH_HIP(hipSetDevice(at->device));
  return ph_attr_count(at, lo_dev, hi_dev, nq, out_count_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" void phnsw_attr_destroy(phnsw_attr *at) {
  if (!at) return;
  try {
    hipSetDevice(at->device);
    attr_free(at);  // waits for the events that close the calls in flight
  } catch (...) {
  }
}

// ------------------------------------------------------------------ C ABI: exact top-k over a range

extern "C" int phnsw_search_exact_ranged_device(const phnsw_index *ix, const phnsw_attr *at, const float *queries_dev, uint32_t ldq,
                                                const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                                const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t k, uint32_t *out_ids_dev,
                                                float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev, void *stream) try {
  const char *const call = "phnsw_search_exact_ranged_device";
  PH_TRY(ph_ranged_check(ix, at, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !lo_dev || !hi_dev || nq > PH_LABEL_NQ_MAX) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; lo and hi; nq < 2^31 - 1; queries need ldq >= "
                 "store ld, multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhRangedCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.lo = lo_dev, c.hi = hi_dev, c.nq = nq;
  c.k = (uint32_t)k;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_ranged_device(ix, at, c);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_ranged(const phnsw_index *ix, const phnsw_attr *at, const float *queries, const uint64_t *qids,
                                         uint64_t nq, const uint64_t *exclude, const uint32_t *lo, const uint32_t *hi, uint64_t k,
                                         uint64_t *out_ids, float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_search_exact_ranged";
  PH_TRY(ph_ranged_check(ix, at, k, call));
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!out_ids || !out_d || !out_len || !lo || !hi || nq > PH_LABEL_NQ_MAX) {
    ph_set_error("%s: invalid argument (outputs; lo and hi; nq < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, call));
  phnsw_attr *mat = const_cast<phnsw_attr *>(at);
  PhLabeledSet *set = ph_handle_set_acquire(mat->pool, nullptr, true);
  PhHostCall h(mat->pool, set);
  PH_TRY(h.stage_in(s, queries, qids, exclude, nq, (size_t)nq * 2u, 0, (uint32_t)k, (uint32_t)k));  // extras: lo | hi
  PhRangedCall c = {};
  h.fill(c);
  uint32_t *const lo_dev = h.extra(), *const hi_dev = lo_dev + nq;
  PH_HIP(hipMemcpyAsync(lo_dev, lo, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
  PH_HIP(hipMemcpyAsync(hi_dev, hi, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
  c.lo = lo_dev, c.hi = hi_dev, c.k = (uint32_t)k;
  PH_TRY(ranged_run(ix, at, c, *set));
  return h.finish(out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }

// ------------------------------------------------------------------ the graph walk by range

extern "C" int phnsw_search_batch_ranged_device(const phnsw_index *ix, const phnsw_attr *at, const float *queries_dev, uint32_t ldq,
                                                const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                                uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *lo_dev,
                                                const uint32_t *hi_dev, uint32_t flags, uint32_t *out_ids_dev, float *out_d_dev,
                                                uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev,
                                                void *stream) try {
  const char *const call = "phnsw_search_batch_ranged_device";
  PH_TRY(walk_check(ix, at, sp, flags, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !lo_dev || !hi_dev || nq > 0xFFFFFFFFull) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; lo and hi; queries need ldq >= store ld, "
                 "multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhSearchCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq;
  c.sp = sp, c.upto = upto_layers;
  c.filter.attr_of = at->attr_of, c.filter.range_lo = lo_dev, c.filter.range_hi = hi_dev, c.filter.flags = flags;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.status = status_dev, c.out_stats = out_stats_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_search_device(ix, c);
} catch (...) { return ph_caught(); }

// The host form stages everything once, on the stream of a scratch set of the handle, as phnsw_search_batch_labeled does.
extern "C" int phnsw_search_batch_ranged(const phnsw_index *ix, const phnsw_attr *at, const float *queries, const uint64_t *qids,
                                         uint64_t nq, const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude,
                                         const uint32_t *lo, const uint32_t *hi, uint32_t flags, uint64_t k, uint64_t *out_ids,
                                         float *out_d, uint64_t *out_len, uint64_t *out_stats) try {
  const char *const call = "phnsw_search_batch_ranged";
  PH_TRY(walk_check(ix, at, sp, flags, call));
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
  if (!out_ids || !out_d || !out_len || !lo || !hi || nq > 0xFFFFFFFFull) {
    ph_set_error("%s: invalid argument (outputs; lo and hi; nq < 2^32)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, call));
  phnsw_attr *mat = const_cast<phnsw_attr *>(at);
  PhLabeledSet *set = ph_handle_set_acquire(mat->pool, nullptr, true);
  PhHostCall h(mat->pool, set);
  // extras: stats(2), which the host reads back with len and status | lo | hi | the redo list
  PH_TRY(h.stage_in(s, queries, qids, exclude, nq, (size_t)nq * 5u, 2, ef, k ? (uint32_t)k : ef));
  uint32_t *const lo_dev = h.extra() + 2u * nq, *const hi_dev = lo_dev + nq, *const redo_dev = hi_dev + nq;
  PhSearchCall c = {};
  h.fill(c);
  PH_HIP(hipMemcpyAsync(lo_dev, lo, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
  PH_HIP(hipMemcpyAsync(hi_dev, hi, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
  c.filter.attr_of = at->attr_of, c.filter.range_lo = lo_dev, c.filter.range_hi = hi_dev, c.filter.flags = flags;
  c.sp = sp, c.upto = upto_layers, c.out_stats = h.extra();
  return ph_walk_host_run(ix, h, c, redo_dev, ef, out_ids, out_d, out_len, out_stats);
} catch (...) { return ph_caught(); }
