// Exact radius search over a LIST of row ids per query (phnsw_search_exact_radius_labeled[_device],
// phnsw_search_exact_radius_ranged[_device]): every listed row of the query's label -- or of the query's key range --
// closer to the query than the query's radius, as the CSR result of phnsw_search_exact_radius.  It joins two things the
// library has: the lists of a handle (a label's posting list, a range's span of the sorted column: both ids + at, len;
// PhListView, phnsw_internal.h) scanned as list_scan.h scans them, and the tail of the radius call (radius_tail.h).
//
//   1. ph_list_radius_lookup_{labels,range}_kernel   per query the list (at, len) -- empty for PHNSW_LABEL_NONE, a label
//                                  nobody carries, lo > hi and a Stored query id at or past n --, the sort key
//                                  (ph_range_sort_key: the list's start) and refuse[q] = 0 or 4; radix sort of (key, query)
//   2. ph_radius_init_kernel       count[q] = 0, the cursor = 0, status[q] = refuse[q]
//   3. ph_list_radius_scan_kernel  one wave64 per (position of the sorted batch, slice of its list), slice-major: 64 ids
//                                  at a time into dist.batch of the store's policy, in = ok && id != exclude && d < r, a
//                                  ballot, the hits as keys into the wave's LDS buffer; the buffer is flushed -- ONE atomic
//                                  add on the 64-bit cursor, then coalesced stores of (key, query) records -- when the next
//                                  batch would not fit and at the end of the item (list_radius_plan.h).  One pass: a
//                                  distance costs a row read from HBM here, and counting first would read every row twice.
//                                  count[q] gets one atomic add per item (the slices of a query run in different waves);
//                                  records at or past the pool's capacity are dropped but counted.  A query whose radius is
//                                  NaN, zero or negative, or whose list is empty, reads no row at all
//   4. the tail (radius_tail.h): exclusive sum, the total's read-back, two radix passes, the unpack
//
// The pool's order depends on scheduling; the sorted order does not, because the keys of one query are distinct.  So the
// result is one whatever the slice count.  Nothing is read back before step 4: the pool is sized from what the handle
// knows on the host (list_radius_plan.h).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "host_call.h"
#include "list_radius_plan.h"
#include "list_scan.h"
#include "phnsw_device.h"
#include "radius_tail.h"
#include "range_plan.h"

struct PhListRadiusArgs {
  PhDistArgs dist;
  const float *queries;  // [nq][ldq] or nullptr
  uint32_t ldq;
  const uint32_t *qids, *exclude;  // [nq]; nullable
  const uint32_t *want, *lo, *hi;  // [nq]: the label, or the bounds
  const float *radius;             // [nq]
  uint32_t nq, n, slices;
  PhListArrays view;  // the handle's device arrays
  // by query: key (the sort key), iota (the query itself, the sort's value), at and len (its list), refuse
  uint32_t *key, *iota, *at, *len, *refuse;
  const uint32_t *sorted;  // [nq] by position of the sorted batch: its query
  uint32_t pq_lds;         // bytes of dynamic LDS in front of the staging buffer: a PQ store's table
  unsigned long long *cursor;  // records reserved so far, dropped ones included
  uint32_t *count;             // [nq + 1]
  uint64_t *keys;              // [records]
  uint32_t *qs;                // [records]
  uint64_t records;            // 0: count only
};

__device__ __forceinline__ void ph_list_radius_lookup_finish(const PhListRadiusArgs &a, uint32_t q, bool bad_query, uint32_t at,
                                                             uint32_t len) {
  a.at[q] = at, a.len[q] = len, a.refuse[q] = bad_query ? ST_MISSING : ST_OK;
  a.key[q] = ph_range_sort_key(at, len), a.iota[q] = q;
}

__global__ __launch_bounds__(256) void ph_list_radius_lookup_labels_kernel(PhListRadiusArgs a) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < a.nq; p += (uint64_t)gridDim.x * 256u) {
    const uint32_t q = (uint32_t)p;
    const bool bad_query = !a.queries && a.qids[q] >= a.n;
    const uint32_t s = bad_query ? PH_LABEL_SLOT_NONE : ph_label_slot(a.view.values, a.view.nlabels, a.want[q], PHNSW_LABEL_NONE);
    uint32_t at = 0u, len = 0u;
    if (s != PH_LABEL_SLOT_NONE) {
      at = a.view.first[s];
      len = a.view.first[s + 1u] - at;
      if (at > a.view.listed || len > a.view.listed - at) at = 0u, len = 0u;  // (first is ascending and ends at listed)
    }
    ph_list_radius_lookup_finish(a, q, bad_query, len ? at : 0u, len);
  }
}

__global__ __launch_bounds__(256) void ph_list_radius_lookup_range_kernel(PhListRadiusArgs a) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < a.nq; p += (uint64_t)gridDim.x * 256u) {
    const uint32_t q = (uint32_t)p;
    const bool bad_query = !a.queries && a.qids[q] >= a.n;
    uint32_t at = 0u, len = 0u;
    if (!bad_query) ph_range_span(a.view.skeys, a.view.listed, a.lo[q], a.hi[q], &at, &len);  // at + len <= listed
    ph_list_radius_lookup_finish(a, q, bad_query, at, len);
  }
}

// the wave's staged keys into the pool: one atomic add for all of them, then coalesced stores; uniform over the wave
__device__ __forceinline__ void ph_list_radius_flush(const PhListRadiusArgs &a, const uint64_t *stage, uint32_t staged, uint32_t q,
                                                     uint32_t lane) {
  unsigned long long base = 0ull;
  if (lane == 0) base = atomicAdd(a.cursor, (unsigned long long)staged);
  base = rl64(base, 0);
  __syncthreads();  // the staged keys are there
  for (uint32_t i = lane; i < staged; i += 64u) {
    const uint64_t slot = base + i;
    if (slot < a.records) a.keys[slot] = stage[i], a.qs[slot] = q;
  }
  __syncthreads();  // ... and taken: the buffer is free
}

// One wave64 per (position of the sorted batch, slice of its list); work item = slice * nq + position (slice-major, the
// positions by list start: ph_ranged_scan_kernel's order).  Everything that decides a branch is uniform over the wave.
template <class Dist>
__global__ __launch_bounds__(64) void ph_list_radius_scan_kernel(PhListRadiusArgs a) {
  extern __shared__ float list_radius_lds[];
  const uint32_t lane = threadIdx.x;
  uint64_t *const stage = (uint64_t *)((char *)list_radius_lds + a.pq_lds);  // [PH_LIST_RADIUS_STAGE]
  const uint64_t items = (uint64_t)a.nq * a.slices;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t pos = (uint32_t)(item % a.nq), slice = (uint32_t)(item / a.nq);
    const uint32_t q = min(a.sorted[pos], a.nq - 1u);  // (the sort's value: a query)
    const float r = a.radius[q];
    const uint32_t at = a.at[q], len = a.len[q];  // a bad query's list is empty; at + len <= listed
    if (!(r > 0.0f) || !len) continue;  // the contract: a zero, negative or NaN radius matches nothing and reads no row
    uint64_t b0, b1;
    ph_label_slice_range(slice, a.slices, len, &b0, &b1);
    if (b0 >= b1) continue;
    __syncthreads();  // the previous item's LDS (a PQ table) is done with
    Dist dist;
    if (a.queries)
      dist.prepare_raw(a.dist, a.queries + (uint64_t)q * a.ldq, list_radius_lds, lane);
    else
      dist.prepare_stored(a.dist, a.qids[q], list_radius_lds, lane);
    const uint32_t ex = a.exclude ? a.exclude[q] : PH_EMPTY32;
    const uint32_t *const list = a.view.ids + at;
    uint32_t staged = 0, cnt = 0;
    for (uint64_t b = b0; b < b1; b++) {
      const uint32_t j = (uint32_t)b * PH_LABEL_BATCH + lane;
      const bool ok = j < len;
      const uint32_t id = ok ? list[j] : 0u;  // a listed id: a row of the store
      const float d = dist.batch(a.dist, __ballot(ok), id, lane);
      const bool in = ok && id != ex && d < r;
      const uint64_t m = __ballot(in);
      const uint32_t hits = (uint32_t)__popcll(m);
      cnt += hits;
      if (!a.records || !hits) continue;
      if (ph_list_radius_flush_first(staged, hits)) {
        ph_list_radius_flush(a, stage, staged, q, lane);
        staged = 0;
      }
      if (in) stage[staged + (uint32_t)__popcll(m & lanemask_lt(lane))] = mkkey(d, id);  // < staged + hits <= the buffer
      staged += hits;
    }
    if (!cnt) continue;
    if (staged) ph_list_radius_flush(a, stage, staged, q, lane);
    if (lane == 0) {
      if (!a.records) atomicAdd(a.cursor, (unsigned long long)cnt);  // count only: nothing was flushed
      atomicAdd(a.count + q, cnt);
    }
  }
}

typedef void (*PhListRadiusFn)(PhListRadiusArgs);
template <template <int, int> class D>
static PhListRadiusFn list_radius_rows_fn(uint32_t nv4) {
  switch (ph_chunk_count(nv4)) {
    case 1: return ph_list_radius_scan_kernel<D<1, 4>>;
    case 3: return ph_list_radius_scan_kernel<D<3, 4>>;
    case 6: return ph_list_radius_scan_kernel<D<6, 4>>;
    default: return nullptr;
  }
}
static PhListRadiusFn list_radius_scan_fn(const phnsw_store *s) {
  switch (s->kind) {
    case PH_ROWS_PQ: return ph_list_radius_scan_kernel<DistPQ>;
    case PH_ROWS_F16: return list_radius_rows_fn<DistF16>(s->ld / 4);
    case PH_ROWS_I8: return list_radius_rows_fn<DistI8>(s->ld / 4);
    case PH_ROWS_I8Q: return list_radius_rows_fn<DistI8Q>(s->ld / 4);
    default: return list_radius_rows_fn<DistF32>(s->ld / 4);
  }
}

namespace {

// the request, checked; device pointers of the caller.  labels: by label (want); else by range (lo and hi)
struct PhListRadiusCall {
  bool labels;
  const float *queries;  // [nq][ldq], or nullptr: Stored queries (qids)
  uint32_t ldq;
  const uint32_t *qids, *exclude;  // [nq] or nullptr
  const uint32_t *want, *lo, *hi;  // [nq]
  uint64_t nq;
  const float *radius;  // [nq]
  uint64_t cap;
  uint64_t *out_first;  // [nq + 1]
  uint32_t *status;     // [nq]
  uint64_t *out_total;  // nullable
  bool total_to_host;   // read the total back even when cap == 0
  long long forced_slices;  // PHNSW_LABEL_SLICES / PHNSW_RANGE_SLICES
  hipStream_t stream;
};

// Steps 1 to 4 without the unpack, on a set the caller holds: *total and *sorted as ph_radius_tail leaves them
int list_radius_run(const phnsw_index *ix, const PhListView &view, const PhListRadiusCall &c, PhLabeledSet &set, uint64_t *total,
                    const uint64_t **sorted) {
  const phnsw_store *s = ix->store;
  const uint64_t nq = c.nq;
  *total = 0, *sorted = nullptr;
  PH_TRY(set.ready());
  if (!set.h_total) PH_HIP(hipHostMalloc((void **)&set.h_total, 8u, hipHostMallocDefault));
  const PhRangePre pre_lay = ph_range_pre(nq);  // key, iota, query (here: refuse), at, len, skey, sorted
  PH_TRY(set.block_ensure(&set.pre, &set.pre_bytes, (size_t)pre_lay.words * 4u, c.stream));
  uint32_t *const pre = (uint32_t *)set.pre;
  const uint64_t records = ph_list_radius_pool_records(c.cap, nq, view.longest);
  const PhRadiusLayout lay = ph_list_radius_layout(nq, records);
  PH_TRY(set.block_ensure(&set.post, &set.post_bytes, (size_t)lay.bytes, c.stream));
  char *const post = (char *)set.post;

  PhListRadiusArgs a = {};
  a.dist = ph_dist_args(s);
  a.queries = c.queries, a.ldq = c.ldq, a.qids = c.qids, a.exclude = c.exclude, a.want = c.want, a.lo = c.lo, a.hi = c.hi;
  a.radius = c.radius, a.nq = (uint32_t)nq, a.n = (uint32_t)s->n, a.view = view.dev;
  a.key = pre + pre_lay.key, a.iota = pre + pre_lay.iota, a.refuse = pre + pre_lay.query, a.at = pre + pre_lay.at;
  a.len = pre + pre_lay.len;
  uint32_t *const skey = pre + pre_lay.skey, *const sorted_q = pre + pre_lay.sorted;
  a.sorted = sorted_q;
  a.cursor = (unsigned long long *)(post + lay.head), a.count = (uint32_t *)(post + lay.count);
  a.keys = (uint64_t *)(post + lay.keys_a), a.qs = (uint32_t *)(post + lay.q_a), a.records = records;

  // before anything is enqueued: the kernel with its dynamic LDS, the slice count from the waves of it the device holds
  // and the longest list the handle can have, hipCUB's temporaries for the batch's sort
  const size_t pq_lds = (ph_pq_lds_bytes(s) + 15u) & ~(size_t)15u;
  const PhListRadiusFn fn = list_radius_scan_fn(s);
  const size_t lds = pq_lds + (size_t)PH_LIST_RADIUS_STAGE * 8u;
  a.pq_lds = (uint32_t)pq_lds;
  uint64_t resident = 0;
  PH_TRY(ph_resident_waves(*view.resident, view.pool->mutex, s->device, (const void *)fn, lds, &resident));
  a.slices = ph_label_slice_count(nq, resident, view.longest, c.forced_slices);
  // ... and the tail's: `tmp` is sized ONCE, here, for everything the call enqueues that uses it -- a block that grew
  // in mid-call would go back to the pool with the batch's sort still queued on it (call_set.h's rule)
  PhRadiusTail t = {};
  t.nq = nq, t.cap = c.cap, t.records = records, t.cursor = a.cursor, t.count = a.count;
  t.keys_a = a.keys, t.keys_b = (uint64_t *)(post + lay.keys_b), t.qs_a = a.qs, t.qs_b = (uint32_t *)(post + lay.q_b);
  t.out_first = c.out_first, t.out_total = c.out_total, t.total_to_host = c.total_to_host;
  t.h_total = set.h_total, t.set = &set, t.tmp = &set.tmp, t.tmp_bytes = &set.tmp_bytes, t.stream = c.stream;
  size_t sort_bytes = 0;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, a.key, skey, a.iota, sorted_q, (int)nq, 0, 32, c.stream));
  PhRadiusTailSizes tail_sizes;
  PH_TRY(ph_radius_tail_sizes(t, &tail_sizes));
  PH_TRY(set.block_ensure(&set.tmp, &set.tmp_bytes, std::max(sort_bytes, tail_sizes.most()), c.stream));
  t.tmp_ready = true;

  StepTimes times;
  times.on = env_ll("PHNSW_DENSE_TIMES") > 0, times.stream = c.stream;
  times.begin(0);
  if (c.labels)
    hipLaunchKernelGGL(ph_list_radius_lookup_labels_kernel, dim3(grid1(nq)), dim3(256), 0, c.stream, a);
  else
    hipLaunchKernelGGL(ph_list_radius_lookup_range_kernel, dim3(grid1(nq)), dim3(256), 0, c.stream, a);
  PH_HIP(hipGetLastError());
  size_t bytes = sort_bytes;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(set.tmp, bytes, a.key, skey, a.iota, sorted_q, (int)nq, 0, 32, c.stream));
  hipLaunchKernelGGL(ph_radius_init_kernel, dim3(grid1(nq + 1u)), dim3(256), 0, c.stream, a.count, a.cursor, a.refuse, c.status, nq);
  PH_HIP(hipGetLastError());
  times.end();
  times.begin(1);
  const uint64_t items = nq * (uint64_t)a.slices;
  hipLaunchKernelGGL(fn, dim3((uint32_t)std::min<uint64_t>(items, 1u << 20)), dim3(64), lds, c.stream, a);
  PH_HIP(hipGetLastError());
  times.end();

  times.begin(2);
  PH_TRY(ph_radius_tail(t, total, sorted));  // the one synchronisation, when there is a pool (or the host form asks)
  times.end();
  float ms[3];
  if (times.collect(ms, 3))
    fprintf(stderr, "[phnsw] exact_radius_%s: %llu queries in %u slices, %llu in radius: lookup %.3f ms, scan %.3f ms, scan+sort %.3f ms\n",
            c.labels ? "labeled" : "ranged", (unsigned long long)nq, a.slices, (unsigned long long)*total, ms[0], ms[1], ms[1] + ms[2]);
  return 0;
}

// what every entry point checks first, in this order: the index, cap ...
int list_radius_check(const phnsw_index *ix, uint64_t cap, const char *call) {
  if (ix) PH_TRY(ph_bits_unsupported(ix->store, call));  // a bits store has the plain walk alone
  if (!ix || ix->layers.empty()) {
    ph_set_error("%s: null index or index without layers", call);
    return PHNSW_E_INVALID;
  }
  if (!ph_radius_cap_valid(cap)) {
    ph_set_error("%s: cap must be at most 2^31 - 1 (got %llu)", call, (unsigned long long)cap);
    return PHNSW_E_INVALID;
  }
  return 0;
}

// ... then, after the handle: the store, as ph_labeled_check / ph_ranged_check test it at k = 1, every message naming the call
int list_radius_store_check(const phnsw_index *ix, const char *call) {
  if (ph_store_pq_shared(ix->store)) {  // as for the distance batch, whose arithmetic the scan runs
    ph_set_error("%s: not supported over a shared-codebook PQ store; use its reconstruction store", call);
    return PHNSW_E_UNSUPPORTED;
  }
  if (const int rc = ph_exact_supported(ix, 1u)) {  // the row length, a PQ table beside the scan's LDS
    const std::string why = phnsw_last_error();
    ph_set_error("%s: %s", call, why.c_str());
    return rc;
  }
  return 0;
}

struct PhListRadiusDeviceOut {
  uint64_t *out_first;
  uint32_t *out_ids;
  float *out_d;
  uint32_t *status;
  uint64_t *out_total;
};

// the device forms after the index, cap, handle and store checks
int list_radius_device(const phnsw_index *ix, const PhListView &view, PhListRadiusCall &c, const PhListRadiusDeviceOut &o,
                       const char *call) {
  if (c.nq == 0) return 0;
  if (!ph_device_queries_ok(ix, c.queries, c.qids, c.ldq) || !c.radius || !o.out_first || !o.status || !o.out_total ||
      (c.labels ? !c.want : (!c.lo || !c.hi)) || (c.cap && (!o.out_ids || !o.out_d)) || c.nq > 0x7FFFFFFEull) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; %s; radius; out_first, status and out_total; out_ids and "
                 "out_d unless cap is 0; nq <= 2^31 - 2; queries need ldq >= store ld, multiple of 4, 16-byte base)", call,
                 c.labels ? "want" : "lo and hi");
    return PHNSW_E_INVALID;
  }
  c.out_first = o.out_first, c.status = o.status, c.out_total = o.out_total, c.total_to_host = false;
  PH_HIP(hipSetDevice(ix->store->device));
  PhLabeledSet *set = ph_handle_set_acquire(*view.pool, c.stream, false);
  PhSetGuard guard{*view.pool, set, c.stream};
  uint64_t total;
  const uint64_t *sorted;
  PH_TRY(list_radius_run(ix, view, c, *set, &total, &sorted));
  if (sorted) PH_TRY(ph_radius_unpack(sorted, total, o.out_ids, o.out_d, c.stream));
  return 0;
}

// the host forms after the index, cap, handle and store checks; filt0, filt1: want and nullptr, or lo and hi
int list_radius_host(const phnsw_index *ix, const PhListView &view, const float *queries, const uint64_t *qids, uint64_t nq,
                     const uint64_t *exclude, const uint32_t *filt0, const uint32_t *filt1, bool labels, const float *radius,
                     uint64_t cap, uint64_t *out_first, uint64_t *out_ids, float *out_d, uint64_t *out_total, long long forced,
                     const char *call) {
  if (nq == 0) {  // no query: the empty result, complete
    if (out_first) out_first[0] = 0;
    if (out_total) *out_total = 0;
    return 0;
  }
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!filt0 || (!labels && !filt1) || !radius || !out_first || !out_total || (cap && (!out_ids || !out_d)) || nq > 0x7FFFFFFEull) {
    ph_set_error("%s: invalid argument (%s; radius, out_first and out_total; out_ids and out_d unless cap is 0; nq <= 2^31 - 2)",
                 call, labels ? "want" : "lo and hi");
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, call));
  PhLabeledSet *set = ph_handle_set_acquire(*view.pool, nullptr, true);
  PhHostCall h(*view.pool, set);
  PH_TRY(h.stage_in(s, queries, qids, exclude, nq, (size_t)nq * 3u, 0, 0, 0));  // extras: the radii | want or lo | hi
  PhListRadiusCall c = {};
  c.queries = h.queries, c.ldq = h.queries ? h.ld : 0u, c.qids = h.qids, c.exclude = h.exclude, c.nq = nq;
  c.status = h.small + 3u * nq, c.stream = h.st;  // the ids were checked: every status is 0
  uint32_t *const r_dev = h.extra(), *const f0_dev = r_dev + nq, *const f1_dev = f0_dev + nq;
  PH_HIP(hipMemcpyAsync(r_dev, radius, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
  PH_HIP(hipMemcpyAsync(f0_dev, filt0, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
  if (!labels) PH_HIP(hipMemcpyAsync(f1_dev, filt1, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
  c.radius = (const float *)r_dev, c.labels = labels;
  if (labels)
    c.want = f0_dev;
  else
    c.lo = f0_dev, c.hi = f1_dev;
  c.cap = cap, c.total_to_host = true, c.forced_slices = forced;
  PH_TRY(h.blocks.alloc(&c.out_first, (size_t)(nq + 1u) * 8u));
  uint64_t total;
  const uint64_t *sorted;
  PH_TRY(list_radius_run(ix, view, c, *set, &total, &sorted));
  if (sorted) {
    uint64_t *ids = nullptr;
    float *d = nullptr;
    PH_TRY(h.blocks.alloc(&ids, (size_t)total * 8u));
    PH_TRY(h.blocks.alloc(&d, (size_t)total * 4u));
    PH_TRY(ph_radius_unpack(sorted, total, ids, d, h.st));
    PH_HIP(hipMemcpyAsync(out_ids, ids, (size_t)total * 8u, hipMemcpyDeviceToHost, h.st));
    PH_HIP(hipMemcpyAsync(out_d, d, (size_t)total * 4u, hipMemcpyDeviceToHost, h.st));
  }
  PH_HIP(hipMemcpyAsync(out_first, c.out_first, (size_t)(nq + 1u) * 8u, hipMemcpyDeviceToHost, h.st));
  PH_TRY(h.sync());
  *out_total = total;
  return 0;
}

}  // namespace

// ------------------------------------------------------------------ C ABI

extern "C" int phnsw_search_exact_radius_labeled_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev,
                                                        uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                        const uint32_t *exclude_dev, const uint32_t *want_dev,
                                                        const float *radius_dev, uint64_t cap, uint64_t *out_first_dev,
                                                        uint32_t *out_ids_dev, float *out_d_dev, uint32_t *status_dev,
                                                        uint64_t *out_total_dev, void *stream) try {
  const char *const call = "phnsw_search_exact_radius_labeled_device";
  PH_TRY(list_radius_check(ix, cap, call));
  PH_TRY(ph_labels_fresh(ix, lb, call));
  PH_TRY(list_radius_store_check(ix, call));
  PhListRadiusCall c = {};
  c.labels = true, c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.want = want_dev, c.nq = nq;
  c.radius = radius_dev, c.cap = cap, c.forced_slices = env_ll("PHNSW_LABEL_SLICES"), c.stream = (hipStream_t)stream;
  const PhListRadiusDeviceOut o = {out_first_dev, out_ids_dev, out_d_dev, status_dev, out_total_dev};
  return list_radius_device(ix, ph_labels_view(lb), c, o, call);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_radius_labeled(const phnsw_index *ix, const phnsw_labels *lb, const float *queries,
                                                 const uint64_t *qids, uint64_t nq, const uint64_t *exclude, const uint32_t *want,
                                                 const float *radius, uint64_t cap, uint64_t *out_first, uint64_t *out_ids,
                                                 float *out_d, uint64_t *out_total) try {
  const char *const call = "phnsw_search_exact_radius_labeled";
  PH_TRY(list_radius_check(ix, cap, call));
  PH_TRY(ph_labels_fresh(ix, lb, call));
  PH_TRY(list_radius_store_check(ix, call));
  return list_radius_host(ix, ph_labels_view(lb), queries, qids, nq, exclude, want, nullptr, true, radius, cap, out_first, out_ids,
                          out_d, out_total, env_ll("PHNSW_LABEL_SLICES"), call);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_radius_ranged_device(const phnsw_index *ix, const phnsw_attr *at, const float *queries_dev,
                                                       uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                       const uint32_t *exclude_dev, const uint32_t *lo_dev, const uint32_t *hi_dev,
                                                       const float *radius_dev, uint64_t cap, uint64_t *out_first_dev,
                                                       uint32_t *out_ids_dev, float *out_d_dev, uint32_t *status_dev,
                                                       uint64_t *out_total_dev, void *stream) try {
  const char *const call = "phnsw_search_exact_radius_ranged_device";
  PH_TRY(list_radius_check(ix, cap, call));
  PH_TRY(ph_attr_fresh(ix, at, call));
  PH_TRY(list_radius_store_check(ix, call));
  PhListRadiusCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.lo = lo_dev, c.hi = hi_dev, c.nq = nq;
  c.radius = radius_dev, c.cap = cap, c.forced_slices = env_ll("PHNSW_RANGE_SLICES"), c.stream = (hipStream_t)stream;
  const PhListRadiusDeviceOut o = {out_first_dev, out_ids_dev, out_d_dev, status_dev, out_total_dev};
  return list_radius_device(ix, ph_attr_view(at), c, o, call);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_radius_ranged(const phnsw_index *ix, const phnsw_attr *at, const float *queries,
                                                const uint64_t *qids, uint64_t nq, const uint64_t *exclude, const uint32_t *lo,
                                                const uint32_t *hi, const float *radius, uint64_t cap, uint64_t *out_first,
                                                uint64_t *out_ids, float *out_d, uint64_t *out_total) try {
  const char *const call = "phnsw_search_exact_radius_ranged";
  PH_TRY(list_radius_check(ix, cap, call));
  PH_TRY(ph_attr_fresh(ix, at, call));
  PH_TRY(list_radius_store_check(ix, call));
  return list_radius_host(ix, ph_attr_view(at), queries, qids, nq, exclude, lo, hi, false, radius, cap, out_first, out_ids, out_d,
                          out_total, env_ll("PHNSW_RANGE_SLICES"), call);
} catch (...) { return ph_caught(); }
