// Exact radius search (phnsw_search_exact_radius[_device]): every candidate of ONE shared allow-list closer to a query
// than the query's radius, as a CSR result.  The candidates and the distances are those of filter_dense.hip -- the same
// list builder, the same node chunk x position chunk tables (dense_plan.h, ph_tiny_table_chunk) -- and what differs is
// what is taken from a table: a threshold select with a variable-length result instead of a top-k.
//
//   1. ph_dense_list_enqueue     count, ascending candidate list, sanitised Stored ids (filter_dense.hip)
//      -- the host reads the list's length c (the first synchronisation)
//   2. ph_radius_init_kernel     count[q] = 0, the cursor = 0, status[q] = 0 or 4
//   3. per node chunk, per position chunk: ph_tiny_table_chunk into D[positions][stride], then
//      ph_radius_compact_kernel  one wave64 per position: pass 1 counts the row's entries with D[p][j] < radius[q] (an
//                                f32 comparison; a NaN, zero or negative radius matches nothing, and neither NaN nor
//                                +inf is below any radius), lane 0 reserves that many records with one atomic add on
//                                the 64-bit cursor and adds them to count[q]; pass 2 writes (mkkey(d, id), q) records
//                                by a ballot prefix per 64 entries.  Records at or past the pool's capacity are
//                                dropped, but counted (radius_plan.h)
//   4. (from here on: radius_tail.h) the exclusive sum of count [nq + 1] into out_first; the cursor is the total
//      -- the host reads the total (the second synchronisation; the device form's count-only call skips it)
//   5. total <= cap: two stable radix passes, by key and then by query, and ph_radius_unpack_kernel
//
// The pool's order depends on which wave reserved first; the sorted order does not, because the keys of one query are
// distinct (the id is part of the key), and out_first comes from the counts alone.  So the result is one whatever the
// chunk sizes and the scheduling.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "dense_plan.h"
#include "exact_slices.h"
#include "host_call.h"
#include "phnsw_device.h"
#include "radius_plan.h"
#include "radius_tail.h"

struct PhRadiusArgs {
  const float *D;            // [npos][stride]: the table of this (node chunk, position chunk)
  uint32_t stride, tn;       // tn <= stride
  uint32_t npos, pos_first;  // position p is query pos_first + p
  const uint32_t *list;      // [tn]: the node chunk's VectorIds, ascending
  const uint32_t *exclude;   // [nq] or nullptr
  const uint32_t *refuse;    // [nq] or nullptr: 0, or the status of a refused query
  const float *radius;       // [nq]
  unsigned long long *cursor;  // records reserved so far, dropped ones included
  uint32_t *count;           // [nq + 1]
  uint64_t *keys;            // [records]
  uint32_t *qs;              // [records]
  uint64_t records;          // 0: count only
};

// (ph_radius_init_kernel: radius_tail.h, shared with filter_list_radius.hip)

// One wave64 per position.  Everything that decides a branch (the query, its radius, the row's count) is uniform over
// the wave; count[q] is touched by this wave alone within a launch, and launches follow each other on one stream.
__global__ __launch_bounds__(64) void ph_radius_compact_kernel(PhRadiusArgs a) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t p = blockIdx.x; p < a.npos; p += gridDim.x) {
    const uint32_t q = a.pos_first + p;
    const float r = a.radius[q];
    if (!(r > 0.0f) || (a.refuse && a.refuse[q])) continue;  // the contract: a zero, negative or NaN radius matches nothing
    const uint32_t ex = a.exclude ? a.exclude[q] : PH_EMPTY32;
    const float *const row = a.D + (uint64_t)p * a.stride;
    uint32_t cnt = 0;
    for (uint32_t b = 0; b < a.tn; b += 64u) {
      const uint32_t j = b + lane;
      const bool in = j < a.tn && a.list[j] != ex && row[j] < r;
      cnt += (uint32_t)__popcll(__ballot(in));
    }
    if (!cnt) continue;
    unsigned long long base = 0ull;
    if (lane == 0) {
      base = atomicAdd(a.cursor, (unsigned long long)cnt);
      a.count[q] += cnt;
    }
    if (!a.records) continue;
    base = rl64(base, 0);
    for (uint32_t b = 0; b < a.tn; b += 64u) {
      const uint32_t j = b + lane;
      const uint32_t id = j < a.tn ? a.list[j] : PH_EMPTY32;
      const float d = j < a.tn ? row[j] : 0.0f;
      const bool in = j < a.tn && id != ex && d < r;
      const uint64_t m = __ballot(in);
      const uint64_t slot = base + (uint32_t)__popcll(m & lanemask_lt(lane));
      if (in && slot < a.records) a.keys[slot] = mkkey(d, id), a.qs[slot] = q;
      base += (uint32_t)__popcll(m);
    }
  }
}

// (ph_radius_unpack_kernel, the tail from the exclusive sum on: radius_tail.h)

// ------------------------------------------------------------------ a call's scratch

// A PhCallSet (call_set.h) of the index's `radii` pool; of `ws` only the tiny_* operand fields are used, as in PhDenseSet
struct PhRadiusSet : PhCallSet {
  void *pre = nullptr;  // the candidate list's scratch (dense_plan.h)
  size_t pre_bytes = 0;
  void *post = nullptr;  // radius_plan.h's layout
  size_t post_bytes = 0;
  void *tmp = nullptr;  // the scan's and the sorts' temporary storage
  size_t tmp_bytes = 0;
  uint32_t *h_head = nullptr;  // pinned: [0..1] the count and the list's length, [2..3] the total (one 8-byte word)
  PhWorkspace ws;
};

// the request, checked; device pointers of the caller
struct PhRadiusCall {
  const float *queries;  // [nq][ldq], or nullptr: Stored queries (qids)
  uint32_t ldq;
  const uint32_t *qids, *exclude;  // [nq] or nullptr
  uint64_t nq;
  const uint32_t *filter;  // one bitmap; nullptr: every vector of the index
  const float *radius;     // [nq]
  uint64_t cap;
  uint64_t *out_first;     // [nq + 1]
  uint32_t *status;        // [nq]
  uint64_t *out_total;     // nullable
  bool total_to_host;      // read the total back even when cap == 0
  hipStream_t stream;
};

namespace {

// Steps 1 to 5 without the unpack: *total is exact (and 0 when it was not read back: the device form's count-only
// call); *sorted is the (query, key) ordered records when ph_radius_emits(*total, cap), else nullptr
int radius_run(const phnsw_index *ix, const PhRadiusCall &c, PhRadiusSet &set, uint64_t *total, const uint64_t **sorted) {
  const phnsw_store *s = ix->store;
  const uint64_t nq = c.nq, nwords = ph_exact_words(s->n);
  *total = 0, *sorted = nullptr;
  PH_TRY(set.ready());
  if (!set.h_head) PH_HIP(hipHostMalloc((void **)&set.h_head, 16u, hipHostMallocDefault));
  const uint32_t lcap = ph_dense_list_cap(ix);
  PH_TRY(set.block_ensure(&set.pre, &set.pre_bytes, (size_t)ph_dense_pre_words(nwords, lcap, nq) * 4u, c.stream));

  StepTimes times;
  times.on = env_ll("PHNSW_DENSE_TIMES") > 0, times.stream = c.stream;
  PhDenseList l;
  PH_TRY(ph_dense_list_enqueue(ix, c.filter, c.qids, nq, (uint32_t *)set.pre, &times, 0, 1, c.stream, &l));
  PH_HIP(hipMemcpyAsync(set.h_head, l.head, 8, hipMemcpyDeviceToHost, c.stream));
  PH_HIP(hipStreamSynchronize(c.stream));  // the first synchronisation: the tables' shape depends on the count
  const uint64_t cand = set.h_head[1];
  if (cand != set.h_head[0] || cand > lcap) {
    ph_set_error("exact radius search: the bitmap changed while the call read it (%u candidates counted, %u listed)",
                 set.h_head[0], set.h_head[1]);
    return PHNSW_E_INVALID;
  }

  const uint32_t nodes_knob = ph_dense_nodes_knob(env_ll("PHNSW_DENSE_NODES"));
  const PhDensePlan plan = ph_dense_plan(cand, nq, nodes_knob, ph_dense_bytes_knob(env_ll("PHNSW_DENSE_TABLE_BYTES")));
  const uint64_t records = ph_radius_pool_records(c.cap, nq, cand);
  const PhRadiusLayout lay = ph_radius_layout(nq, records, plan.table_floats);
  PH_TRY(set.block_ensure(&set.post, &set.post_bytes, (size_t)lay.bytes, c.stream));
  char *const post = (char *)set.post;
  PhRadiusArgs a = {};
  a.cursor = (unsigned long long *)(post + lay.head), a.count = (uint32_t *)(post + lay.count);
  a.keys = (uint64_t *)(post + lay.keys_a), a.qs = (uint32_t *)(post + lay.q_a), a.records = records;
  uint64_t *const keys_b = (uint64_t *)(post + lay.keys_b);
  uint32_t *const qs_b = (uint32_t *)(post + lay.q_b);
  float *const D = (float *)(post + lay.table);
  a.D = D, a.exclude = c.exclude, a.refuse = c.qids ? l.refuse : nullptr, a.radius = c.radius;
  hipLaunchKernelGGL(ph_radius_init_kernel, dim3(grid1(nq + 1u)), dim3(256), 0, c.stream, a.count, a.cursor, a.refuse, c.status, nq);
  PH_HIP(hipGetLastError());

  const bool verbose = getenv("PHNSW_VERBOSE") != nullptr;
  const uint32_t *const qids = c.qids ? l.safe : nullptr;
  for (uint32_t i = 0; i < plan.node_chunks; i++) {
    uint64_t nfirst;
    ph_dense_node_chunk(plan, i, &nfirst, &a.tn, &a.stride);
    a.list = l.list + nfirst;  // nfirst + tn <= cand
    set.ws.tiny_pack_key.valid = false;  // the list is scratch that calls reuse: a kept operand serves one node chunk (ph_table_run)
    for (uint64_t j = 0; j < plan.pos_chunks; j++) {
      uint64_t pfirst;
      ph_dense_pos_chunk(plan, j, &pfirst, &a.npos);
      a.pos_first = (uint32_t)pfirst;
      bool kept = false;
      times.begin(2);
      const int trc = ph_tiny_table_chunk(ix, set.ws, c.queries ? c.queries + pfirst * c.ldq : nullptr, c.ldq,
                                          qids ? qids + pfirst : nullptr, nullptr, a.npos, a.list, a.tn, D, c.stream, &kept);
      times.end();
      if (trc > 0) {
        ph_set_error("exact radius search: no device memory for the table's operands (%u positions x %u candidates)", a.npos, a.tn);
        return PHNSW_E_HIP;
      }
      if (trc) return trc;
      if (verbose)
        fprintf(stderr, "[phnsw] exact radius table: node chunk %u/%u (%u ids), positions %llu..+%u, %s, node operand %s\n", i + 1u,
                plan.node_chunks, a.tn, (unsigned long long)pfirst, a.npos, set.ws.tiny_table_g ? "matrix cores" : "vector units",
                kept ? "kept" : "packed");
      times.begin(3);
      hipLaunchKernelGGL(ph_radius_compact_kernel, dim3(ph_radius_grid(a.npos)), dim3(64), 0, c.stream, a);
      PH_HIP(hipGetLastError());
      times.end();
    }
  }

  times.begin(4);
  PhRadiusTail t = {};
  t.nq = nq, t.cap = c.cap, t.records = records, t.cursor = a.cursor, t.count = a.count;
  t.keys_a = a.keys, t.keys_b = keys_b, t.qs_a = a.qs, t.qs_b = qs_b;
  t.out_first = c.out_first, t.out_total = c.out_total, t.total_to_host = c.total_to_host;
  t.h_total = (uint64_t *)set.h_head + 1, t.set = &set, t.tmp = &set.tmp, t.tmp_bytes = &set.tmp_bytes, t.stream = c.stream;
  PH_TRY(ph_radius_tail(t, total, sorted));  // the second synchronisation: whether and how much to sort
  times.end();
  float ms[5];
  if (times.collect(ms, 5))
    fprintf(stderr, "[phnsw] exact_radius: %llu queries x %llu candidates, %llu in radius: count %.3f ms, list %.3f ms, pack+table %.3f ms, "
            "compact %.3f ms, scan+sort %.3f ms\n", (unsigned long long)nq, (unsigned long long)cand, (unsigned long long)*total, ms[0],
            ms[1], ms[2], ms[3], ms[4]);
  return 0;
}

// what both entry points check first, in phnsw_search_exact_shared's order with cap in k's place: the index, cap, the store
int radius_check(const phnsw_index *ix, uint64_t cap, const char *call) {
  if (ix && !ix->layers.empty() && !ph_radius_cap_valid(cap)) {
    ph_set_error("%s: cap must be at most 2^31 - 1 (got %llu)", call, (unsigned long long)cap);
    return PHNSW_E_INVALID;
  }
  return ph_dense_check(ix, 1, call);
}

}  // namespace

PhCallSet *ph_radius_host_set(phnsw_index *ix) { return ph_set_acquire<PhRadiusSet>(ix->radii); }

void ph_radius_free(phnsw_index *ix) {
  ph_sets_free<PhRadiusSet>(ix->radii, [](PhRadiusSet &s) {
    if (s.pre) ph_pool_free(s.pre);
    if (s.post) ph_pool_free(s.post);
    if (s.tmp) ph_pool_free(s.tmp);
    if (s.h_head) hipHostFree(s.h_head);
    ph_tiny_free(s.ws);
  });
}

// ------------------------------------------------------------------ C ABI

extern "C" int phnsw_search_exact_radius_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                                                const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                                const uint32_t *filter_dev, const float *radius_dev, uint64_t cap,
                                                uint64_t *out_first_dev, uint32_t *out_ids_dev, float *out_d_dev,
                                                uint32_t *status_dev, uint64_t *out_total_dev, void *stream) try {
  const char *const call = "phnsw_search_exact_radius_device";
  PH_TRY(radius_check(ix, cap, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !radius_dev || !out_first_dev || !status_dev || !out_total_dev ||
      (cap && (!out_ids_dev || !out_d_dev)) || nq > 0x7FFFFFFEull) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; radius; out_first, status and out_total; out_ids and "
                 "out_d unless cap is 0; nq <= 2^31 - 2; queries need ldq >= store ld, multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhRadiusCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq;
  c.filter = filter_dev ? filter_dev : ix->default_filter;  // phnsw_index_set_filter_device
  c.radius = radius_dev, c.cap = cap, c.out_first = out_first_dev, c.status = status_dev, c.out_total = out_total_dev;
  c.total_to_host = false, c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  phnsw_index *mix = const_cast<phnsw_index *>(ix);
  PhRadiusSet *set = ph_set_acquire<PhRadiusSet>(mix->radii);
  PhSetGuard guard{mix->radii, set, c.stream};
  uint64_t total;
  const uint64_t *sorted;
  PH_TRY(radius_run(ix, c, *set, &total, &sorted));
  if (sorted) PH_TRY(ph_radius_unpack(sorted, total, out_ids_dev, out_d_dev, c.stream));
  return 0;
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_radius(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                                         const uint64_t *exclude, const uint32_t *filter, const float *radius, uint64_t cap,
                                         uint64_t *out_first, uint64_t *out_ids, float *out_d, uint64_t *out_total) try {
  const char *const call = "phnsw_search_exact_radius";
  PH_TRY(radius_check(ix, cap, call));
  if (nq == 0) {  // no query: the empty result, complete
    if (out_first) out_first[0] = 0;
    if (out_total) *out_total = 0;
    return 0;
  }
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!radius || !out_first || !out_total || (cap && (!out_ids || !out_d)) || nq > 0x7FFFFFFEull) {
    ph_set_error("%s: invalid argument (radius, out_first and out_total; out_ids and out_d unless cap is 0; nq <= 2^31 - 2)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, "search"));
  phnsw_index *mix = const_cast<phnsw_index *>(ix);
  PhRadiusSet *set = ph_set_acquire<PhRadiusSet>(mix->radii);
  PhHostCall h(mix->radii, set);
  PH_TRY(h.stage_in(s, queries, qids, exclude, nq, (size_t)nq, 0, 0, 0));  // small's extra: the radii
  PhRadiusCall c = {};
  c.queries = h.queries, c.ldq = h.queries ? h.ld : 0u, c.qids = h.qids, c.exclude = h.exclude, c.nq = nq;
  c.status = h.small + 3u * nq, c.stream = h.st;  // the ids were checked: every status is 0
  PH_HIP(hipMemcpyAsync(h.extra(), radius, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
  c.radius = (const float *)h.extra();
  if (filter) {
    const size_t words = (size_t)ph_exact_words(s->n);
    uint32_t *f = nullptr;
    PH_TRY(h.blocks.alloc(&f, words * 4u));
    PH_HIP(hipMemcpyAsync(f, filter, words * 4u, hipMemcpyHostToDevice, h.st));
    c.filter = f;
  } else {
    c.filter = ix->default_filter;  // phnsw_index_set_filter_device: device words
  }
  c.cap = cap, c.total_to_host = true;
  PH_TRY(h.blocks.alloc(&c.out_first, (size_t)(nq + 1u) * 8u));
  uint64_t total;
  const uint64_t *sorted;
  PH_TRY(radius_run(ix, c, *set, &total, &sorted));
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
} catch (...) { return ph_caught(); }
