// Exact top-k for a TABLE of allow-lists with a per-query selector (phnsw_search_exact_grouped[_device]): a handful of
// distinct bitmaps, each shared by many queries of the batch -- tenants, ACL classes.  The batch is grouped by bitmap on
// the device and every group runs as the queries x candidates distance tables of filter_dense.hip, with ONE stream
// synchronisation for the whole call.
//
//   1. ph_grouped_keys_kernel    a 32-bit key per query (group_plan.h): its bitmap, ALL, or reject (a selector outside
//                                the table, a Stored id at or past n) with the status it will report
//      radix sort (key, query)   order[]: the queries of a key are contiguous positions, in query order
//      ph_grouped_flags_kernel   where a key starts; their exclusive sum numbers the groups in position order
//      ph_grouped_heads_kernel   per group its first position and its key; the number of groups
//   2. ph_grouped_count_kernel   candidates per GROUP (ph_exact_word: the scan's own candidate test, no exclude)
//      ph_grouped_cum_kernel     their exclusive 64-bit prefix: where a group's list starts inside its round
//      -- the host reads the groups and the counts (the one synchronisation)
//   3. per round of groups under the list budget (group_plan.h), grids over (words, groups of the round):
//      ph_grouped_popc_kernel / ph_grouped_prefix_kernel / ph_grouped_list_kernel: the ascending VectorId list of
//      every group, CSR; the prefix checks the list's length against the count, the list kernel every word against
//      its popcount: a bitmap that changed under the call marks its group, whose rows come back empty with status 7
//   4. per group ph_table_run (filter_dense.hip): per node chunk, per position chunk (dense_plan.h) the table
//      (ph_tiny_table_chunk, tiny.hip: the search's table kernels), position p of the group being query order[first + p],
//   5. then ph_table_select_kernel: one wave64 per position, the running top-k carried between node chunks in a
//      [nq][k] key scratch indexed by the QUERY; rows of refused queries and of groups without candidates are written
//      by the same kernel over no table
//
// The keys are distinct, so the k smallest are one set in one order whatever the grouping and the chunk sizes; the
// distances are the table's, i.e. phnsw_distance_batch's bits, so a row equals phnsw_search_exact_filtered's bit for bit.
// The block scan and the block sum of the list builder are exact_topk.h's (profiles/exact_once/).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dense_plan.h"
#include "exact_slices.h"
#include "exact_topk.h"
#include "filter_candidate.h"
#include "group_plan.h"
#include "host_call.h"
#include "phnsw_device.h"

// ------------------------------------------------------------------ grouping

__global__ __launch_bounds__(256) void ph_grouped_keys_kernel(const uint32_t *filter_of, const uint32_t *qids, uint32_t nq,
                                                              uint32_t n, uint64_t nfilters, uint32_t *keys, uint32_t *iota,
                                                              uint32_t *safe, uint32_t *why) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * 256u) {
    uint32_t key = ph_group_key(filter_of[q], nfilters);
    uint32_t st = key == PH_GROUP_KEY_REJECT ? PH_GROUP_ST_SELECTOR : PH_GROUP_ST_OK;
    uint32_t v = qids ? qids[q] : 0u;
    if (v >= n) v = 0u, key = PH_GROUP_KEY_REJECT, st = PH_GROUP_ST_MISSING;  // the pack kernels read rows unchecked (n >= 1)
    keys[q] = key, iota[q] = (uint32_t)q, safe[q] = v, why[q] = st;
  }
}

// flags [nq + 1]: 1 where a key starts; entry nq is 0, so its exclusive sum is the number of groups
__global__ __launch_bounds__(256) void ph_grouped_flags_kernel(const uint32_t *skeys, uint32_t nq, uint32_t *flags) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p <= nq; p += (uint64_t)gridDim.x * 256u)
    flags[p] = p < nq && (p == 0 || skeys[p] != skeys[p - 1u]) ? 1u : 0u;
}

struct PhGroupedHeadArgs {
  const uint32_t *skeys, *flags, *slots;  // [nq], [nq + 1], [nq + 1]
  uint32_t nq, gmax;                      // gmax: ph_group_max, the groups the arrays hold
  uint32_t *head, *gfirst, *gkey;         // head[0] = groups; gfirst [gmax + 1], gkey [gmax]
};
__global__ __launch_bounds__(256) void ph_grouped_heads_kernel(PhGroupedHeadArgs a) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < a.nq; p += (uint64_t)gridDim.x * 256u) {
    if (p == 0) {
      const uint32_t ng = a.slots[a.nq];
      a.head[0] = ng;
      if (ng <= a.gmax) a.gfirst[ng] = a.nq;
    }
    if (!a.flags[p]) continue;
    const uint32_t s = a.slots[p];
    if (s < a.gmax) a.gfirst[s] = (uint32_t)p, a.gkey[s] = a.skeys[p];  // distinct keys <= nfilters + 2: always
  }
}

// ------------------------------------------------------------------ counts and candidate lists

struct PhGroupedListArgs {
  const uint32_t *filters;  // the table: nfilters bitmaps, stride_words apart
  uint32_t stride_words;
  uint64_t nfilters;
  uint32_t n, nwords;
  // the index's bottom layer, as the candidate test takes it
  uint32_t n_nodes;
  const uint32_t *nodes, *vec2node;
  const uint32_t *ngroups;  // device word: the number of groups
  uint32_t gmax;
  const uint32_t *gkey;  // [gmax]
  uint32_t *gcount;      // [gmax]
  uint64_t *gcum;        // [gmax + 1]: exclusive prefix of gcount
  uint32_t *gerr;        // [gmax]: nonzero = the group's bitmap changed while the call read it
  // the round: groups [g0, g0 + ng)
  uint32_t g0, ng;
  uint32_t *off;   // [ng][nwords + 1]
  uint32_t *list;  // the round's lists, group g at entry gcum[g] - gcum[g0]
};

// word w of the bitmap a key names, reduced to candidates; the reject group has none and reads no bitmap
__device__ __forceinline__ uint32_t ph_grouped_word(const PhGroupedListArgs &a, uint32_t key, uint32_t w, uint32_t nlim) {
  if (key == PH_GROUP_KEY_REJECT) return 0u;
  const uint32_t *const bitmap =
      ph_group_key_has_bitmap(key, a.nfilters) ? a.filters + ph_group_bitmap_at(key, a.stride_words) : nullptr;
  return ph_exact_word(bitmap, w, a.nwords, nlim, a.vec2node);
}

// one block per group, striding: a popcount over the scan's candidate test
__global__ __launch_bounds__(256) void ph_grouped_count_kernel(PhGroupedListArgs a) {
  const uint32_t nlim = ph_exact_id_limit(a.n, a.n_nodes, a.nodes, a.vec2node);
  const uint32_t ng = min(a.ngroups[0], a.gmax);
  for (uint32_t g = blockIdx.x; g < ng; g += gridDim.x) {
    const uint32_t key = a.gkey[g];
    uint32_t c = 0;
    for (uint32_t w = threadIdx.x; w < a.nwords; w += 256u) c += (uint32_t)__popc(ph_grouped_word(a, key, w, nlim));
    c = ph_block_sum256(c);
    if (threadIdx.x == 0) a.gcount[g] = c;
  }
}

// one workgroup: gcum[0 .. ng] = exclusive 64-bit prefix of gcount[0 .. ng), 1024 groups at a time
__global__ __launch_bounds__(1024) void ph_grouped_cum_kernel(PhGroupedListArgs a) {
  const uint32_t ng = min(a.ngroups[0], a.gmax);
  unsigned long long base = 0;
  for (uint32_t at = 0; at < ng; at += 1024u) {
    const uint32_t g = at + threadIdx.x;
    const unsigned long long before = ph_block_exclusive_scan<unsigned long long>(g < ng ? a.gcount[g] : 0ull, base);
    if (g < ng) a.gcum[g] = before;
    __syncthreads();  // the totals are rewritten by the next 1024
  }
  if (threadIdx.x == 0) a.gcum[ng] = base;
}

// grid (words, groups of the round): candidates per bitmap word
__global__ __launch_bounds__(256) void ph_grouped_popc_kernel(PhGroupedListArgs a) {
  const uint32_t nlim = ph_exact_id_limit(a.n, a.n_nodes, a.nodes, a.vec2node);
  const uint32_t key = a.gkey[a.g0 + blockIdx.y];
  uint32_t *const off = a.off + (uint64_t)blockIdx.y * ph_group_off_words(a.nwords);
  for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < a.nwords; w += (uint64_t)gridDim.x * 256u)
    off[w] = (uint32_t)__popc(ph_grouped_word(a, key, (uint32_t)w, nlim));
}

// one workgroup per group of the round: the exclusive prefix of its counts in place, the total checked against the count
// the round was laid out from
__global__ __launch_bounds__(1024) void ph_grouped_prefix_kernel(PhGroupedListArgs a) {
  const uint32_t g = a.g0 + blockIdx.x;
  uint32_t *const off = a.off + (uint64_t)blockIdx.x * ph_group_off_words(a.nwords);
  uint32_t base = 0;
  for (uint64_t at = 0; at < a.nwords; at += 1024u) {
    const uint64_t w = at + threadIdx.x;
    const uint32_t before = ph_block_exclusive_scan(w < a.nwords ? off[w] : 0u, base);
    if (w < a.nwords) off[w] = before;
    __syncthreads();  // the totals are rewritten by the next 1024
  }
  if (threadIdx.x == 0) off[a.nwords] = base, a.gerr[g] = base != a.gcount[g] ? 1u : 0u;
}

// grid (words, groups of the round): every word writes as many ids as its popcount WAS, at its offset.  Every entry of
// a list is written with an id below n whatever the bitmap does meanwhile (the table kernels read rows unchecked): a
// word with fewer bits now pads with id 0, a list whose length is not the count is filled with id 0 by the group's
// first block; both mark the group.
__global__ __launch_bounds__(256) void ph_grouped_list_kernel(PhGroupedListArgs a) {
  const uint32_t nlim = ph_exact_id_limit(a.n, a.n_nodes, a.nodes, a.vec2node);
  const uint32_t g = a.g0 + blockIdx.y;
  const uint32_t key = a.gkey[g], cap = a.gcount[g];
  const uint32_t *const off = a.off + (uint64_t)blockIdx.y * ph_group_off_words(a.nwords);
  uint32_t *const list = a.list + (a.gcum[g] - a.gcum[a.g0]);
  if (off[a.nwords] != cap) {  // uniform over the group's blocks: the prefix kernel has marked it
    if (blockIdx.x == 0)
      for (uint32_t i = threadIdx.x; i < cap; i += 256u) list[i] = 0u;
    return;
  }
  for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < a.nwords; w += (uint64_t)gridDim.x * 256u) {
    const uint32_t o = off[w], cnt = off[w + 1u] - o;  // o + cnt <= off[nwords] == cap
    uint32_t t = ph_grouped_word(a, key, (uint32_t)w, nlim);
    if ((uint32_t)__popc(t) != cnt) a.gerr[g] = 1u;
    for (uint32_t i = 0; i < cnt; i++) {
      list[o + i] = t ? (uint32_t)w * 32u + (uint32_t)__ffs((int)t) - 1u : 0u;  // ascending within the word and across words
      t &= t - 1u;
    }
  }
}

// ------------------------------------------------------------------ a call's scratch

// A PhCallSet (call_set.h) of the index's `groupeds` pool.  Of `ws` only the tiny_* operand fields are used.
struct PhGroupedSet : PhCallSet {
  void *pre = nullptr, *tmp = nullptr, *lists = nullptr, *post = nullptr;  // group_plan.h; tmp: the sort's and the scan's
  size_t pre_bytes = 0, tmp_bytes = 0, lists_bytes = 0, post_bytes = 0;
  uint32_t *h_read = nullptr;  // pinned: head, groups and counts as the host reads them
  size_t h_read_words = 0;
  PhWorkspace ws;
};

// the request, checked; device pointers of the caller
struct PhGroupedCall {
  const float *queries;  // [nq][ldq], or nullptr: Stored queries (qids)
  uint32_t ldq;
  const uint32_t *qids, *exclude;  // [nq] or nullptr
  uint64_t nq;
  const uint32_t *filters;  // the table
  uint32_t stride_words;
  uint64_t nfilters;
  const uint32_t *filter_of;  // [nq]
  uint32_t k;
  uint32_t *out_ids;  // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
  hipStream_t stream;
};

namespace {

// the orchestration on a set the caller holds; c is checked, 0 < nq <= PH_GROUP_NQ_MAX
int grouped_run(const phnsw_index *ix, const PhGroupedCall &c, PhGroupedSet &set) {
  const phnsw_store *s = ix->store;
  const uint64_t nq = c.nq, nwords = ph_exact_words(s->n);
  const uint64_t gmax = ph_group_max(nq, c.nfilters);
  const PhGroupPre lay = ph_group_pre(nq, gmax);
  PH_TRY(set.ready());
  if (set.h_read_words < lay.read_words) {
    if (set.h_read) {
      PH_HIP(hipEventSynchronize(set.done));
      PH_HIP(hipHostFree(set.h_read));
      set.h_read = nullptr, set.h_read_words = 0;
    }
    PH_HIP(hipHostMalloc((void **)&set.h_read, (size_t)lay.read_words * 4u, hipHostMallocDefault));
    set.h_read_words = (size_t)lay.read_words;
  }
  PH_TRY(set.block_ensure(&set.pre, &set.pre_bytes, (size_t)lay.words * 4u, c.stream));
  uint32_t *const pre = (uint32_t *)set.pre;
  uint32_t *const head = pre + lay.head, *const gfirst = pre + lay.gfirst, *const gkey = pre + lay.gkey;
  uint32_t *const gcount = pre + lay.gcount, *const gerr = pre + lay.gerr;
  uint64_t *const gcum = (uint64_t *)(pre + lay.gcum);
  uint32_t *const keys = pre + lay.keys, *const skeys = pre + lay.skeys, *const iota = pre + lay.iota;
  uint32_t *const order = pre + lay.order, *const flags = pre + lay.flags, *const slots = pre + lay.slots;
  uint32_t *const safe = pre + lay.safe, *const why = pre + lay.why;
  size_t sort_bytes = 0, scan_bytes = 0;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys, skeys, iota, order, (int)nq, 0, 32, c.stream));
  PH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, flags, slots, (int)(nq + 1u), c.stream));
  PH_TRY(set.block_ensure(&set.tmp, &set.tmp_bytes, std::max<size_t>(std::max(sort_bytes, scan_bytes), 16), c.stream));

  enum { GROUP, COUNT, LIST, TABLE, SELECT, STEPS };
  StepTimes times;  // pack and table are one figure: both are enqueued inside tiny_table
  times.on = env_ll("PHNSW_GROUP_TIMES") > 0, times.stream = c.stream;
  times.begin(GROUP);
  hipLaunchKernelGGL(ph_grouped_keys_kernel, dim3(grid1(nq)), dim3(256), 0, c.stream, c.filter_of, c.qids, (uint32_t)nq,
                     (uint32_t)s->n, c.nfilters, keys, iota, safe, why);
  PH_HIP(hipGetLastError());
  size_t bytes = set.tmp_bytes;
  PH_HIP(hipcub::DeviceRadixSort::SortPairs(set.tmp, bytes, keys, skeys, iota, order, (int)nq, 0, 32, c.stream));
  hipLaunchKernelGGL(ph_grouped_flags_kernel, dim3(grid1(nq + 1u)), dim3(256), 0, c.stream, skeys, (uint32_t)nq, flags);
  PH_HIP(hipGetLastError());
  bytes = set.tmp_bytes;
  PH_HIP(hipcub::DeviceScan::ExclusiveSum(set.tmp, bytes, flags, slots, (int)(nq + 1u), c.stream));
  PhGroupedHeadArgs h = {};
  h.skeys = skeys, h.flags = flags, h.slots = slots, h.nq = (uint32_t)nq, h.gmax = (uint32_t)gmax;
  h.head = head, h.gfirst = gfirst, h.gkey = gkey;
  hipLaunchKernelGGL(ph_grouped_heads_kernel, dim3(grid1(nq)), dim3(256), 0, c.stream, h);
  PH_HIP(hipGetLastError());
  times.end();

  PhGroupedListArgs l = {};
  l.filters = c.filters, l.stride_words = c.stride_words, l.nfilters = c.nfilters;
  l.n = (uint32_t)s->n, l.nwords = (uint32_t)nwords;
  ph_exact_bottom_layer(ix, &l.n_nodes, &l.nodes, &l.vec2node);
  l.ngroups = slots + nq, l.gmax = (uint32_t)gmax, l.gkey = gkey, l.gcount = gcount, l.gcum = gcum, l.gerr = gerr;
  const uint64_t cap = std::min<uint64_t>(s->n, l.n_nodes);  // a candidate is a vector of the bottom layer
  times.begin(COUNT);
  hipLaunchKernelGGL(ph_grouped_count_kernel, dim3((uint32_t)std::min<uint64_t>(gmax, 4096u)), dim3(256), 0, c.stream, l);
  hipLaunchKernelGGL(ph_grouped_cum_kernel, dim3(1), dim3(1024), 0, c.stream, l);
  PH_HIP(hipGetLastError());
  times.end();
  PH_HIP(hipMemcpyAsync(set.h_read, pre, (size_t)lay.read_words * 4u, hipMemcpyDeviceToHost, c.stream));
  PH_HIP(hipStreamSynchronize(c.stream));  // the one synchronisation: rounds and tables depend on the groups and their counts
  const uint64_t ngroups = set.h_read[lay.head];
  const uint32_t *const hfirst = set.h_read + lay.gfirst, *const hkey = set.h_read + lay.gkey;
  const uint32_t *const hcount = set.h_read + lay.gcount;
  bool sane = ngroups >= 1u && ngroups <= gmax && hfirst[0] == 0u && hfirst[ngroups] == nq;
  for (uint64_t g = 0; sane && g < ngroups; g++)
    sane = hfirst[g] < hfirst[g + 1u] && hcount[g] <= cap && (g == 0 || hkey[g - 1u] < hkey[g]);
  if (!sane) {
    ph_set_error("exact grouped search: the selectors or a bitmap changed while the call read them (%llu groups of %llu queries)",
                 (unsigned long long)ngroups, (unsigned long long)nq);
    return PHNSW_E_INVALID;
  }

  // what the rest needs, from the counts: the list block of the largest round, the largest table of any group
  const uint64_t budget = ph_group_bytes_knob(env_ll("PHNSW_GROUP_LIST_BYTES"));
  const uint32_t nodes_knob = ph_dense_nodes_knob(env_ll("PHNSW_DENSE_NODES"));
  const uint64_t bytes_knob = ph_dense_bytes_knob(env_ll("PHNSW_DENSE_TABLE_BYTES"));
  uint64_t rounds = 0, table_floats = 0, listed = 0;
  const uint64_t list_bytes = ph_group_list_bytes(hcount, ngroups, nwords, budget, &rounds);
  for (uint64_t g = 0; g < ngroups; g++) {
    if (!hcount[g]) continue;
    const PhDensePlan plan = ph_dense_plan(hcount[g], hfirst[g + 1u] - hfirst[g], nodes_knob, bytes_knob);
    table_floats = std::max(table_floats, plan.table_floats);
    listed += hcount[g];
  }
  PH_TRY(set.block_ensure(&set.lists, &set.lists_bytes, (size_t)list_bytes, c.stream));
  PH_TRY(set.block_ensure(&set.post, &set.post_bytes, (size_t)std::max<uint64_t>(ph_group_post_bytes(nq, c.k, table_floats), 16u),
                      c.stream));
  PhTableRun r = {};
  r.queries = c.queries, r.ldq = c.ldq, r.qids = c.qids ? safe : nullptr;
  r.nodes_knob = nodes_knob, r.bytes_knob = bytes_knob;
  r.exclude = c.exclude, r.refuse = why, r.k = c.k;
  r.keys = (uint64_t *)set.post, r.D = (float *)((char *)set.post + ph_group_key_bytes(nq, c.k));
  r.out_ids = c.out_ids, r.out_d = c.out_d, r.out_len = c.out_len, r.status = c.status;
  r.stream = c.stream, r.times = &times, r.step_table = TABLE, r.step_select = SELECT;
  r.call = "exact grouped search";
  const bool verbose = getenv("PHNSW_VERBOSE") != nullptr;
  const uint32_t wgrid = grid1(nwords);

  for (uint64_t g0 = 0, round = 0; g0 < ngroups; round++) {
    const uint64_t g1 = ph_group_round_end(hcount, ngroups, g0, nwords, budget);
    l.g0 = (uint32_t)g0, l.ng = (uint32_t)(g1 - g0);
    l.off = (uint32_t *)set.lists;
    l.list = l.off + ph_group_round_off_words(g0, g1, nwords);
    times.begin(LIST);
    if (nwords) hipLaunchKernelGGL(ph_grouped_popc_kernel, dim3(wgrid, l.ng), dim3(256), 0, c.stream, l);
    hipLaunchKernelGGL(ph_grouped_prefix_kernel, dim3(l.ng), dim3(1024), 0, c.stream, l);
    if (nwords) hipLaunchKernelGGL(ph_grouped_list_kernel, dim3(wgrid, l.ng), dim3(256), 0, c.stream, l);
    PH_HIP(hipGetLastError());
    times.end();
    if (verbose)
      fprintf(stderr, "[phnsw] exact grouped round %llu/%llu: groups %llu..%llu of %llu\n", (unsigned long long)round + 1u,
              (unsigned long long)rounds, (unsigned long long)g0, (unsigned long long)g1, (unsigned long long)ngroups);
    uint64_t list_at = 0;
    for (uint64_t g = g0; g < g1; list_at += hcount[g], g++) {
      char prefix[96] = "";
      if (verbose) snprintf(prefix, sizeof prefix, "exact grouped table: group %llu (key %u), ", (unsigned long long)g, hkey[g]);
      // positions [first, first + npos) of the order are the group's queries; without candidates: empty rows, and the
      // status of the reject group's queries, from the select itself
      r.order = order, r.first = hfirst[g], r.npos = hfirst[g + 1u] - hfirst[g];
      r.list = l.list + list_at, r.cand = hcount[g], r.changed = gerr + g, r.verbose_prefix = prefix;
      PH_TRY(ph_table_run(ix, set.ws, r));
    }
    g0 = g1;
  }
  float ms[STEPS];
  if (times.collect(ms, STEPS))
    fprintf(stderr, "[phnsw] exact_grouped: %llu queries, %llu groups in %llu rounds, %llu listed candidates: group %.3f ms, "
            "count %.3f ms, list %.3f ms, pack+table %.3f ms, select %.3f ms\n",
            (unsigned long long)nq, (unsigned long long)ngroups, (unsigned long long)rounds, (unsigned long long)listed, ms[GROUP],
            ms[COUNT], ms[LIST], ms[TABLE], ms[SELECT]);
  return 0;
}

// the table arguments both forms take
bool table_args_ok(const phnsw_index *ix, const uint32_t *filters, uint32_t stride_words, uint64_t nfilters,
                   const uint32_t *filter_of, uint64_t nq) {
  return filters && filter_of && stride_words != 0u && stride_words >= ph_exact_words(ix->store->n) && nfilters >= 1u &&
         nfilters <= PH_GROUP_NFILTERS_MAX && nq <= PH_GROUP_NQ_MAX;
}

}  // namespace

void ph_grouped_free(phnsw_index *ix) {
  ph_sets_free<PhGroupedSet>(ix->groupeds, [](PhGroupedSet &s) {
    if (s.pre) ph_pool_free(s.pre);
    if (s.tmp) ph_pool_free(s.tmp);
    if (s.lists) ph_pool_free(s.lists);
    if (s.post) ph_pool_free(s.post);
    if (s.h_read) hipHostFree(s.h_read);
    ph_tiny_free(s.ws);
  });
}

// ------------------------------------------------------------------ C ABI

extern "C" int phnsw_search_exact_grouped_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                                                 const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                                 const uint32_t *filters_dev, uint32_t filter_stride_words, uint64_t nfilters,
                                                 const uint32_t *filter_of_dev, uint64_t k, uint32_t *out_ids_dev,
                                                 float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev,
                                                 void *stream) try {
  const char *const call = "phnsw_search_exact_grouped_device";
  PH_TRY(ph_dense_check(ix, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !table_args_ok(ix, filters_dev, filter_stride_words, nfilters, filter_of_dev, nq)) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; filters and filter_of, a stride of at least "
                 "ceil(n/32) words, 1 <= nfilters <= 0xFFFFFFFE, nq < 2^31 - 1; queries need ldq >= store ld, multiple of 4, "
                 "16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhGroupedCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq;
  c.filters = filters_dev, c.stride_words = filter_stride_words, c.nfilters = nfilters, c.filter_of = filter_of_dev;
  c.k = (uint32_t)k;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  phnsw_index *mix = const_cast<phnsw_index *>(ix);
  PhGroupedSet *set = ph_set_acquire<PhGroupedSet>(mix->groupeds);
  PhSetGuard guard{mix->groupeds, set, c.stream};
  return grouped_run(ix, c, *set);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_grouped(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                                          const uint64_t *exclude, const uint32_t *filters, uint32_t filter_stride_words,
                                          uint64_t nfilters, const uint32_t *filter_of, uint64_t k, uint64_t *out_ids,
                                          float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_search_exact_grouped";
  PH_TRY(ph_dense_check(ix, k, call));
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!out_ids || !out_d || !out_len || !table_args_ok(ix, filters, filter_stride_words, nfilters, filter_of, nq)) {
    ph_set_error("%s: invalid argument (outputs; filters and filter_of, a stride of at least ceil(n/32) words, "
                 "1 <= nfilters <= 0xFFFFFFFE, nq < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, "search"));
  for (uint64_t i = 0; i < nq; i++)
    if (ph_group_key(filter_of[i], nfilters) == PH_GROUP_KEY_REJECT) {
      ph_set_error("%s: query %llu selects bitmap %u of a table of %llu (PHNSW_FILTER_ALL = no bitmap)", call,
                   (unsigned long long)i, filter_of[i], (unsigned long long)nfilters);
      return PHNSW_E_INVALID;
    }
  phnsw_index *mix = const_cast<phnsw_index *>(ix);
  PhGroupedSet *set = ph_set_acquire<PhGroupedSet>(mix->groupeds);
  PhHostCall h(mix->groupeds, set);
  PH_TRY(h.stage_in(s, queries, qids, exclude, nq, (size_t)nq, 0, (uint32_t)k, (uint32_t)k));  // extras: the selectors
  PhGroupedCall c = {};
  h.fill(c);
  PH_HIP(hipMemcpyAsync(h.extra(), filter_of, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
  c.filter_of = h.extra();
  {  // the whole table, strides and all: what lies between the bitmaps is never read
    const size_t words = (size_t)((nfilters - 1u) * filter_stride_words + ph_exact_words(s->n));
    uint32_t *f = nullptr;
    PH_TRY(h.blocks.alloc(&f, words * 4u));
    PH_HIP(hipMemcpyAsync(f, filters, words * 4u, hipMemcpyHostToDevice, h.st));
    c.filters = f, c.stride_words = filter_stride_words, c.nfilters = nfilters;
  }
  c.k = (uint32_t)k;
  PH_TRY(grouped_run(ix, c, *set));
  PH_TRY(h.take());
  PH_TRY(h.download_words());
  PH_TRY(h.sync());
  // ids and selectors were checked: a status here is 7, a bitmap of the (device-resident copy of the) table changed;
  // the caller's rows are then left as they were
  for (uint64_t i = 0; i < nq; i++)
    if (h.status(i)) {
      ph_set_error("%s: a bitmap changed while the call read it (query %llu, status %u)", call, (unsigned long long)i,
                   h.status(i));
      return PHNSW_E_INVALID;
    }
  return h.finish(out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }
