// Exact top-k over ONE allow-list shared by the whole batch, as a distance table (phnsw_search_exact_shared[_device]):
// with a shared bitmap every query meets the same candidate rows, so the work is a queries x rows table -- the work
// tiny.hip already does for the dense top layers -- and not the per-query scan of filter_exact.hip.
//
//   1. ph_filter_count          candidates of the one bitmap
//   2. ph_dense_popc_kernel     candidates per bitmap word (ph_exact_word: the scan's own candidate test, no exclude)
//      ph_dense_prefix_kernel   their exclusive prefix over the ceil(n / 32) words; the total is the list's length
//      ph_dense_list_kernel     every word writes its ids at its offset: the ascending VectorId list of the candidates
//      -- the host reads the length c (the one synchronisation); c == 0 writes empty rows and returns
//   3. ph_dense_qids_kernel     Stored queries: ids at or past n replaced by 0 (the pack kernel reads rows unchecked)
//                               and given the status word the select reports them with: 4 and an empty row, as the scan
//   4. ph_table_run: per node chunk, per position chunk (dense_plan.h): ph_tiny_table_chunk (tiny.hip) -- the search's
//      table kernels, the per-hop bits -- into D[positions][stride]
//   5. ph_table_select_kernel   one wave64 per position: the running top-k of (distance, id) keys over the chunk's row
//                               of D, carried between node chunks in a [nq][k] key scratch; after the last node chunk
//                               the row is written
//
// The keys are distinct, so the k smallest are one set in one order whatever the chunk sizes; the distances are the
// table's, i.e. phnsw_distance_batch's bits, so a row equals phnsw_search_exact_filtered's row bit for bit.
// Steps 4 and 5 also serve every group of filter_grouped.hip: position p is then query order[p], and a query may be
// refused for its selector or its group's bitmap.  The running top-k, the block scan and the row writer are
// exact_topk.h's (profiles/exact_once/).
#include <hip/hip_runtime.h>

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

// ------------------------------------------------------------------ the candidate list

struct PhDenseListArgs {
  const uint32_t *filter;  // nullptr: every vector of the index
  uint32_t n, nwords;
  // the index's bottom layer, as the candidate test takes it
  uint32_t n_nodes;
  const uint32_t *nodes, *vec2node;
  uint32_t *head;  // [PH_DENSE_HEAD_WORDS]: [1] = the list's length
  uint32_t *off;   // [nwords + 1]
  uint32_t *list;  // [cap]
  uint32_t cap;
};

__global__ __launch_bounds__(256) void ph_dense_popc_kernel(PhDenseListArgs a) {
  const uint32_t nlim = ph_exact_id_limit(a.n, a.n_nodes, a.nodes, a.vec2node);
  for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < a.nwords; w += (uint64_t)gridDim.x * 256u)
    a.off[w] = (uint32_t)__popc(ph_exact_word(a.filter, (uint32_t)w, a.nwords, nlim, a.vec2node));
}

// One workgroup walks the counts 1024 at a time and leaves their exclusive prefix in place (ph_block_exclusive_scan).
// The total is at most n <= 2^31 - 1.
__global__ __launch_bounds__(1024) void ph_dense_prefix_kernel(PhDenseListArgs a) {
  uint32_t base = 0;
  for (uint64_t at = 0; at < a.nwords; at += 1024u) {
    const uint64_t w = at + threadIdx.x;
    const uint32_t before = ph_block_exclusive_scan(w < a.nwords ? a.off[w] : 0u, base);
    if (w < a.nwords) a.off[w] = before;
    __syncthreads();  // the totals are rewritten by the next 1024
  }
  if (threadIdx.x == 0) a.off[a.nwords] = base, a.head[1] = base;
}

__global__ __launch_bounds__(256) void ph_dense_list_kernel(PhDenseListArgs a) {
  const uint32_t nlim = ph_exact_id_limit(a.n, a.n_nodes, a.nodes, a.vec2node);
  for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < a.nwords; w += (uint64_t)gridDim.x * 256u) {
    uint32_t o = a.off[w];
    for (uint32_t t = ph_exact_word(a.filter, (uint32_t)w, a.nwords, nlim, a.vec2node); t; t &= t - 1u) {
      if (o < a.cap) a.list[o] = (uint32_t)w * 32u + (uint32_t)__ffs((int)t) - 1u;  // ascending within the word and across words
      o++;
    }
  }
}

// Stored queries as the table kernels may read them: an id at or past n becomes 0 (n >= 1: the index has a bottom layer
// with candidates when this runs into a table) and its word of `refuse` is the status the select reports for it
__global__ __launch_bounds__(256) void ph_dense_qids_kernel(const uint32_t *qids, uint64_t nq, uint32_t n, uint32_t *safe,
                                                            uint32_t *refuse) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * 256u) {
    const uint32_t v = qids[q];
    safe[q] = v < n ? v : 0u;
    refuse[q] = v < n ? ST_OK : ST_MISSING;
  }
}

// Steps 1 to 3 on scratch the caller holds (`pre`: ph_dense_pre_words(words of the store, ph_dense_list_cap, nq) words),
// enqueued on `stream`: the count, the list and -- with Stored queries -- their sanitised ids and refusal words.  The
// exact radius search (filter_radius.hip) builds its candidates with it too.
uint32_t ph_dense_list_cap(const phnsw_index *ix) {
  uint32_t n_nodes;
  const uint32_t *nodes, *vec2node;
  ph_exact_bottom_layer(ix, &n_nodes, &nodes, &vec2node);
  return (uint32_t)std::min<uint64_t>(ix->store->n, n_nodes);  // a candidate is a vector of the bottom layer
}

int ph_dense_list_enqueue(const phnsw_index *ix, const uint32_t *filter, const uint32_t *qids, uint64_t nq, uint32_t *pre,
                          StepTimes *times, int step_count, int step_list, hipStream_t stream, PhDenseList *out) {
  const phnsw_store *s = ix->store;
  const uint64_t nwords = ph_exact_words(s->n);
  PhDenseListArgs l = {};
  l.filter = filter, l.n = (uint32_t)s->n, l.nwords = (uint32_t)nwords;
  ph_exact_bottom_layer(ix, &l.n_nodes, &l.nodes, &l.vec2node);
  l.cap = ph_dense_list_cap(ix);
  uint32_t *const head = pre, *const off = head + PH_DENSE_HEAD_WORDS, *const list = off + ph_dense_off_words(nwords);
  uint32_t *const safe = list + l.cap, *const refuse = safe + nq;
  l.head = head, l.off = off, l.list = list;
  times->begin(step_count);
  PhFilter one = {filter, 0u, 0u};
  PH_TRY(ph_filter_count(ix, one, 1, head, stream));
  times->end();
  times->begin(step_list);
  const uint32_t wgrid = (uint32_t)std::min<uint64_t>((nwords + 255u) / 256u, 1u << 16);
  if (nwords) {
    hipLaunchKernelGGL(ph_dense_popc_kernel, dim3(wgrid), dim3(256), 0, stream, l);
    hipLaunchKernelGGL(ph_dense_prefix_kernel, dim3(1), dim3(1024), 0, stream, l);
    hipLaunchKernelGGL(ph_dense_list_kernel, dim3(wgrid), dim3(256), 0, stream, l);
  } else {
    PH_HIP(hipMemsetAsync(head, 0, PH_DENSE_HEAD_WORDS * 4u, stream));
  }
  if (qids)
    hipLaunchKernelGGL(ph_dense_qids_kernel, dim3((uint32_t)std::min<uint64_t>((nq + 255u) / 256u, 1u << 16)), dim3(256), 0,
                       stream, qids, nq, (uint32_t)s->n, safe, refuse);
  PH_HIP(hipGetLastError());
  times->end();
  out->head = head, out->list = list, out->safe = safe, out->refuse = refuse;
  return 0;
}

// ------------------------------------------------------------------ the select

struct PhTableSelectArgs {
  const float *D;          // [npos][stride]: the table of this (node chunk, position chunk); unread when tn == 0
  uint32_t stride, tn;     // tn <= stride
  uint32_t npos, pos_first;  // positions of this chunk
  const uint32_t *order;   // [npos]: position p is query order[p]; nullptr: query pos_first + p
  const uint32_t *list;    // [tn]: the node chunk's VectorIds, ascending
  const uint32_t *exclude;  // [nq] or nullptr
  const uint32_t *refuse;   // [nq] or nullptr: 0, or the status of a refused query
  const uint32_t *changed;  // nullptr, or the group's word: nonzero = its bitmap changed while the call read it
  uint64_t *keys;           // [nq][k]: the running top-k between node chunks, ascending, KEY_NONE padded
  uint32_t k;
  uint32_t first, last;  // the first node chunk starts empty; the last one writes the row
  uint32_t *out_ids;     // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
};

// One wave64 per position; the row of the table goes by the position, the exclude, the refusal and the key scratch by
// the query.  A batch of the row is one ballot against the current k-th key (PhExactTopK::insert) and most batches end
// there once the list is full.  A refused query gets the empty row and its status.
__global__ __launch_bounds__(64) void ph_table_select_kernel(PhTableSelectArgs a) {
  extern __shared__ uint64_t select_keys[];  // ph_dense_select_lds(k)
  const uint32_t lane = threadIdx.x;
  const uint32_t changed = a.changed && a.changed[0] ? PH_GROUP_ST_CHANGED : ST_OK;
  for (uint32_t p = blockIdx.x; p < a.npos; p += gridDim.x) {
    const uint32_t q = a.order ? a.order[p] : a.pos_first + p;  // < nq <= 2^32 - 1
    __syncthreads();  // the previous position's lists are done with
    PhExactTopK top;
    top.init(select_keys, a.k);
    uint64_t *const mine = a.keys + (uint64_t)q * a.k;
    const uint32_t why = a.refuse ? a.refuse[q] : ST_OK;
    const uint32_t refused = why ? why : changed;
    if (!a.first) top.load(mine, lane);
    if (!refused)
      top.insert_row(a.D + (uint64_t)p * a.stride, a.list, a.tn, a.exclude ? a.exclude[q] : PH_EMPTY32, lane);
    if (a.last) {
      ph_exact_write_row(a, q, top.cur, refused ? 0u : top.len, false, lane);
      if (lane == 0 && refused) a.status[q] = refused;  // 4, 6 or 7 after the row writer's 0, same lane
    } else {
      ph_exact_store_list(mine, top.cur, top.len, a.k, lane);
    }
  }
}

// ------------------------------------------------------------------ a call's scratch

// A PhCallSet (call_set.h) of the index's `denses` pool.  Of `ws` only the tiny_* operand fields are used (tiny_table's
// packed operands and their key): the search launches' workspaces, with their mutex and alternation, are not touched.
struct PhDenseSet : PhCallSet {
  void *pre = nullptr;  // sized before the count is known (dense_plan.h)
  size_t pre_bytes = 0;
  void *post = nullptr;  // key scratch + table
  size_t post_bytes = 0;
  uint32_t *h_head = nullptr;  // pinned: the count and the list's length as the host reads them
  PhWorkspace ws;
};

// the request, checked; device pointers of the caller
struct PhDenseCall {
  const float *queries;  // [nq][ldq], or nullptr: Stored queries (qids)
  uint32_t ldq;
  const uint32_t *qids, *exclude;  // [nq] or nullptr
  uint64_t nq;
  const uint32_t *filter;  // one bitmap; nullptr: every vector of the index
  uint32_t k;
  uint32_t *out_ids;  // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
  hipStream_t stream;
};

namespace {

int select_launch(const PhTableRun &r, const PhTableSelectArgs &a) {
  hipLaunchKernelGGL(ph_table_select_kernel, dim3(std::min<uint32_t>(a.npos, 1u << 20)), dim3(64),
                     (size_t)ph_dense_select_lds(r.k), r.stream, a);
  PH_HIP(hipGetLastError());
  return 0;
}

// the orchestration on a set the caller holds; c is checked, nq > 0
int dense_run(const phnsw_index *ix, const PhDenseCall &c, PhDenseSet &set) {
  const phnsw_store *s = ix->store;
  const uint64_t nq = c.nq, nwords = ph_exact_words(s->n);
  PH_TRY(set.ready());
  if (!set.h_head) PH_HIP(hipHostMalloc((void **)&set.h_head, PH_DENSE_HEAD_WORDS * 4u, hipHostMallocDefault));
  const uint32_t lcap = ph_dense_list_cap(ix);
  PH_TRY(set.block_ensure(&set.pre, &set.pre_bytes, (size_t)ph_dense_pre_words(nwords, lcap, nq) * 4u, c.stream));

  StepTimes times;  // pack and table are one figure: both are enqueued inside tiny_table
  times.on = env_ll("PHNSW_DENSE_TIMES") > 0, times.stream = c.stream;
  PhDenseList l;
  PH_TRY(ph_dense_list_enqueue(ix, c.filter, c.qids, nq, (uint32_t *)set.pre, &times, 0, 1, c.stream, &l));
  uint32_t *const head = l.head, *const list = l.list, *const safe = l.safe, *const refuse = l.refuse;
  PH_HIP(hipMemcpyAsync(set.h_head, head, 8, hipMemcpyDeviceToHost, c.stream));
  PH_HIP(hipStreamSynchronize(c.stream));  // the one synchronisation: the table's shape depends on the count
  const uint64_t cand = set.h_head[1];
  if (cand != set.h_head[0] || cand > lcap) {
    ph_set_error("exact shared search: the bitmap changed while the call read it (%u candidates counted, %u listed)",
                 set.h_head[0], set.h_head[1]);
    return PHNSW_E_INVALID;
  }

  PhTableRun r = {};
  r.queries = c.queries, r.ldq = c.ldq, r.qids = c.qids ? safe : nullptr, r.npos = nq, r.list = list, r.cand = cand;
  r.exclude = c.exclude, r.refuse = c.qids ? refuse : nullptr, r.k = c.k;
  r.out_ids = c.out_ids, r.out_d = c.out_d, r.out_len = c.out_len, r.status = c.status;
  r.stream = c.stream, r.times = &times, r.step_table = 2, r.step_select = 3;
  r.verbose_prefix = "exact shared table: ", r.call = "exact shared search";
  if (cand) {
    r.nodes_knob = ph_dense_nodes_knob(env_ll("PHNSW_DENSE_NODES"));
    r.bytes_knob = ph_dense_bytes_knob(env_ll("PHNSW_DENSE_TABLE_BYTES"));
    const PhDensePlan plan = ph_dense_plan(cand, nq, r.nodes_knob, r.bytes_knob);
    PH_TRY(set.block_ensure(&set.post, &set.post_bytes, (size_t)ph_dense_post_bytes(plan, c.k), c.stream));
    r.keys = (uint64_t *)set.post, r.D = (float *)((char *)set.post + ph_dense_key_bytes(nq, c.k));
  }
  if (!cand) times.on = false;  // empty rows (and the status of a Stored query id at or past n): nothing timed or printed
  PH_TRY(ph_table_run(ix, set.ws, r));
  if (!cand) return 0;
  float ms[4];
  if (times.collect(ms, 4))
    fprintf(stderr, "[phnsw] exact_shared: %llu queries x %llu candidates: count %.3f ms, list %.3f ms, pack+table %.3f ms, select %.3f ms\n",
            (unsigned long long)nq, (unsigned long long)cand, ms[0], ms[1], ms[2], ms[3]);
  return 0;
}

}  // namespace

// Node chunks x position chunks of one run (phnsw_internal.h): the table of a chunk (ph_tiny_table_chunk), then its
// select; without candidates the select alone, over no table.  The packed node operand is kept under the list's ADDRESS
// and length, not its contents, and the list is scratch that runs and rounds reuse: the key is dropped per run and per
// node chunk, so the operand serves the position chunks of one node chunk and nothing else.
int ph_table_run(const phnsw_index *ix, PhWorkspace &ws, const PhTableRun &r) {
  PhTableSelectArgs a = {};
  a.exclude = r.exclude, a.refuse = r.refuse, a.changed = r.changed, a.keys = r.keys, a.k = r.k;
  a.out_ids = r.out_ids, a.out_d = r.out_d, a.out_len = r.out_len, a.status = r.status;
  ws.tiny_pack_key.valid = false;
  if (r.cand == 0) {
    a.order = r.order ? r.order + r.first : nullptr, a.pos_first = (uint32_t)r.first, a.npos = (uint32_t)r.npos;
    a.first = 1u, a.last = 1u;
    r.times->begin(r.step_select);
    PH_TRY(select_launch(r, a));
    r.times->end();
    return 0;
  }
  const PhDensePlan plan = ph_dense_plan(r.cand, r.npos, r.nodes_knob, r.bytes_knob);
  a.D = r.D;
  const bool verbose = getenv("PHNSW_VERBOSE") != nullptr;
  for (uint32_t i = 0; i < plan.node_chunks; i++) {
    uint64_t nfirst;
    ph_dense_node_chunk(plan, i, &nfirst, &a.tn, &a.stride);
    a.list = r.list + nfirst;  // nfirst + tn <= cand
    a.first = i == 0 ? 1u : 0u, a.last = i + 1u == plan.node_chunks ? 1u : 0u;
    ws.tiny_pack_key.valid = false;
    for (uint64_t j = 0; j < plan.pos_chunks; j++) {
      uint64_t pfirst;
      ph_dense_pos_chunk(plan, j, &pfirst, &a.npos);
      const uint64_t at = r.first + pfirst;
      a.order = r.order ? r.order + at : nullptr, a.pos_first = (uint32_t)at;
      // with an order the table kernels address the whole batch's queries by it, without one the chunk's own
      const float *const queries = r.queries && !r.order ? r.queries + at * r.ldq : r.queries;
      const uint32_t *const qids = r.qids && !r.order ? r.qids + at : r.qids;
      bool kept = false;
      r.times->begin(r.step_table);
      const int trc = ph_tiny_table_chunk(ix, ws, queries, r.ldq, qids, a.order, a.npos, a.list, a.tn, r.D, r.stream, &kept);
      r.times->end();
      if (trc > 0) {
        ph_set_error("%s: no device memory for the table's operands (%u positions x %u candidates)", r.call, a.npos, a.tn);
        return PHNSW_E_HIP;
      }
      if (trc) return trc;
      if (verbose)
        fprintf(stderr, "[phnsw] %snode chunk %u/%u (%u ids), positions %llu..+%u, %s, node operand %s\n", r.verbose_prefix, i + 1u,
                plan.node_chunks, a.tn, (unsigned long long)pfirst, a.npos, ws.tiny_table_g ? "matrix cores" : "vector units",
                kept ? "kept" : "packed");
      r.times->begin(r.step_select);
      PH_TRY(select_launch(r, a));
      r.times->end();
    }
  }
  return 0;
}

// the checks every entry point makes (filter_grouped.hip's too) before it looks at another argument: index, k, store kind and row length
int ph_dense_check(const phnsw_index *ix, uint64_t k, const char *call) {
  if (ix) PH_TRY(ph_bits_unsupported(ix->store, call));  // a bits store has the plain walk alone
  if (!ix || ix->layers.empty()) {
    ph_set_error("%s: null index or index without layers", call);
    return PHNSW_E_INVALID;
  }
  if (!ph_exact_k_valid(k)) {
    ph_set_error("%s: k must be 1..1024 (got %llu)", call, (unsigned long long)k);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  if (ph_store_pq(s) || ph_store_pq_shared(s)) {
    ph_set_error("%s: a distance table needs row vectors, not a %s store; phnsw_search_exact_filtered scans a PQ store", call,
                 ph_rows_name(s->kind));
    return PHNSW_E_UNSUPPORTED;
  }
  if (!ph_chunk_count(s->ld / 4)) {
    ph_set_error("%s: rows of %u floats are longer than the 1536 the table kernels take; phnsw_search_exact_filtered has no "
                 "such limit on its own", call, s->ld);
    return PHNSW_E_UNSUPPORTED;
  }
  return 0;
}

void ph_dense_free(phnsw_index *ix) {
  ph_sets_free<PhDenseSet>(ix->denses, [](PhDenseSet &s) {
    if (s.pre) ph_pool_free(s.pre);
    if (s.post) ph_pool_free(s.post);
    if (s.h_head) hipHostFree(s.h_head);
    ph_tiny_free(s.ws);
  });
}

// ------------------------------------------------------------------ C ABI

extern "C" int phnsw_exact_shared_supported(const phnsw_index *ix, uint64_t k) try {
  return ph_dense_check(ix, k, "phnsw_exact_shared_supported");
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_shared_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                                                const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                                const uint32_t *filter_dev, uint64_t k, uint32_t *out_ids_dev,
                                                float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev,
                                                void *stream) try {
  const char *const call = "phnsw_search_exact_shared_device";
  PH_TRY(ph_dense_check(ix, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      nq > 0xFFFFFFFFull) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; queries need ldq >= store ld, multiple of 4, "
                 "16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhDenseCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq;
  c.filter = filter_dev ? filter_dev : ix->default_filter;  // phnsw_index_set_filter_device
  c.k = (uint32_t)k;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  phnsw_index *mix = const_cast<phnsw_index *>(ix);
  PhDenseSet *set = ph_set_acquire<PhDenseSet>(mix->denses);
  PhSetGuard guard{mix->denses, set, c.stream};
  return dense_run(ix, c, *set);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_exact_shared(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                                         const uint64_t *exclude, const uint32_t *filter, uint64_t k, uint64_t *out_ids,
                                         float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_search_exact_shared";
  PH_TRY(ph_dense_check(ix, k, call));
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!out_ids || !out_d || !out_len || nq > 0xFFFFFFFFull) {
    ph_set_error("search: invalid argument (queries or ids, outputs, k <= number_of_candidates)");  // the scan's host form
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, "search"));
  phnsw_index *mix = const_cast<phnsw_index *>(ix);
  PhDenseSet *set = ph_set_acquire<PhDenseSet>(mix->denses);
  PhHostCall h(mix->denses, set);
  PH_TRY(h.stage_in(s, queries, qids, exclude, nq, 0, 0, (uint32_t)k, (uint32_t)k));
  PhDenseCall c = {};
  h.fill(c);
  if (filter) {
    const size_t words = (size_t)ph_exact_words(s->n);
    uint32_t *f = nullptr;
    PH_TRY(h.blocks.alloc(&f, words * 4u));
    PH_HIP(hipMemcpyAsync(f, filter, words * 4u, hipMemcpyHostToDevice, h.st));
    c.filter = f;
  } else {
    c.filter = ix->default_filter;  // phnsw_index_set_filter_device: device words
  }
  c.k = (uint32_t)k;
  PH_TRY(dense_run(ix, c, *set));
  return h.finish(out_ids, out_d, out_len);  // the ids were checked: every status is 0
} catch (...) { return ph_caught(); }
