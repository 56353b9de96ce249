// Exact top-k over ONE allow-list shared by the whole batch, as a distance table (phnsw_search_exact_shared[_device]):
// with a shared bitmap every query meets the same candidate rows, so the work is a queries x rows table -- the work
// tiny.hip already does for the dense top layers -- and not the per-query scan of filter_exact.hip.
//
//   1. ph_filter_count          candidates of the one bitmap
//   2. ph_dense_popc_kernel     candidates per bitmap word (ph_exact_word: the scan's own candidate test, no exclude)
//      ph_dense_prefix_kernel   their exclusive prefix over the ceil(n / 32) words; the total is the list's length
//      ph_dense_list_kernel     every word writes its ids at its offset: the ascending VectorId list of the candidates
//      -- the host reads the length c (the one synchronisation); c == 0 writes empty rows and returns
//   3. ph_dense_qids_kernel     Stored queries: ids at or past n replaced by 0 and flagged (the pack kernel reads rows
//                               unchecked); the select reports them, status 4 and an empty row, as the scan does
//   4. per node chunk, per position chunk (dense_plan.h): ph_tiny_table_chunk (tiny.hip) -- the existing table
//      kernels, the per-hop bits -- into D[positions][stride]
//   5. ph_dense_select_kernel   one wave64 per position: the running top-k of (distance, id) keys over the chunk's row
//                               of D, carried between node chunks in a [nq][k] key scratch; after the last node chunk
//                               the row is written
//
// The keys are distinct, so the k smallest are one set in one order whatever the chunk sizes; the distances are the
// table's, i.e. phnsw_distance_batch's bits, so a row equals phnsw_search_exact_filtered's row bit for bit.
// The table kernels, their pack / quant kernels and the scan are untouched (profiles/filter_dense/).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dense_plan.h"
#include "exact_slices.h"
#include "exact_topk.h"
#include "filter_candidate.h"
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

// One workgroup walks the counts 1024 at a time and leaves their exclusive prefix in place: a shuffle scan per wave,
// the 16 waves' totals through LDS, the running base in every thread.  The total is at most n <= 2^31 - 1.
__global__ __launch_bounds__(1024) void ph_dense_prefix_kernel(PhDenseListArgs a) {
  __shared__ uint32_t wave_total[16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t base = 0;
  for (uint64_t at = 0; at < a.nwords; at += 1024u) {
    const uint64_t w = at + threadIdx.x;
    const uint32_t v = w < a.nwords ? a.off[w] : 0u;
    uint32_t incl = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const uint32_t t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    if (lane == 63u) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = base, all = 0;
    for (uint32_t i = 0; i < 16u; i++) {
      if (i < wave) before += wave_total[i];
      all += wave_total[i];
    }
    if (w < a.nwords) a.off[w] = before + incl - v;
    base += all;
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
// with candidates when this runs into a table) and its flag is set
__global__ __launch_bounds__(256) void ph_dense_qids_kernel(const uint32_t *qids, uint64_t nq, uint32_t n, uint32_t *safe,
                                                            uint32_t *flags) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * 256u) {
    const uint32_t v = qids[q];
    safe[q] = v < n ? v : 0u;
    flags[q] = v < n ? 0u : 1u;
  }
}

// ------------------------------------------------------------------ the select

struct PhDenseSelectArgs {
  const float *D;          // [npos][stride]: the table of this (node chunk, position chunk); unread when tn == 0
  uint32_t stride, tn;     // tn <= stride
  uint32_t npos, pos_first;  // positions of this chunk; position p is query pos_first + p
  const uint32_t *list;    // [tn]: the node chunk's VectorIds, ascending
  const uint32_t *exclude;  // [nq] or nullptr
  const uint32_t *flags;    // [nq] or nullptr: a Stored query id at or past n
  uint64_t *keys;           // [nq][k]: the running top-k between node chunks, ascending, KEY_NONE padded
  uint32_t k;
  uint32_t first, last;  // the first node chunk starts empty; the last one writes the row
  uint32_t *out_ids;     // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
};

// One wave64 per position.  The row of D is read 64 entries at a time, coalesced; a batch is one ballot against the
// current k-th key (PhExactTopK::insert) and most batches end there once the list is full.
__global__ __launch_bounds__(64) void ph_dense_select_kernel(PhDenseSelectArgs a) {
  extern __shared__ uint64_t dense_keys[];  // ph_dense_select_lds(k)
  const uint32_t lane = threadIdx.x;
  for (uint32_t p = blockIdx.x; p < a.npos; p += gridDim.x) {
    const uint32_t q = a.pos_first + p;  // < nq <= 2^32 - 1
    __syncthreads();  // the previous position's lists are done with
    PhExactTopK top;
    top.cur = dense_keys, top.nxt = dense_keys + a.k, top.sv = dense_keys + 2u * a.k, top.len = 0, top.k = a.k;
    uint64_t *const mine = a.keys + (uint64_t)q * a.k;
    const bool bad_query = a.flags && a.flags[q] != 0u;
    if (!a.first) {
      uint32_t have = 0;
      for (uint32_t i = lane; i < a.k; i += 64u) {
        const uint64_t key = mine[i];
        top.cur[i] = key;
        have += key != KEY_NONE ? 1u : 0u;
      }
#pragma unroll
      for (int sft = 32; sft >= 1; sft >>= 1) have += __shfl_xor(have, sft);
      top.len = have;  // the padding is KEY_NONE and no key is (mkkey keeps bit 31 of the id word clear)
      __syncthreads();
    }
    if (!bad_query) {
      const uint32_t ex = a.exclude ? a.exclude[q] : PH_EMPTY32;
      const float *const row = a.D + (uint64_t)p * a.stride;
      for (uint32_t b = 0; b < a.tn; b += 64u) {
        const uint32_t j = b + lane;
        const bool ok = j < a.tn;  // tn <= stride: inside the row
        const uint32_t id = ok ? a.list[j] : PH_EMPTY32;
        top.insert(ok && id != ex ? mkkey(row[j], id) : KEY_NONE, lane);
      }
    }
    if (a.last) {
      ph_exact_write_row(a, q, top.cur, top.len, bad_query, lane);
    } else {
      for (uint32_t i = lane; i < a.k; i += 64u) mine[i] = i < top.len ? top.cur[i] : KEY_NONE;
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

int select_launch(const PhDenseCall &c, PhDenseSelectArgs &a) {
  hipLaunchKernelGGL(ph_dense_select_kernel, dim3(std::min<uint32_t>(a.npos, 1u << 20)), dim3(64),
                     (size_t)ph_dense_select_lds(c.k), c.stream, a);
  PH_HIP(hipGetLastError());
  return 0;
}

// the orchestration on a set the caller holds; c is checked, nq > 0
int dense_run(const phnsw_index *ix, const PhDenseCall &c, PhDenseSet &set) {
  const phnsw_store *s = ix->store;
  const uint64_t nq = c.nq, nwords = ph_exact_words(s->n);
  // the packed operand's key describes a list that is scratch: whichever way the last call on this set ended, this one
  // writes other ids there
  set.ws.tiny_pack_key.valid = false;
  PH_TRY(set.ready());
  if (!set.h_head) PH_HIP(hipHostMalloc((void **)&set.h_head, PH_DENSE_HEAD_WORDS * 4u, hipHostMallocDefault));
  PhDenseListArgs l = {};
  l.filter = c.filter, l.n = (uint32_t)s->n, l.nwords = (uint32_t)nwords;
  ph_exact_bottom_layer(ix, &l.n_nodes, &l.nodes, &l.vec2node);
  l.cap = (uint32_t)std::min<uint64_t>(s->n, l.n_nodes);  // a candidate is a vector of the bottom layer
  PH_TRY(set.block_ensure(&set.pre, &set.pre_bytes, (size_t)ph_dense_pre_words(nwords, l.cap, nq) * 4u, c.stream));
  uint32_t *const head = (uint32_t *)set.pre, *const off = head + PH_DENSE_HEAD_WORDS, *const list = off + ph_dense_off_words(nwords);
  uint32_t *const safe = list + l.cap, *const flags = safe + nq;
  l.head = head, l.off = off, l.list = list;

  StepTimes times;  // pack and table are one figure: both are enqueued inside tiny_table
  times.on = env_ll("PHNSW_DENSE_TIMES") > 0, times.stream = c.stream;
  times.begin(0);
  PhFilter one = {c.filter, 0u, 0u};
  PH_TRY(ph_filter_count(ix, one, 1, head, c.stream));
  times.end();
  times.begin(1);
  const uint32_t wgrid = (uint32_t)std::min<uint64_t>((nwords + 255u) / 256u, 1u << 16);
  if (nwords) {
    hipLaunchKernelGGL(ph_dense_popc_kernel, dim3(wgrid), dim3(256), 0, c.stream, l);
    hipLaunchKernelGGL(ph_dense_prefix_kernel, dim3(1), dim3(1024), 0, c.stream, l);
    hipLaunchKernelGGL(ph_dense_list_kernel, dim3(wgrid), dim3(256), 0, c.stream, l);
  } else {
    PH_HIP(hipMemsetAsync(head, 0, PH_DENSE_HEAD_WORDS * 4u, c.stream));
  }
  if (c.qids)
    hipLaunchKernelGGL(ph_dense_qids_kernel, dim3((uint32_t)std::min<uint64_t>((nq + 255u) / 256u, 1u << 16)), dim3(256), 0,
                       c.stream, c.qids, nq, (uint32_t)s->n, safe, flags);
  PH_HIP(hipGetLastError());
  times.end();
  PH_HIP(hipMemcpyAsync(set.h_head, head, 8, hipMemcpyDeviceToHost, c.stream));
  PH_HIP(hipStreamSynchronize(c.stream));  // the one synchronisation: the table's shape depends on the count
  const uint64_t cand = set.h_head[1];
  if (cand != set.h_head[0] || cand > l.cap) {
    ph_set_error("exact shared search: the bitmap changed while the call read it (%u candidates counted, %u listed)",
                 set.h_head[0], set.h_head[1]);
    return PHNSW_E_INVALID;
  }

  PhDenseSelectArgs a = {};
  a.exclude = c.exclude, a.flags = c.qids ? flags : nullptr, a.k = c.k;
  a.out_ids = c.out_ids, a.out_d = c.out_d, a.out_len = c.out_len, a.status = c.status;
  if (cand == 0) {  // empty rows (and the status of a Stored query id at or past n) from the select itself
    a.npos = (uint32_t)nq, a.first = 1u, a.last = 1u;
    return select_launch(c, a);
  }
  const PhDensePlan plan = ph_dense_plan(cand, nq, ph_dense_nodes_knob(env_ll("PHNSW_DENSE_NODES")),
                                         ph_dense_bytes_knob(env_ll("PHNSW_DENSE_TABLE_BYTES")));
  PH_TRY(set.block_ensure(&set.post, &set.post_bytes, (size_t)ph_dense_post_bytes(plan, c.k), c.stream));
  a.keys = (uint64_t *)set.post;
  float *const D = (float *)((char *)set.post + ph_dense_key_bytes(nq, c.k));
  a.D = D;
  const bool verbose = getenv("PHNSW_VERBOSE") != nullptr;
  for (uint32_t i = 0; i < plan.node_chunks; i++) {
    uint64_t nfirst;
    ph_dense_node_chunk(plan, i, &nfirst, &a.tn, &a.stride);
    a.list = list + nfirst;  // nfirst + tn <= cand <= cap
    a.first = i == 0 ? 1u : 0u, a.last = i + 1u == plan.node_chunks ? 1u : 0u;
    // the packed node operand is kept under the list's ADDRESS and length, not its contents: it may serve the position
    // chunks of this node chunk and nothing else
    set.ws.tiny_pack_key.valid = false;
    for (uint64_t j = 0; j < plan.pos_chunks; j++) {
      uint64_t pfirst;
      ph_dense_pos_chunk(plan, j, &pfirst, &a.npos);
      a.pos_first = (uint32_t)pfirst;
      bool kept = false;
      times.begin(2);
      const int trc = ph_tiny_table_chunk(ix, set.ws, c.queries ? c.queries + pfirst * c.ldq : nullptr, c.ldq,
                                          c.qids ? safe + pfirst : nullptr, a.npos, a.list, a.tn, D, c.stream, &kept);
      times.end();
      if (trc > 0) {
        ph_set_error("exact shared search: no device memory for the table's operands (%u positions x %u candidates)", a.npos, a.tn);
        return PHNSW_E_HIP;
      }
      if (trc) return trc;
      if (verbose)
        fprintf(stderr, "[phnsw] exact shared table: node chunk %u/%u (%u ids), positions %llu..+%u, %s, node operand %s\n", i + 1u,
                plan.node_chunks, a.tn, (unsigned long long)pfirst, a.npos,
                set.ws.tiny_table_g ? "matrix cores" : "vector units", kept ? "kept" : "packed");
      times.begin(3);
      PH_TRY(select_launch(c, a));
      times.end();
    }
  }
  float ms[4];
  if (times.collect(ms, 4))
    fprintf(stderr, "[phnsw] exact_shared: %llu queries x %llu candidates: count %.3f ms, list %.3f ms, pack+table %.3f ms, select %.3f ms\n",
            (unsigned long long)nq, (unsigned long long)cand, ms[0], ms[1], ms[2], ms[3]);
  return 0;
}

}  // namespace

// the checks every entry point makes (filter_grouped.hip's too) before it looks at another argument: index, k, store kind and row length
int ph_dense_check(const phnsw_index *ix, uint64_t k, const char *call) {
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
  if (((!queries_dev) == (!qids_dev)) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev || nq > 0xFFFFFFFFull ||
      (queries_dev && (ldq < ix->store->ld || (ldq % 4) || ((uintptr_t)queries_dev % 16)))) {
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
