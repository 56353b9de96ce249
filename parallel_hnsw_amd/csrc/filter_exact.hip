// Exact top-k over an allow-list (phnsw_search_exact_filtered[_device], phnsw_filter_count_device): the answer to a
// SELECTIVE filter, where the graph search -- a post-filter on each layer's queue -- returns about density *
// number_of_candidates results and, at a density of 0.001, nothing.  No traversal: a wave walks its query's bitmap,
// expands the set bits to VectorIds in id order, evaluates them 64 at a time with the very call the distance batch
// makes (dist.batch of the store's policy, misc.hip: the bits are phnsw_distance_batch's by construction) and keeps a
// running top-k of (distance, id) keys in LDS.
//
//   candidates of query q = { v : v < n, bit v of q's bitmap set, v != exclude[q], v a vector of the bottom layer }
//   result                = the k candidates with the smallest (distance, id), ascending; len = min(k, candidates)
//
// The keys are distinct (the id is part of the key), so the k smallest are one set in one order: the result does not
// depend on how the bitmap is cut into slices (exact_slices.h), nor on the order in which candidates arrive.
//
// The candidate test lives in filter_candidate.h, shared with filter_auto.hip, whose routed call also scans a LIST of
// queries (PhExactCall::list): work goes by list position, everything else by the query index.  The running top-k, the
// list feed, the row writer and the block sum live in exact_topk.h, shared with filter_dense.hip, filter_grouped.hip and
// filter_labeled.hip (profiles/exact_once/).  ph_resident_waves, the launch preparation of every one-wave kernel of the
// family, is here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "exact_slices.h"
#include "exact_topk.h"
#include "filter_candidate.h"
#include "phnsw_device.h"

struct PhExactArgs {
  PhDistArgs dist;
  const float *queries;  // [nq][ldq] or nullptr
  uint32_t ldq;
  const uint32_t *qids, *exclude;  // [nq] or nullptr
  const uint32_t *filter;          // nullptr: every vector of the index
  uint32_t filter_stride;          // words from one query's bitmap to the next, 0 = one for all
  uint32_t nq, n, nwords, k, slices;
  const uint32_t *list;  // nullable: work position i is query list[i] (nq positions); scratch goes by position
  uint64_t passes;
  // the index's bottom layer: a candidate is one of its vectors
  uint32_t n_nodes;
  const uint32_t *nodes, *vec2node;  // vec2node == nullptr: identity, the vectors are 0 .. n_nodes - 1
  uint32_t pq_lds;                   // bytes of dynamic LDS in front of the scan's own: a PQ store's table (16-byte multiple)
  uint64_t *scratch;                 // slices > 1: [nq positions][slices][k] keys, each list ascending, KEY_NONE padded
  uint32_t *out_ids;                 // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
};

// One wave64 per (query, slice of the bitmap); work item = slice * nq + q (slice-major, query-minor): the waves resident
// together walk the same part of the id range, so with a shared bitmap they read the same rows and L2 can serve them.
template <class Dist>
__global__ __launch_bounds__(64) void ph_exact_scan_kernel(PhExactArgs a) {
  extern __shared__ float exact_lds[];
  const uint32_t lane = threadIdx.x;
  uint64_t *const keys = (uint64_t *)((char *)exact_lds + a.pq_lds);
  uint32_t *const stage = (uint32_t *)(keys + 2u * a.k + 64u);  // [PH_EXACT_PASS_IDS]
  const uint32_t nlim = ph_exact_id_limit(a.n, a.n_nodes, a.nodes, a.vec2node);
  const uint64_t items = (uint64_t)a.nq * a.slices;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t pos = (uint32_t)(item % a.nq), slice = (uint32_t)(item / a.nq);
    const uint32_t q = a.list ? a.list[pos] : pos;
    __syncthreads();  // the previous item's LDS (table, lists) is done with
    const bool bad_query = !a.queries && a.qids[q] >= a.n;
    Dist dist;
    if (a.queries)
      dist.prepare_raw(a.dist, a.queries + (uint64_t)q * a.ldq, exact_lds, lane);
    else if (!bad_query)
      dist.prepare_stored(a.dist, a.qids[q], exact_lds, lane);
    PhExactTopK top;
    top.init(keys, a.k);
    const uint32_t *const bitmap = a.filter ? a.filter + (uint64_t)q * a.filter_stride : nullptr;
    const uint32_t ex = a.exclude ? a.exclude[q] : PH_EMPTY32;
    uint64_t p0, p1;
    ph_exact_slice_range(slice, a.slices, a.passes, &p0, &p1);
    if (bad_query) p1 = p0;
    for (uint64_t p = p0; p < p1; p++) {
      const uint32_t widx = (uint32_t)(p * PH_EXACT_PASS_WORDS) + lane;  // p < passes <= 2^20
      uint32_t w = ph_exact_word(bitmap, widx, a.nwords, nlim, a.vec2node);
      if (ex != PH_EMPTY32 && (ex >> 5) == widx) w &= ~(1u << (ex & 31u));
      if (!__ballot(w != 0u)) continue;
      // set bits -> ids in id order: lane l's ids follow those of the lanes below it
      const uint32_t cnt = (uint32_t)__popc(w);
      const uint32_t incl = ph_wave_inclusive_sum(cnt, lane);
      const uint32_t total = rl32(incl, 63);  // <= PH_EXACT_PASS_IDS
      uint32_t o = incl - cnt;
      for (uint32_t t = w; t; t &= t - 1u) stage[o++] = widx * 32u + (uint32_t)__ffs((int)t) - 1u;  // o < incl <= total
      __syncthreads();
      for (uint32_t b = 0; b < total; b += 64u) {
        const bool ok = b + lane < total;
        const uint32_t id = ok ? stage[b + lane] : 0u;  // id < nlim <= n: a row of the store
        const float d = dist.batch(a.dist, __ballot(ok), id, lane);
        top.insert(ok ? mkkey(d, id) : KEY_NONE, lane);
      }
      __syncthreads();  // the next pass overwrites the staged ids
    }
    ph_exact_write_slice<false>(a, q, pos, slice, top.cur, top.len, bad_query, lane);
  }
}

// One wave per query: the slices' ascending lists merged through the same running top-k (PH_EXACT_FEED).
__global__ __launch_bounds__(64) void ph_exact_merge_kernel(PhExactArgs a) {
  extern __shared__ float exact_lds[];
  const uint32_t lane = threadIdx.x;
  uint64_t *const keys = (uint64_t *)exact_lds;
  for (uint32_t pos = blockIdx.x; pos < a.nq; pos += gridDim.x) {
    const uint32_t q = a.list ? a.list[pos] : pos;
    __syncthreads();
    PhExactTopK top;
    top.init(keys, a.k);
    for (uint32_t s = 0; s < a.slices; s++)
      PH_EXACT_FEED(top, a.scratch + ((uint64_t)pos * a.slices + s) * a.k, a.k, lane);
    ph_exact_write_row(a, q, top.cur, top.len, !a.queries && a.qids[q] >= a.n, lane);
  }
}

// candidates of each bitmap (no exclude): one block per bitmap, a popcount over the scan's candidate test
__global__ __launch_bounds__(256) void ph_filter_count_kernel(const uint32_t *filter, uint32_t stride, uint64_t nbitmaps,
                                                              uint32_t n, uint32_t nwords, uint32_t n_nodes,
                                                              const uint32_t *nodes, const uint32_t *vec2node,
                                                              uint32_t *out_count) {
  const uint32_t nlim = ph_exact_id_limit(n, n_nodes, nodes, vec2node);
  for (uint64_t b = blockIdx.x; b < nbitmaps; b += gridDim.x) {
    const uint32_t *const bitmap = filter ? filter + b * stride : nullptr;
    uint32_t c = 0;
    for (uint32_t widx = threadIdx.x; widx < nwords; widx += 256u)
      c += (uint32_t)__popc(ph_exact_word(bitmap, widx, nwords, nlim, vec2node));
    c = ph_block_sum256(c);
    if (threadIdx.x == 0) out_count[b] = c;
  }
}

// ------------------------------------------------------------------ launchers

typedef void (*PhExactFn)(PhExactArgs);
template <template <int, int> class D>
static PhExactFn exact_rows_fn(uint32_t nv4) {
  switch (ph_chunk_count(nv4)) {
    case 1: return ph_exact_scan_kernel<D<1, 4>>;
    case 3: return ph_exact_scan_kernel<D<3, 4>>;
    case 6: return ph_exact_scan_kernel<D<6, 4>>;
    default: return nullptr;
  }
}
static PhExactFn exact_fn(const phnsw_store *s) {
  switch (s->kind) {
    case PH_ROWS_PQ: return ph_exact_scan_kernel<DistPQ>;
    case PH_ROWS_F16: return exact_rows_fn<DistF16>(s->ld / 4);
    case PH_ROWS_I8: return exact_rows_fn<DistI8>(s->ld / 4);
    case PH_ROWS_I8Q: return exact_rows_fn<DistI8Q>(s->ld / 4);
    default: return exact_rows_fn<DistF32>(s->ld / 4);
  }
}

static const size_t PH_EXACT_LDS_MAX = 160 * 1024;  // a workgroup's LDS on gfx950

// the bottom layer of the index into the argument block
void ph_exact_bottom_layer(const phnsw_index *ix, uint32_t *n_nodes, const uint32_t **nodes, const uint32_t **vec2node) {
  const PhLayerHost &B = ix->layers.back();
  *n_nodes = B.n_nodes;
  *nodes = B.nodes;
  *vec2node = B.identity ? nullptr : B.vec2node;
}

void ph_exact_free(phnsw_index *ix) {
  for (PhExactScratch &x : ix->exact) {
    if (x.done) {
      hipEventSynchronize(x.done);
      hipEventDestroy(x.done);
    }
    if (x.keys) ph_pool_free(x.keys);
    x = PhExactScratch();
  }
}

int ph_exact_supported(const phnsw_index *ix, uint32_t k) {
  if (ix)  // (the entry points have refused a bits store by name)
    if (int brc = ph_bits_unsupported(ix->store, "exact scan")) return brc;
  const phnsw_store *s = ix->store;
  if (!exact_fn(s)) return ph_dim_unsupported(s->dim);
  const size_t pq_lds = (ph_pq_lds_bytes(s) + 15u) & ~(size_t)15u, own_lds = (size_t)ph_exact_own_lds(k);
  if (pq_lds + own_lds > PH_EXACT_LDS_MAX) {
    ph_set_error("exact filtered search: the PQ tables (%zu bytes) plus the scan's own %zu bytes of LDS at k = %u do not fit a "
                 "workgroup's %zu bytes",
                 pq_lds, own_lds, k, PH_EXACT_LDS_MAX);
    return PHNSW_E_UNSUPPORTED;
  }
  return 0;
}

// The launch preparation of a one-wave kernel with `lds` bytes of dynamic LDS: the attribute a size above 48 KiB needs
// (per call: it belongs to the kernel, not to the memo's owner) and the waves of it the device holds at once, asked of
// the runtime once per (kernel, LDS) and kept in `memo` under `mutex`.
int ph_resident_waves(PhResidentMemo &memo, std::mutex &mutex, int device, const void *fn, size_t lds, uint64_t *waves) {
  if (lds > 48 * 1024) PH_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  std::lock_guard<std::mutex> g(mutex);
  for (const PhResidentMemo::Entry &r : memo.known)
    if (r.fn == fn && r.lds == lds) {
      *waves = r.waves;
      return 0;
    }
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64, lds) != hipSuccess || per_cu <= 0) per_cu = 1;
  if (!memo.cus) PH_HIP(hipDeviceGetAttribute(&memo.cus, hipDeviceAttributeMultiprocessorCount, device));
  *waves = (uint64_t)per_cu * (uint64_t)std::max(memo.cus, 1);
  memo.known.push_back(PhResidentMemo::Entry{fn, lds, *waves});
  return 0;
}

int ph_exact_device(const phnsw_index *ix, const PhExactCall &c) {
  phnsw_index *mix = const_cast<phnsw_index *>(ix);
  const phnsw_store *s = ix->store;
  if (c.nq == 0) return 0;
  if (int rc = ph_exact_supported(ix, c.k)) return rc;
  const PhExactFn fn = exact_fn(s);
  const size_t pq_lds = (ph_pq_lds_bytes(s) + 15u) & ~(size_t)15u, own_lds = (size_t)ph_exact_own_lds(c.k);
  const size_t lds = pq_lds + own_lds;
  uint64_t resident = 0;  // waves of the scan the device holds at once
  if (int rc = ph_resident_waves(mix->exact_resident, mix->exact_mutex, s->device, (const void *)fn, lds, &resident)) return rc;
  const char *e = getenv("PHNSW_EXACT_SLICES");  // tests and tuning: forces the slice count, changes no result
  PhExactArgs a = {};
  a.dist = ph_dist_args(s);
  a.queries = c.queries, a.ldq = c.ldq, a.qids = c.qids, a.exclude = c.exclude;
  a.filter = c.filter.words, a.filter_stride = c.filter.words ? c.filter.stride : 0u;
  a.nq = (uint32_t)c.nq, a.list = c.list, a.n = (uint32_t)s->n, a.nwords = (uint32_t)ph_exact_words(s->n), a.k = c.k;
  a.passes = ph_exact_passes(s->n);
  a.slices = ph_exact_slice_count(c.nq, resident, a.passes, e ? atoll(e) : 0);
  ph_exact_bottom_layer(ix, &a.n_nodes, &a.nodes, &a.vec2node);
  a.pq_lds = (uint32_t)pq_lds;
  a.out_ids = c.out_ids, a.out_d = c.out_d, a.out_len = c.out_len, a.status = c.status;
  const uint64_t items = c.nq * (uint64_t)a.slices;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(items, 1u << 20);  // the kernels stride over what is left
  if (a.slices == 1u) {
    hipLaunchKernelGGL(fn, dim3(grid), dim3(64), lds, c.stream, a);
    PH_HIP(hipGetLastError());
    return 0;
  }
  // per-slice lists: one of the index's two scratch blocks, behind its previous user
  std::lock_guard<std::mutex> g(mix->exact_mutex);
  PhExactScratch &x = mix->exact[mix->exact_next++ & 1u];
  const size_t bytes = (size_t)items * c.k * 8u;
  if (!x.done) PH_HIP(hipEventCreateWithFlags(&x.done, hipEventDisableTiming));
  if (x.bytes < bytes) {
    if (x.keys) {
      PH_HIP(hipEventSynchronize(x.done));  // the block goes back to the pool: nothing may still write it
      ph_pool_free(x.keys);
      x.keys = nullptr, x.bytes = 0;
    }
    PH_HIP(ph_pool_alloc((void **)&x.keys, bytes));
    x.bytes = bytes;
  } else {
    PH_HIP(hipStreamWaitEvent(c.stream, x.done, 0));
  }
  a.scratch = x.keys;
  hipLaunchKernelGGL(fn, dim3(grid), dim3(64), lds, c.stream, a);
  hipLaunchKernelGGL(ph_exact_merge_kernel, dim3((uint32_t)std::min<uint64_t>(c.nq, 1u << 20)), dim3(64), own_lds, c.stream, a);
  PH_HIP(hipGetLastError());
  PH_HIP(hipEventRecord(x.done, c.stream));
  return 0;
}

int ph_filter_count(const phnsw_index *ix, const PhFilter &f, uint64_t nbitmaps, uint32_t *out_count_dev, hipStream_t stream) {
  if (nbitmaps == 0) return 0;
  const phnsw_store *s = ix->store;
  uint32_t n_nodes;
  const uint32_t *nodes, *vec2node;
  ph_exact_bottom_layer(ix, &n_nodes, &nodes, &vec2node);
  hipLaunchKernelGGL(ph_filter_count_kernel, dim3((uint32_t)std::min<uint64_t>(nbitmaps, 1u << 20)), dim3(256), 0, stream,
                     f.words, f.words ? f.stride : 0u, nbitmaps, (uint32_t)s->n, (uint32_t)ph_exact_words(s->n), n_nodes, nodes,
                     vec2node, out_count_dev);
  PH_HIP(hipGetLastError());
  return 0;
}
