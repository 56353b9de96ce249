// One filtered search that picks its method per query (phnsw_search_filtered_auto[_device]): the exact scan of the
// allow-list (filter_exact.hip) where few rows are allowed, the graph walk with a strict post-filter (search.hip) where
// many are, and the scan again for every query whose walk came back short.  Every row then holds exactly
// min(k, candidates) entries and never an id that is not a candidate.  The rule is filter_route.h's.
//
//   1. ph_filter_count          candidates per bitmap
//   2. ph_auto_route_kernel     route[q]; the graph list and the scan list, ascending, their lengths in device words
//      -- the host reads the two lengths (first synchronisation)
//   3. ph_search_device         order = the graph list: strict rows [nq][ef] in scratch, addressed by the original q
//   4. ph_auto_finish_kernel    exclude[q] dropped, k entries copied out; short rows appended to the scan list
//      -- the host reads the scan list's length (second synchronisation; neither happens without a graph list)
//   5. ph_exact_device          list = the scan list: routed and short queries in ONE launch, after the walk
//
// The search kernels and the scan's arithmetic are untouched: a scanned row is phnsw_search_exact_filtered's row bit
// for bit, a graph row is the strict row of phnsw_search_batch_filtered.
//
// A call describes its candidates by bitmaps or BY LABEL (phnsw_search_labeled_auto[_device]: a phnsw_labels handle and
// want[q]).  The five steps and the two kernels are the same; only where a step gets its facts differs:
//   1. the counts are the lengths of the posting lists (ph_labels_count), no bitmap is counted
//   3. the walk is the search kernels' label mode over the handle's column
//   4. "exclude[q] is a candidate" is label_of[exclude[q]] == want[q]
//   5. the scan is filter_labeled.hip's, over the scan list (PhLabeledCall::list)
// ... or BY A SET OF LABELS (phnsw_search_labelset_auto[_device]: the handle, want_first and want_values):
//   1. the counts are ph_labels_count_set's: the lists of the distinct labels of the range, and 0 for a query the scan by
//      set refuses (a range that is not sound, a pair a lower query holds) -- so it is routed to the scan, which reports it
//   3. the walk is the search kernels' set mode
//   4. "exclude[q] is a candidate" is ph_auto_set_candidate, the membership predicate of the walk
//   5. the scan is the subset form of the scan by set (PhLabelsetCall with a list): its claim runs over the whole batch
// ... or BY A NUMERIC RANGE (phnsw_search_ranged_auto[_device]: a phnsw_attr handle, lo[q] and hi[q]):
//   1. the counts are the lengths of the spans (ph_attr_count): no bitmap is made or counted
//   3. the walk is the search kernels' range mode over the handle's column
//   4. "exclude[q] is a candidate" is ph_auto_range_candidate, the predicate of the walk
//   5. the scan is filter_ranged.hip's, over the scan list (PhRangedCall::list)
// ... or BY A LABEL AND A NUMERIC RANGE (phnsw_search_label_ranged_auto[_device]: a phnsw_label_attr handle, want[q], lo[q]
// and hi[q]):
//   1. the counts are the lengths of the spans (ph_label_attr_count): no bitmap is made or counted
//   3. the walk is the search kernels' label-range mode over the handle's column
//   4. "exclude[q] is a candidate" is ph_auto_pair_candidate, the predicate of the walk (ph_pair_holds)
//   5. the scan is filter_label_ranged.hip's, over the scan list (PhLabelRangedCall::list)
// ... or BY A SET OF LABELS AND A NUMERIC RANGE (phnsw_search_labelset_ranged_auto[_device]: a phnsw_label_attr handle,
// want_first, want_values, lo[q] and hi[q]):
//   1. the counts are ph_label_attr_count_set's: the spans of the distinct labels of the range, and 0 for a query the scan
//      refuses (a range that is not sound, a pair a lower query holds) -- so it is routed to the scan, which reports it
//   3. the walk is the search kernels' set-range mode over the handle's column
//   4. "exclude[q] is a candidate" is ph_auto_pairset_candidate, the predicate of the walk (ph_pairset_holds)
//   5. the scan is the subset form of the scan by set and range (PhLabelsetRangedCall with a list): its claim runs over
//      the whole batch
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "filter_candidate.h"
#include "filter_route.h"
#include "host_call.h"
#include "phnsw_device.h"

static_assert(PH_ROUTE_GRAPH == PHNSW_ROUTE_GRAPH && PH_ROUTE_SCAN == PHNSW_ROUTE_SCAN &&
                  PH_ROUTE_GRAPH_THEN_SCAN == PHNSW_ROUTE_GRAPH_THEN_SCAN,
              "filter_route.h and phnsw.h name the same routes");

struct PhAutoArgs {
  uint32_t nq, n, k, ef;
  uint64_t scan_below;
  const uint32_t *qids, *exclude;  // [nq] or nullptr
  const uint32_t *filter;          // nullptr: every vector of the index
  uint32_t filter_stride;          // 0 = one bitmap for all
  uint32_t per_query;              // counts holds nq entries, else one
  const uint32_t *label_of, *want;  // a call by label: the handle's column [n] and want [nq]; else nullptr
  // a call by set: the column, want == nullptr and the table (graph-list queries have sound ranges: their counts are not 0)
  const uint32_t *set_first, *set_values;
  // a call by range: the handle's column [n] and the bounds [nq]; else nullptr
  const uint32_t *attr_of, *range_lo, *range_hi;
  // a call by label and range: the handle's column [n], the labels and the bounds [nq]; else nullptr
  const uint64_t *pair_of;
  const uint32_t *pair_want, *pair_lo, *pair_hi;
  // the index's bottom layer, as the candidate test takes it
  uint32_t n_nodes;
  const uint32_t *nodes, *vec2node;
  // the call's scratch (filter_route.h)
  uint32_t *head;          // [0] length of the graph list, [1] of the scan list
  const uint32_t *counts;  // candidates per bitmap
  uint32_t *glist, *slist, *route;
  const uint32_t *walk_ids;  // [nq][ef]: the strict rows of the graph list's queries
  const float *walk_d;
  const uint32_t *walk_len;
  uint32_t *out_ids;  // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;
};

// One workgroup walks the batch 256 queries at a time: the rule per query, a ballot per wave and a scan over the four
// waves' counts give every query its place, so both lists come out ascending.
__global__ __launch_bounds__(256) void ph_auto_route_kernel(PhAutoArgs a) {
  __shared__ uint32_t wave_g[4], wave_s[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t lt = lanemask_lt(lane);
  uint32_t gbase = 0, sbase = 0;  // entries of the two lists so far: the same in every thread
  for (uint64_t base = 0; base < a.nq; base += 256u) {
    const uint64_t q64 = base + threadIdx.x;
    const bool valid = q64 < a.nq;
    const uint32_t q = (uint32_t)q64;
    uint32_t r = PH_ROUTE_SCAN;
    if (valid) {
      r = ph_auto_route(a.counts[a.per_query ? q : 0u], a.scan_below, a.ef, a.k, a.n_nodes);
      // a Stored query id at or past n has no row to walk from: the scan reports it (status 4, an empty row)
      if (a.qids && a.qids[q] >= a.n) r = PH_ROUTE_SCAN;
      a.route[q] = r;
    }
    const uint64_t gm = __ballot(valid && r == PH_ROUTE_GRAPH), sm = __ballot(valid && r == PH_ROUTE_SCAN);
    if (lane == 0) wave_g[wave] = (uint32_t)__popcll(gm), wave_s[wave] = (uint32_t)__popcll(sm);
    __syncthreads();
    uint32_t goff = gbase, soff = sbase, gtot = 0, stot = 0;
    for (uint32_t w = 0; w < 4u; w++) {
      if (w < wave) goff += wave_g[w], soff += wave_s[w];
      gtot += wave_g[w], stot += wave_s[w];
    }
    if (valid) {  // goff + rank < gbase + gtot <= nq, and so for the scan list
      if (r == PH_ROUTE_GRAPH)
        a.glist[goff + (uint32_t)__popcll(gm & lt)] = q;
      else
        a.slist[soff + (uint32_t)__popcll(sm & lt)] = q;
    }
    gbase += gtot, sbase += stot;
    __syncthreads();  // the counts are rewritten by the next 256
  }
  if (threadIdx.x == 0) a.head[0] = gbase, a.head[1] = sbase;
}

// One wave per query of the graph list: its strict row without exclude[q], cut to k and padded, into the caller's
// row; a row shorter than the candidates allow moves its query to the scan list (route 2), and so does a walk whose
// spill list overflowed (status 5: the scan needs none).  Any other status stays, with an empty row.
__global__ __launch_bounds__(64) void ph_auto_finish_kernel(PhAutoArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint64_t lt = lanemask_lt(lane);
  const uint32_t nlim = ph_exact_id_limit(a.n, a.n_nodes, a.nodes, a.vec2node);
  const uint32_t glen = min(a.head[0], a.nq);
  for (uint32_t i = blockIdx.x; i < glen; i += gridDim.x) {
    const uint32_t q = a.glist[i];  // < nq: the route kernel wrote it
    const uint32_t st = a.status[q];
    const uint32_t len = st == ST_OK ? min(a.walk_len[q], a.ef) : 0u;
    const uint32_t ex = a.exclude ? a.exclude[q] : PH_EMPTY32;
    uint32_t kept = 0;
    for (uint32_t b = 0; b < len && kept < a.k; b += 64u) {
      const uint32_t j = b + lane;
      const uint32_t id = j < len ? a.walk_ids[(uint64_t)q * a.ef + j] : PH_EMPTY32;
      const bool keep = id != PH_EMPTY32 && id != ex;
      const uint64_t km = __ballot(keep);
      const uint32_t to = kept + (uint32_t)__popcll(km & lt);
      if (keep && to < a.k) {
        a.out_ids[(uint64_t)q * a.k + to] = id;
        a.out_d[(uint64_t)q * a.k + to] = a.walk_d[(uint64_t)q * a.ef + j];
      }
      kept += (uint32_t)__popcll(km);
    }
    kept = min(kept, a.k);
    for (uint32_t j = kept + lane; j < a.k; j += 64u) {
      a.out_ids[(uint64_t)q * a.k + j] = PH_EMPTY32;
      a.out_d[(uint64_t)q * a.k + j] = PH_FMAX;
    }
    if (lane == 0) {
      const uint32_t *const bitmap = a.filter ? a.filter + (uint64_t)q * a.filter_stride : nullptr;
      bool ex_cand;
      if (a.pair_of && a.set_first)
        ex_cand = ph_auto_pairset_candidate(a.pair_of, a.n, a.set_first[q], a.set_first[q + 1u], a.set_values, a.pair_lo[q], a.pair_hi[q],
                                            ex, 0xFFFFFFFFFFFFFFFFull);
      else if (a.pair_of)
        ex_cand = ph_auto_pair_candidate(a.pair_of, a.n, a.pair_want[q], a.pair_lo[q], a.pair_hi[q], ex, 0xFFFFFFFFFFFFFFFFull);
      else if (a.attr_of)
        ex_cand = ph_auto_range_candidate(a.attr_of, a.n, a.range_lo[q], a.range_hi[q], ex, PHNSW_ATTR_NONE);
      else if (a.set_first)
        ex_cand = ph_auto_set_candidate(a.label_of, a.n, a.set_first[q], a.set_first[q + 1u], a.set_values, ex, PHNSW_LABEL_NONE);
      else if (a.label_of)
        ex_cand = ph_auto_label_candidate(a.label_of, a.n, a.want[q], ex, PHNSW_LABEL_NONE);
      else
        ex_cand = ph_exact_is_candidate(bitmap, ex, nlim, a.vec2node);
      const uint32_t e = (ex != PH_EMPTY32 && ex_cand) ? 1u : 0u;
      const uint32_t full = ph_auto_full_len(a.counts[a.per_query ? q : 0u], e, a.k);
      if (st == ST_OVERFLOW || (st == ST_OK && kept < full)) {
        const uint32_t at = atomicAdd(&a.head[1], 1u);  // < nq: q was in the graph list, not in this one
        if (at < a.nq) a.slist[at] = q;
        a.route[q] = PH_ROUTE_GRAPH_THEN_SCAN;  // the scan writes the row, its length and the status
      } else {
        a.out_len[q] = kept;
      }
    }
  }
}

// ------------------------------------------------------------------ a call's scratch

// A PhCallSet (call_set.h) of the index's `autos` pool.
struct PhAutoSet : PhCallSet {
  void *block = nullptr;
  size_t bytes = 0;
  uint32_t *h_head = nullptr;  // pinned: the list lengths as the host reads them
};

namespace {

// the orchestration on a set the caller holds; c is checked
int auto_run(const phnsw_index *ix, const PhAutoCall &c, PhAutoSet &set) {
  const phnsw_store *s = ix->store;
  const uint64_t nq = c.nq;
  const uint32_t ef = (uint32_t)c.sp->number_of_candidates;
  const bool by_label = c.labels != nullptr, by_set = by_label && c.want_first != nullptr;
  const bool by_range = c.attr != nullptr;
  const bool by_pair = c.label_attr != nullptr, by_pairset = by_pair && c.want_first != nullptr;
  const bool per_query = by_label || by_range || by_pair || (c.filter.words && c.filter.stride != 0u);
  PH_TRY(set.ready());
  if (!set.h_head) PH_HIP(hipHostMalloc((void **)&set.h_head, PH_AUTO_HEAD_WORDS * 4u, hipHostMallocDefault));
  // (a call by set: the claim's owner words [nwant] behind everything else)
  const uint64_t words = ph_auto_scratch_words(nq, per_query, ef);
  PH_TRY(set.block_ensure(&set.block, &set.bytes, (size_t)(words + (by_set || by_pairset ? c.nwant : 0u)) * 4u, c.stream));
  const uint64_t nb = ph_auto_bitmaps(nq, per_query);
  uint32_t *const head = (uint32_t *)set.block, *const counts = head + PH_AUTO_HEAD_WORDS, *const glist = counts + nb;
  uint32_t *const slist = glist + ph_auto_list_words(nq), *const route_own = slist + ph_auto_list_words(nq);
  uint32_t *const walk_len = route_own + nq, *const walk_ids = walk_len + nq;
  float *const walk_d = (float *)(walk_ids + nq * ef);

  if (by_pairset)
    PH_TRY(ph_label_attr_count_set(c.label_attr, c.want_first, c.want_values, c.pair_lo, c.pair_hi, nq, c.nwant, counts, head + words,
                                   c.stream));
  else if (by_pair)
    PH_TRY(ph_label_attr_count(c.label_attr, c.pair_want, c.pair_lo, c.pair_hi, nq, counts, c.stream));
  else if (by_range)
    PH_TRY(ph_attr_count(c.attr, c.range_lo, c.range_hi, nq, counts, c.stream));
  else if (by_set)
    PH_TRY(ph_labels_count_set(c.labels, c.want_first, c.want_values, nq, c.nwant, counts, head + words, c.stream));
  else if (by_label)
    PH_TRY(ph_labels_count(c.labels, c.want, nq, counts, c.stream));
  else
    PH_TRY(ph_filter_count(ix, c.filter, nb, counts, c.stream));
  PhAutoArgs a = {};
  a.nq = (uint32_t)nq, a.n = (uint32_t)s->n, a.k = c.k, a.ef = ef;
  a.scan_below = by_pairset ? ph_auto_scan_below_labelset_ranged(c.scan_below)
                 : by_pair  ? ph_auto_scan_below_label_ranged(c.scan_below)
                 : by_range ? ph_auto_scan_below_ranged(c.scan_below)
                 : by_set ? ph_auto_scan_below_labelset(c.scan_below)
                        : (by_label ? ph_auto_scan_below_labeled(c.scan_below) : ph_auto_scan_below(c.scan_below, per_query));
  a.qids = c.qids, a.exclude = c.exclude;
  PhFilter filter = c.filter;  // what the walk gets
  if (by_label) {
    filter = PhFilter{};
    filter.label_of = a.label_of = ph_labels_column(c.labels), filter.want = a.want = c.want;
    if (by_set) {
      filter.want = a.want = nullptr;
      filter.set_first = a.set_first = c.want_first, filter.set_values = a.set_values = c.want_values;
      filter.set_nwant = (uint32_t)c.nwant;
    }
  }
  if (by_range) {
    filter = PhFilter{};
    filter.attr_of = a.attr_of = ph_attr_column(c.attr);
    filter.range_lo = a.range_lo = c.range_lo, filter.range_hi = a.range_hi = c.range_hi;
  }
  if (by_pair) {
    filter = PhFilter{};
    filter.pair_of = a.pair_of = ph_label_attr_column(c.label_attr);
    filter.pair_want = a.pair_want = c.pair_want, filter.pair_lo = a.pair_lo = c.pair_lo, filter.pair_hi = a.pair_hi = c.pair_hi;
    if (by_pairset) {  // (graph-list queries have sound ranges: their counts are not 0)
      filter.pair_want = a.pair_want = nullptr;
      filter.set_first = a.set_first = c.want_first, filter.set_values = a.set_values = c.want_values;
      filter.set_nwant = (uint32_t)c.nwant;
    }
  }
  a.filter = filter.words, a.filter_stride = filter.words ? filter.stride : 0u, a.per_query = per_query ? 1u : 0u;
  ph_exact_bottom_layer(ix, &a.n_nodes, &a.nodes, &a.vec2node);
  a.head = head, a.counts = counts, a.glist = glist, a.slist = slist, a.route = c.out_route ? c.out_route : route_own;
  a.walk_ids = walk_ids, a.walk_d = walk_d, a.walk_len = walk_len;
  a.out_ids = c.out_ids, a.out_d = c.out_d, a.out_len = c.out_len, a.status = c.status;
  hipLaunchKernelGGL(ph_auto_route_kernel, dim3(1), dim3(256), 0, c.stream, a);
  PH_HIP(hipGetLastError());
  PH_HIP(hipMemcpyAsync(set.h_head, head, 8, hipMemcpyDeviceToHost, c.stream));
  PH_HIP(hipStreamSynchronize(c.stream));
  const uint64_t glen = std::min<uint64_t>(set.h_head[0], nq);
  uint64_t slen = std::min<uint64_t>(set.h_head[1], nq);

  if (glen) {
    PhSearchCall w = {};
    w.queries = c.queries, w.ldq = c.ldq, w.qids = c.qids, w.exclude = c.exclude;
    w.nq = glen, w.order = glist;  // positions of the list; the kernels address everything by the query index it holds
    w.sp = c.sp;
    w.filter = filter, w.filter.flags = PHNSW_FILTER_STRICT;
    w.out_ids = walk_ids, w.out_d = walk_d, w.out_len = walk_len, w.status = c.status;
    w.stream = c.stream;
    PH_TRY(ph_search_device(ix, w));
    hipLaunchKernelGGL(ph_auto_finish_kernel, dim3((uint32_t)std::min<uint64_t>(glen, 1u << 16)), dim3(64), 0, c.stream, a);
    PH_HIP(hipGetLastError());
    PH_HIP(hipMemcpyAsync(set.h_head + 1, head + 1, 4, hipMemcpyDeviceToHost, c.stream));
    PH_HIP(hipStreamSynchronize(c.stream));
    slen = std::min<uint64_t>(set.h_head[1], nq);
  }
  if (slen && by_pairset) {
    PhLabelsetRangedCall sx = {};
    PhLabelRangedCall &x = sx.c;
    x.queries = c.queries, x.ldq = c.ldq, x.qids = c.qids, x.exclude = c.exclude, x.lo = c.pair_lo, x.hi = c.pair_hi;
    x.nq = slen, x.list = slist;
    x.k = c.k;
    x.out_ids = c.out_ids, x.out_d = c.out_d, x.out_len = c.out_len, x.status = c.status;
    x.stream = c.stream;
    sx.want_first = c.want_first, sx.want_values = c.want_values, sx.nwant = c.nwant, sx.batch_nq = nq;
    PH_TRY(ph_labelset_ranged_device(ix, c.label_attr, sx));
  } else if (slen && by_pair) {
    PhLabelRangedCall x = {};
    x.queries = c.queries, x.ldq = c.ldq, x.qids = c.qids, x.exclude = c.exclude;
    x.want = c.pair_want, x.lo = c.pair_lo, x.hi = c.pair_hi;
    x.nq = slen, x.list = slist;
    x.k = c.k;
    x.out_ids = c.out_ids, x.out_d = c.out_d, x.out_len = c.out_len, x.status = c.status;
    x.stream = c.stream;
    PH_TRY(ph_label_ranged_device(ix, c.label_attr, x));
  } else if (slen && by_range) {
    PhRangedCall x = {};
    x.queries = c.queries, x.ldq = c.ldq, x.qids = c.qids, x.exclude = c.exclude, x.lo = c.range_lo, x.hi = c.range_hi;
    x.nq = slen, x.list = slist;
    x.k = c.k;
    x.out_ids = c.out_ids, x.out_d = c.out_d, x.out_len = c.out_len, x.status = c.status;
    x.stream = c.stream;
    PH_TRY(ph_ranged_device(ix, c.attr, x));
  } else if (slen && by_set) {
    PhLabelsetCall sx = {};
    PhLabeledCall &x = sx.c;
    x.queries = c.queries, x.ldq = c.ldq, x.qids = c.qids, x.exclude = c.exclude;
    x.nq = slen, x.list = slist;
    x.k = c.k;
    x.out_ids = c.out_ids, x.out_d = c.out_d, x.out_len = c.out_len, x.status = c.status;
    x.stream = c.stream;
    sx.want_first = c.want_first, sx.want_values = c.want_values, sx.nwant = c.nwant, sx.batch_nq = nq;
    PH_TRY(ph_labelset_device(ix, c.labels, sx));
  } else if (slen && by_label) {
    PhLabeledCall x = {};
    x.queries = c.queries, x.ldq = c.ldq, x.qids = c.qids, x.exclude = c.exclude, x.want = c.want;
    x.nq = slen, x.list = slist;
    x.k = c.k;
    x.out_ids = c.out_ids, x.out_d = c.out_d, x.out_len = c.out_len, x.status = c.status;
    x.stream = c.stream;
    PH_TRY(ph_labeled_device(ix, c.labels, x));
  } else if (slen) {
    PhExactCall x = {};
    x.queries = c.queries, x.ldq = c.ldq, x.qids = c.qids, x.exclude = c.exclude;
    x.nq = slen, x.list = slist;
    x.filter = c.filter, x.filter.flags = 0u;
    x.k = c.k;
    x.out_ids = c.out_ids, x.out_d = c.out_d, x.out_len = c.out_len, x.status = c.status;
    x.stream = c.stream;
    PH_TRY(ph_exact_device(ix, x));
  }
  return 0;
}

// the checks both entry points make before they look at a pointer: index, parameters, k, store kind
int auto_check(const phnsw_index *ix, const phnsw_search_params *sp, uint64_t k, const char *call) {
  if (ix) PH_TRY(ph_bits_unsupported(ix->store, call));  // a bits store has the plain walk alone
  PH_TRY(ph_check_sp(ix, sp));
  if (!ph_auto_k_valid(k, sp->number_of_candidates)) {
    ph_set_error("%s: k must be 1..number_of_candidates (got %llu, number_of_candidates %llu)", call, (unsigned long long)k,
                 (unsigned long long)sp->number_of_candidates);
    return PHNSW_E_INVALID;
  }
  PH_TRY(ph_exact_check(ix, k, call));  // a shared-codebook PQ store
  return ph_exact_supported(ix, (uint32_t)k);
}

}  // namespace

void ph_auto_free(phnsw_index *ix) {
  ph_sets_free<PhAutoSet>(ix->autos, [](PhAutoSet &s) {
    if (s.block) ph_pool_free(s.block);
    if (s.h_head) hipHostFree(s.h_head);
  });
}

int ph_auto_device(const phnsw_index *ix, const PhAutoCall &c) {
  if (c.nq == 0) return 0;
  phnsw_index *mix = const_cast<phnsw_index *>(ix);
  PhAutoSet *set = ph_set_acquire<PhAutoSet>(mix->autos);
  PhSetGuard guard{mix->autos, set, c.stream};
  return auto_run(ix, c, *set);
}

// ------------------------------------------------------------------ C ABI

extern "C" int phnsw_search_filtered_auto_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                                                 const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                                 const uint32_t *exclude_dev, const uint32_t *filter_dev,
                                                 uint32_t filter_stride_words, uint64_t k, uint64_t scan_below,
                                                 uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                 uint32_t *out_route_dev, uint32_t *status_dev, void *stream) try {
  const char *const call = "phnsw_search_filtered_auto_device";
  PH_TRY(auto_check(ix, sp, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !ph_auto_nq_valid(nq)) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; queries need ldq >= store ld, multiple of 4, "
                 "16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhAutoCall c = {};
  PH_TRY(ph_filter_check(ix, filter_dev, filter_stride_words, 0u, call, &c.filter));
  if (!c.filter.words) c.filter.words = ix->default_filter;  // phnsw_index_set_filter_device
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq, c.sp = sp;
  c.k = (uint32_t)k, c.scan_below = scan_below;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.out_route = out_route_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_auto_device(ix, c);
} catch (...) { return ph_caught(); }

// the host form of the three descriptions; lb != nullptr: by label (want: host words [nq]; filter unused) or, with
// want_first, by set (want_first [nq + 1], want_values: host words; want unused), else by bitmap; at != nullptr: by range
// (range_lo, range_hi: host words [nq]; lb and filter unused); la != nullptr: by label and range (pair_want, range_lo,
// range_hi: host words [nq]; lb, at and filter unused)
static int auto_host(const char *call, const phnsw_index *ix, const phnsw_labels *lb, const float *queries, const uint64_t *qids,
                     uint64_t nq, const phnsw_search_params *sp, const uint64_t *exclude, const uint32_t *filter,
                     uint32_t filter_stride_words, const uint32_t *want, const uint32_t *want_first, const uint32_t *want_values,
                     uint64_t k, uint64_t scan_below, uint64_t *out_ids, float *out_d, uint64_t *out_len, uint32_t *out_route,
                     const phnsw_attr *at = nullptr, const uint32_t *range_lo = nullptr, const uint32_t *range_hi = nullptr,
                     const phnsw_label_attr *la = nullptr, const uint32_t *pair_want = nullptr) {
  const bool by_set = (lb || la) && want_first;  // with la: by set and range (pair_want unused)
  if (la && ((!pair_want && !want_first) || !range_lo || !range_hi || nq > 0x7FFFFFFEull)) {
    ph_set_error("%s: invalid argument (want%s, lo and hi; nq < 2^31 - 1)", call, want_first ? "_first" : "");
    return PHNSW_E_INVALID;
  }
  if (at && (!range_lo || !range_hi || nq > 0x7FFFFFFEull)) {
    ph_set_error("%s: invalid argument (lo and hi; nq < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  if (!ph_auto_queries_valid(queries != nullptr, qids != nullptr) || !out_ids || !out_d || !out_len || !ph_auto_nq_valid(nq) ||
      (lb && ((!want && !want_first) || nq > 0x7FFFFFFEull))) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs%s)", call, lb ? "; want; nq < 2^31 - 1" : "");
    return PHNSW_E_INVALID;
  }
  const uint64_t nwant = by_set ? want_first[nq] : 0u;
  if (by_set && ((!want_values && nwant) || nwant > 0x7FFFFFFEull)) {
    ph_set_error("%s: invalid argument (want_values unless want_first[nq] is 0; want_first[nq] < 2^31 - 1)", call);
    return PHNSW_E_INVALID;
  }
  PhFilter hf = {};
  if (!lb && !at && !la) PH_TRY(ph_filter_check(ix, filter, filter_stride_words, 0u, call, &hf));
  const phnsw_store *s = ix->store;
  if (by_set) {  // as the walk and the scan by set refuse them: naming the call and the query
    PH_TRY(ph_stored_ids_check(qids, nq, s->n, call, true));
    for (uint64_t q = 0; q < nq; q++)
      if ((q == 0 && want_first[0] != 0u) || want_first[q] > want_first[q + 1u]) {
        ph_set_error("%s: query %llu: want_first must start at 0 and never run backwards (want_first[%llu] = %u, "
                     "want_first[%llu] = %u)", call, (unsigned long long)q, (unsigned long long)q, want_first[q],
                     (unsigned long long)q + 1u, want_first[q + 1u]);
        return PHNSW_E_INVALID;
      }
  } else {
    PH_TRY(ph_stored_ids_check(qids, nq, s->n, "search"));
  }
  PH_HIP(hipSetDevice(s->device));
  phnsw_index *mix = const_cast<phnsw_index *>(ix);
  PhAutoSet *set = ph_set_acquire<PhAutoSet>(mix->autos);
  PhHostCall h(mix->autos, set);
  // extras: route | want, or for a call by set want_first [nq + 1] | want_values [nwant], or for a call by range lo | hi, or for a call by
  // label and range want | lo | hi, or for a call by set and range want_first [nq + 1] | want_values [nwant] | lo | hi
  PH_TRY(h.stage_in(s, queries, qids, exclude, nq, (size_t)nq * 4u + (by_set ? 1u + (size_t)nwant : 0u), 1, (uint32_t)k, (uint32_t)k));
  PhAutoCall c = {};
  h.fill(c);
  c.filter = hf;
  if (la && by_set) {  // the description of a call by set and range: 4 * (nq + 1) + 4 * nwant + 8 * nq bytes
    uint32_t *const first_dev = h.extra() + nq, *const values_dev = first_dev + nq + 1u, *const lo_dev = values_dev + nwant;
    uint32_t *const hi_dev = lo_dev + nq;
    PH_HIP(hipMemcpyAsync(first_dev, want_first, (size_t)(nq + 1u) * 4u, hipMemcpyHostToDevice, h.st));
    if (nwant) PH_HIP(hipMemcpyAsync(values_dev, want_values, (size_t)nwant * 4u, hipMemcpyHostToDevice, h.st));
    PH_HIP(hipMemcpyAsync(lo_dev, range_lo, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
    PH_HIP(hipMemcpyAsync(hi_dev, range_hi, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
    c.label_attr = la, c.pair_lo = lo_dev, c.pair_hi = hi_dev;
    c.want_first = first_dev, c.want_values = values_dev, c.nwant = nwant;
  } else if (la) {  // the description of a call by label and range: 12 bytes per query
    uint32_t *const want_dev = h.extra() + nq, *const lo_dev = want_dev + nq, *const hi_dev = lo_dev + nq;
    PH_HIP(hipMemcpyAsync(want_dev, pair_want, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
    PH_HIP(hipMemcpyAsync(lo_dev, range_lo, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
    PH_HIP(hipMemcpyAsync(hi_dev, range_hi, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
    c.label_attr = la, c.pair_want = want_dev, c.pair_lo = lo_dev, c.pair_hi = hi_dev;
  } else if (at) {  // the description of a call by range: 8 bytes per query
    uint32_t *const lo_dev = h.extra() + nq, *const hi_dev = lo_dev + nq;
    PH_HIP(hipMemcpyAsync(lo_dev, range_lo, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
    PH_HIP(hipMemcpyAsync(hi_dev, range_hi, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
    c.attr = at, c.range_lo = lo_dev, c.range_hi = hi_dev;
  } else if (by_set) {  // the description of a call by set: 4 * (nq + 1) + 4 * nwant bytes
    uint32_t *const first_dev = h.extra() + nq, *const values_dev = first_dev + nq + 1u;
    PH_HIP(hipMemcpyAsync(first_dev, want_first, (size_t)(nq + 1u) * 4u, hipMemcpyHostToDevice, h.st));
    if (nwant) PH_HIP(hipMemcpyAsync(values_dev, want_values, (size_t)nwant * 4u, hipMemcpyHostToDevice, h.st));
    c.labels = lb, c.want_first = first_dev, c.want_values = values_dev, c.nwant = nwant;
  } else if (lb) {  // the description of a call by label: 4 bytes per query
    uint32_t *const want_dev = h.extra() + nq;
    PH_HIP(hipMemcpyAsync(want_dev, want, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
    c.labels = lb, c.want = want_dev;
  } else if (hf.words) {  // whole strides, as phnsw_search_batch_filtered copies them
    const size_t words = hf.stride ? (size_t)nq * hf.stride : (size_t)((s->n + 31u) / 32u);
    uint32_t *f = nullptr;
    PH_TRY(h.blocks.alloc(&f, words * 4u));
    PH_HIP(hipMemcpyAsync(f, hf.words, words * 4u, hipMemcpyHostToDevice, h.st));
    c.filter.words = f;
  } else {
    c.filter.words = ix->default_filter;  // phnsw_index_set_filter_device: device words
  }
  c.sp = sp, c.k = (uint32_t)k, c.scan_below = scan_below, c.out_route = h.extra();
  PH_TRY(auto_run(ix, c, *set));
  PH_TRY(h.finish(out_ids, out_d, nullptr));
  for (uint64_t i = 0; i < nq; i++) {
    if (h.status(i) != 0u) {  // the ids were checked: what is left is the walk's own failure
      ph_set_error("search: a candidate vector is missing from a lower layer (layers not nested, lib.rs:261)");
      return PHNSW_E_MISSING_NODE;
    }
    out_len[i] = h.len(i);
    if (out_route) out_route[i] = h.read_extra(0, i);
  }
  return 0;
}

extern "C" int phnsw_search_filtered_auto(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                                          const phnsw_search_params *sp, const uint64_t *exclude, const uint32_t *filter,
                                          uint32_t filter_stride_words, uint64_t k, uint64_t scan_below, uint64_t *out_ids,
                                          float *out_d, uint64_t *out_len, uint32_t *out_route) try {
  const char *const call = "phnsw_search_filtered_auto";
  PH_TRY(auto_check(ix, sp, k, call));
  if (nq == 0) return 0;
  return auto_host(call, ix, nullptr, queries, qids, nq, sp, exclude, filter, filter_stride_words, nullptr, nullptr, nullptr, k,
                   scan_below, out_ids, out_d, out_len, out_route);
} catch (...) { return ph_caught(); }

// ---- by label

extern "C" int phnsw_search_labeled_auto(const phnsw_index *ix, const phnsw_labels *lb, const float *queries, const uint64_t *qids,
                                         uint64_t nq, const phnsw_search_params *sp, const uint64_t *exclude,
                                         const uint32_t *want, uint64_t k, uint64_t scan_below, uint64_t *out_ids, float *out_d,
                                         uint64_t *out_len, uint32_t *out_route) try {
  const char *const call = "phnsw_search_labeled_auto";
  PH_TRY(auto_check(ix, sp, k, call));
  PH_TRY(ph_labeled_check(ix, lb, k, call));
  if (nq == 0) return 0;
  return auto_host(call, ix, lb, queries, qids, nq, sp, exclude, nullptr, 0u, want, nullptr, nullptr, k, scan_below, out_ids,
                   out_d, out_len, out_route);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_labeled_auto_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev,
                                                uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                const phnsw_search_params *sp, const uint32_t *exclude_dev,
                                                const uint32_t *want_dev, uint64_t k, uint64_t scan_below, uint32_t *out_ids_dev,
                                                float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_route_dev,
                                                uint32_t *status_dev, void *stream) try {
  const char *const call = "phnsw_search_labeled_auto_device";
  PH_TRY(auto_check(ix, sp, k, call));
  PH_TRY(ph_labeled_check(ix, lb, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !want_dev || !ph_auto_nq_valid(nq) || nq > 0x7FFFFFFEull) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; want; queries need ldq >= store ld, multiple "
                 "of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhAutoCall c = {};
  c.labels = lb, c.want = want_dev;
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq, c.sp = sp;
  c.k = (uint32_t)k, c.scan_below = scan_below;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.out_route = out_route_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_auto_device(ix, c);
} catch (...) { return ph_caught(); }

// ---- by a set of labels

extern "C" int phnsw_search_labelset_auto(const phnsw_index *ix, const phnsw_labels *lb, const float *queries, const uint64_t *qids,
                                          uint64_t nq, const phnsw_search_params *sp, const uint64_t *exclude,
                                          const uint32_t *want_first, const uint32_t *want_values, uint64_t k, uint64_t scan_below,
                                          uint64_t *out_ids, float *out_d, uint64_t *out_len, uint32_t *out_route) try {
  const char *const call = "phnsw_search_labelset_auto";
  PH_TRY(auto_check(ix, sp, k, call));
  PH_TRY(ph_labeled_check(ix, lb, k, call));
  if (nq == 0) return 0;
  if (!want_first) {
    ph_set_error("%s: invalid argument (want_first)", call);
    return PHNSW_E_INVALID;
  }
  return auto_host(call, ix, lb, queries, qids, nq, sp, exclude, nullptr, 0u, nullptr, want_first, want_values, k, scan_below,
                   out_ids, out_d, out_len, out_route);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_labelset_auto_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev,
                                                 uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                 const phnsw_search_params *sp, const uint32_t *exclude_dev,
                                                 const uint32_t *want_first_dev, const uint32_t *want_values_dev, uint64_t nwant,
                                                 uint64_t k, uint64_t scan_below, uint32_t *out_ids_dev, float *out_d_dev,
                                                 uint32_t *out_len_dev, uint32_t *out_route_dev, uint32_t *status_dev,
                                                 void *stream) try {
  const char *const call = "phnsw_search_labelset_auto_device";
  PH_TRY(auto_check(ix, sp, k, call));
  PH_TRY(ph_labeled_check(ix, lb, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !want_first_dev || (!want_values_dev && nwant)) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; want_first; want_values unless nwant is 0; "
                 "queries need ldq >= store ld, multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  if (nq > 0x7FFFFFFEull || nwant > 0x7FFFFFFEull) {
    ph_set_error("%s: nq and nwant must be below 2^31 - 1", call);
    return PHNSW_E_INVALID;
  }
  PhAutoCall c = {};
  c.labels = lb, c.want_first = want_first_dev, c.want_values = want_values_dev, c.nwant = nwant;
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq, c.sp = sp;
  c.k = (uint32_t)k, c.scan_below = scan_below;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.out_route = out_route_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_auto_device(ix, c);
} catch (...) { return ph_caught(); }

// ---- by a numeric range

extern "C" int phnsw_search_ranged_auto(const phnsw_index *ix, const phnsw_attr *at, const float *queries, const uint64_t *qids,
                                        uint64_t nq, const phnsw_search_params *sp, const uint64_t *exclude, const uint32_t *lo,
                                        const uint32_t *hi, uint64_t k, uint64_t scan_below, uint64_t *out_ids, float *out_d,
                                        uint64_t *out_len, uint32_t *out_route) try {
  const char *const call = "phnsw_search_ranged_auto";
  PH_TRY(auto_check(ix, sp, k, call));
  PH_TRY(ph_ranged_check(ix, at, k, call));
  if (nq == 0) return 0;
  return auto_host(call, ix, nullptr, queries, qids, nq, sp, exclude, nullptr, 0u, nullptr, nullptr, nullptr, k, scan_below, out_ids,
                   out_d, out_len, out_route, at, lo, hi);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_ranged_auto_device(const phnsw_index *ix, const phnsw_attr *at, const float *queries_dev, uint32_t ldq,
                                               const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                               const uint32_t *exclude_dev, const uint32_t *lo_dev, const uint32_t *hi_dev,
                                               uint64_t k, uint64_t scan_below, uint32_t *out_ids_dev, float *out_d_dev,
                                               uint32_t *out_len_dev, uint32_t *out_route_dev, uint32_t *status_dev,
                                               void *stream) try {
  const char *const call = "phnsw_search_ranged_auto_device";
  PH_TRY(auto_check(ix, sp, k, call));
  PH_TRY(ph_ranged_check(ix, at, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !lo_dev || !hi_dev || !ph_auto_nq_valid(nq) || nq > 0x7FFFFFFEull) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; lo and hi; queries need ldq >= store ld, "
                 "multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhAutoCall c = {};
  c.attr = at, c.range_lo = lo_dev, c.range_hi = hi_dev;
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq, c.sp = sp;
  c.k = (uint32_t)k, c.scan_below = scan_below;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.out_route = out_route_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_auto_device(ix, c);
} catch (...) { return ph_caught(); }

// ---- by a label and a numeric range

extern "C" int phnsw_search_label_ranged_auto(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries,
                                              const uint64_t *qids, uint64_t nq, const phnsw_search_params *sp,
                                              const uint64_t *exclude, const uint32_t *want, const uint32_t *lo, const uint32_t *hi,
                                              uint64_t k, uint64_t scan_below, uint64_t *out_ids, float *out_d, uint64_t *out_len,
                                              uint32_t *out_route) try {
  const char *const call = "phnsw_search_label_ranged_auto";
  PH_TRY(auto_check(ix, sp, k, call));
  PH_TRY(ph_label_ranged_check(ix, h, k, call));
  if (nq == 0) return 0;
  return auto_host(call, ix, nullptr, queries, qids, nq, sp, exclude, nullptr, 0u, nullptr, nullptr, nullptr, k, scan_below, out_ids,
                   out_d, out_len, out_route, nullptr, lo, hi, h, want);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_label_ranged_auto_device(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries_dev,
                                                     uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                     const phnsw_search_params *sp, const uint32_t *exclude_dev,
                                                     const uint32_t *want_dev, const uint32_t *lo_dev, const uint32_t *hi_dev,
                                                     uint64_t k, uint64_t scan_below, uint32_t *out_ids_dev, float *out_d_dev,
                                                     uint32_t *out_len_dev, uint32_t *out_route_dev, uint32_t *status_dev,
                                                     void *stream) try {
  const char *const call = "phnsw_search_label_ranged_auto_device";
  PH_TRY(auto_check(ix, sp, k, call));
  PH_TRY(ph_label_ranged_check(ix, h, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !want_dev || !lo_dev || !hi_dev || !ph_auto_nq_valid(nq) || nq > 0x7FFFFFFEull) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; want, lo and hi; queries need ldq >= store ld, "
                 "multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhAutoCall c = {};
  c.label_attr = h, c.pair_want = want_dev, c.pair_lo = lo_dev, c.pair_hi = hi_dev;
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq, c.sp = sp;
  c.k = (uint32_t)k, c.scan_below = scan_below;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.out_route = out_route_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_auto_device(ix, c);
} catch (...) { return ph_caught(); }

// ---- by a set of labels and a numeric range

extern "C" int phnsw_search_labelset_ranged_auto(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries,
                                                 const uint64_t *qids, uint64_t nq, const phnsw_search_params *sp,
                                                 const uint64_t *exclude, const uint32_t *want_first, const uint32_t *want_values,
                                                 const uint32_t *lo, const uint32_t *hi, uint64_t k, uint64_t scan_below,
                                                 uint64_t *out_ids, float *out_d, uint64_t *out_len, uint32_t *out_route) try {
  const char *const call = "phnsw_search_labelset_ranged_auto";
  PH_TRY(auto_check(ix, sp, k, call));
  PH_TRY(ph_label_ranged_check(ix, h, k, call));
  if (nq == 0) return 0;
  if (!want_first) {
    ph_set_error("%s: invalid argument (want_first)", call);
    return PHNSW_E_INVALID;
  }
  return auto_host(call, ix, nullptr, queries, qids, nq, sp, exclude, nullptr, 0u, nullptr, want_first, want_values, k, scan_below,
                   out_ids, out_d, out_len, out_route, nullptr, lo, hi, h, nullptr);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_labelset_ranged_auto_device(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries_dev,
                                                        uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                                        const phnsw_search_params *sp, const uint32_t *exclude_dev,
                                                        const uint32_t *want_first_dev, const uint32_t *want_values_dev,
                                                        uint64_t nwant, const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t k,
                                                        uint64_t scan_below, uint32_t *out_ids_dev, float *out_d_dev,
                                                        uint32_t *out_len_dev, uint32_t *out_route_dev, uint32_t *status_dev,
                                                        void *stream) try {
  const char *const call = "phnsw_search_labelset_ranged_auto_device";
  PH_TRY(auto_check(ix, sp, k, call));
  PH_TRY(ph_label_ranged_check(ix, h, k, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !out_ids_dev || !out_d_dev || !out_len_dev || !status_dev ||
      !want_first_dev || (!want_values_dev && nwant) || !lo_dev || !hi_dev) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; outputs; want_first; want_values unless nwant is 0; lo and "
                 "hi; queries need ldq >= store ld, multiple of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  if (nq > 0x7FFFFFFEull || nwant > 0x7FFFFFFEull) {
    ph_set_error("%s: nq and nwant must be below 2^31 - 1", call);
    return PHNSW_E_INVALID;
  }
  PhAutoCall c = {};
  c.label_attr = h, c.pair_lo = lo_dev, c.pair_hi = hi_dev;
  c.want_first = want_first_dev, c.want_values = want_values_dev, c.nwant = nwant;
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq, c.sp = sp;
  c.k = (uint32_t)k, c.scan_below = scan_below;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.out_route = out_route_dev, c.status = status_dev;
  c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_auto_device(ix, c);
} catch (...) { return ph_caught(); }
