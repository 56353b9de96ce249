// What the exact scans over a LIST of row ids share -- a label's posting list (filter_labeled.hip), the span of a range
// in a sorted attribute column (filter_ranged.hip): the scan loop of one wave over one slice of one list, the merge of
// the slices' lists, the scratch set kept with a handle and its acquire, and the run of a host walk once it is staged.
#pragma once
#include <hip/hip_runtime.h>

#include "exact_topk.h"
#include "filter_candidate.h"
#include "host_call.h"
#include "label_plan.h"
#include "phnsw_device.h"

// One wave64, one (position, slice): the batches of the slice of list[0 .. len), 64 ids at a time into dist.batch of the
// store's policy, every candidate but exclude[q] into the running top-k, and what is left of it written as
// ph_exact_write_slice writes it.  dist is prepared for query q (not for a bad one, whose len is 0); keys: the wave's
// [2k + 64] LDS.  A: the kernel's argument block (dist, exclude, k, slices, scratch and the outputs).
template <bool PAIRS, class Dist, class A>
__device__ __forceinline__ void ph_list_scan(const A &a, Dist &dist, uint64_t *keys, const uint32_t *list, uint32_t len,
                                             uint32_t q, uint32_t pos, uint32_t slice, bool bad_query, uint32_t lane) {
  PhExactTopK top;
  top.init(keys, a.k);
  const uint32_t ex = a.exclude ? a.exclude[q] : PH_EMPTY32;
  uint64_t b0, b1;
  ph_label_slice_range(slice, a.slices, len, &b0, &b1);
  for (uint64_t b = b0; b < b1; b++) {
    const uint32_t j = (uint32_t)b * PH_LABEL_BATCH + lane;
    const bool ok = j < len;
    const uint32_t id = ok ? list[j] : 0u;  // a listed id: a row of the store
    const float d = dist.batch(a.dist, __ballot(ok), id, lane);
    top.insert(ok && id != ex ? mkkey(d, id) : KEY_NONE, lane);
  }
  ph_exact_write_slice<PAIRS>(a, q, pos, slice, top.cur, top.len, bad_query, lane);
}

// One wave per position: the slices' ascending lists merged through the same running top-k (PH_EXACT_FEED).  A: nq
// positions, order[pos] the query of a position, scratch [nq][slices][k].
template <class A>
__global__ __launch_bounds__(64) void ph_list_merge_kernel(A a) {
  extern __shared__ float list_merge_lds[];
  const uint32_t lane = threadIdx.x;
  uint64_t *const keys = (uint64_t *)list_merge_lds;
  for (uint32_t pos = blockIdx.x; pos < a.nq; pos += gridDim.x) {
    const uint32_t q = a.order[pos];
    __syncthreads();
    PhExactTopK top;
    top.init(keys, a.k);
    for (uint32_t s = 0; s < a.slices; s++)
      PH_EXACT_FEED(top, a.scratch + ((uint64_t)pos * a.slices + s) * a.k, a.k, lane);
    ph_exact_write_row(a, q, top.cur, top.len, !a.queries && a.qids[q] >= a.n, lane);
  }
}

// A PhCallSet (call_set.h) kept with a HANDLE (phnsw_labels, phnsw_attr), not the index.
struct PhLabeledSet : PhCallSet {
  void *pre = nullptr, *tmp = nullptr, *keys = nullptr;
  size_t pre_bytes = 0, tmp_bytes = 0, keys_bytes = 0;
  uint64_t tmp_nq = 0;  // the batch size tmp_need was asked of hipCUB for (0: none yet)
  size_t tmp_need = 0;
  // the exact radius search over lists (filter_list_radius.hip): the record pool in radius_plan.h's layout, and the
  // pinned word the total is read back into
  void *post = nullptr;
  size_t post_bytes = 0;
  uint64_t *h_total = nullptr;
};

const size_t PH_LABEL_SETS = 4;  // scratch sets a handle makes before calls share one behind its event

// own_stream: the host form, which runs on the set's own stream (`stream` is then ignored)
static inline PhLabeledSet *ph_handle_set_acquire(PhCallPool &pool, hipStream_t stream, bool own_stream) {
  // First a set whose last call ran on this very stream: stream order already protects it, so back-to-back calls on one
  // stream share one set however far the device is behind.  Then a set whose last call has finished.  Then, while fewer
  // than PH_LABEL_SETS exist, a new one, so that calls on different streams overlap; past that a free set whose event
  // the call's stream waits for.  A handle so holds at most max(PH_LABEL_SETS, calls inside the library at once) sets,
  // each as large as the largest call it served, until the handle is destroyed.
  std::lock_guard<std::mutex> g(pool.mutex);
  if (!own_stream)
    for (PhCallSet *s : pool.sets)
      if (!s->in_use && !s->stream && s->has_last && s->last == stream) {
        s->in_use = true;
        return static_cast<PhLabeledSet *>(s);
      }
  PhCallSet *busy = nullptr;
  for (PhCallSet *s : pool.sets) {
    if (s->in_use) continue;
    if (!s->done || hipEventQuery(s->done) == hipSuccess) {
      s->in_use = true;
      return static_cast<PhLabeledSet *>(s);
    }
    busy = s;
  }
  (void)hipGetLastError();  // hipErrorNotReady of the query is no error of the call
  if (busy && pool.sets.size() >= PH_LABEL_SETS) {
    busy->in_use = true;
    return static_cast<PhLabeledSet *>(busy);
  }
  PhLabeledSet *s = new PhLabeledSet();
  s->in_use = true;
  pool.sets.push_back(s);
  return s;
}
static inline void ph_handle_sets_free(PhCallPool &pool) {
  ph_sets_free<PhLabeledSet>(pool, [](PhLabeledSet &s) {
    if (s.pre) ph_pool_free(s.pre);
    if (s.tmp) ph_pool_free(s.tmp);
    if (s.keys) ph_pool_free(s.keys);
    if (s.post) ph_pool_free(s.post);
    if (s.h_total) hipHostFree(s.h_total);
  });
}

// the key of a vector as a handle lists it -- its value, or NONE (PHNSW_LABEL_NONE and PHNSW_ATTR_NONE are one word)
// where the vector is not listed -- and the values of the construction's sort.  (A kernel of the header: each unit
// launches its own copy; filter_label_ranged.hip writes composites and launches none.)
[[maybe_unused]] static __global__ __launch_bounds__(256) void ph_label_key_kernel(const uint32_t *labels, uint32_t n,
                                                                                   uint32_t n_nodes, const uint32_t *nodes,
                                                                                   const uint32_t *vec2node, uint32_t *keys,
                                                                                   uint32_t *iota) {
  const uint32_t nlim = ph_exact_id_limit(n, n_nodes, nodes, vec2node);
  for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < n; v += (uint64_t)gridDim.x * 256u) {
    const bool listed = v < nlim && (!vec2node || vec2node[v] != PH_EMPTY32);
    keys[v] = listed ? labels[v] : PHNSW_LABEL_NONE;
    iota[v] = (uint32_t)v;
  }
}

// The snapshot test every call by a handle makes (ix has layers): the handle was made for this index as it stands.
// `what`: "labels" or "attribute" in the message.  filter_labeled.hip
int ph_snapshot_fresh(const phnsw_index *ix, bool present, const phnsw_index *h_ix, uint64_t h_n, uint32_t h_nodes, const char *what,
                      const char *call);

// The run of a host walk (by label, by set, by range) once everything is staged: filter_labeled.hip
int ph_walk_host_run(const phnsw_index *ix, PhHostCall &h, PhSearchCall &c, uint32_t *redo_dev, uint32_t ef, uint64_t *out_ids,
                     float *out_d, uint64_t *out_len, uint64_t *out_stats);
