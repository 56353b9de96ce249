// The search kernels (search.hip has the long form) and the functions that name their instances, for the two
// translation units that instantiate them: search.hip the kernels as they always were, search_filtered.hip their bitmap
// twins, the kernels of a search restricted to an allow-list of VectorIds, search_labeled.hip their label twins, the same
// restriction read from a label column; search_collect.hip and search_collect_labeled.hip the collecting twins of those
// two (PH_FM_COLLECT); search_labelset.hip the twins over a SET of labels per query (PH_FM_LABELSET); search_ranged.hip
// the twins over a numeric range of an attribute column per query (PH_FM_RANGE); search_label_ranged.hip the twins over a
// label and a numeric range per query (PH_FM_LABEL_RANGE); search_labelset_ranged.hip the twins over a set of labels and a
// numeric range per query (PH_FM_LABELSET_RANGE).  Nine units so that they compile side by side.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "phnsw_internal.h"

#include "filter_route.h"
#include "phnsw_device.h"

// -DPH_HOP_PROFILE: a debugging build that prints, per layer of every query, where the hops' time went
// (100 MHz ticks of s_memrealtime; each phase ends with a forced wait).  Never part of libphnsw.so proper.
#ifdef PH_HOP_PROFILE
#define PH_TICK(k)                                   \
  {                                                  \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)");   \
    const uint64_t t_now = wall_clock64();           \
    tprof[k] += t_now - t_last;                      \
    t_last = t_now;                                  \
  }
#else
#define PH_TICK(k)
#endif

// INSTR: Hnsw::search_instrumented (lib.rs:667-673).  Every visit_queue entry of the reference carries the
// index_sum of its discovery path (lib.rs:211-220: parent's sum + 1-based rank in the parent's sorted batch); the
// value returned is the index_sum of the node expanded at the last hop of the bottom layer that changed
// candidates.first() (lib.rs:225-231).  The sums ride along in a third queue array (the prefix scratch S, idle
// during the hops) and a parallel spill array; the plain kernels compile none of it.
// BIG (threshold_nn only, ph_search_kernel_big): the layer queue lives in global memory with a capacity chosen at
// launch (a.cap_max), so resize_capacity can go on doubling past what LDS holds.  The queue is then shared between
// the lanes of the wave through L2: every barrier of the body also orders and invalidates (queue_sync), and the loops
// over the queue's 64-entry chunks run to the live length instead of being unrolled CAPC times.
template <bool BIG>
__device__ __forceinline__ void queue_sync() {
  if constexpr (BIG) __threadfence();
  __syncthreads();
}

// The row-store throughput kernels (f32, f16, i8 rows alike) whose walks can get an LDS visited table (vis_table_slots: what the CU's LDS leaves a
// resident wave beside its queues, at least max(1024, 4 ef) slots): queues of 128 slots; of 256 except at <= 256
// dimensions (16 waves per CU leave under 1024 slots); of 512 at 1536 dimensions (8 waves per CU).  Every other
// kernel compiles none of the table code, which would only cost it registers (<8, DistF32<1,4>>: 125 -> 129 VGPRs,
// 4 -> 3 waves per SIMD).  The one-wave-per-SIMD latency kernels (U = 0) measured 2 % slower with the table for
// batches of 1, 64 and 1024 and keep the bitmap too.
__host__ __device__ constexpr bool vis_lds_shape(int capc, int nv) {
  return capc == 2 || (capc == 4 && nv != 1) || (capc == 8 && nv == 6);
}
template <int CAPC, class D, class = void>
struct vis_lds_policy : std::false_type {};
template <int CAPC, class D>
struct vis_lds_policy<CAPC, D, std::enable_if_t<D::ROW_STORE>>
    : std::integral_constant<bool, D::ROWS_IN_FLIGHT != 0 && vis_lds_shape(CAPC, D::CHUNKS)> {};

// The LDS visited set: slot of a NodeId (multiplicative hash, scaled to any table size)
__device__ __forceinline__ uint32_t vis_slot(uint32_t id, uint32_t slots) {
  return (uint32_t)(((uint64_t)(id * 0x9E3779B1u) * slots) >> 32);
}

// test-and-insert of one id per lane (valid lanes): true when the id was not in the table.  EMPTY = fresh,
// equal = visited, anything else = the next slot; the loop runs until every lane has resolved.  The load limit
// keeps the table from filling, so every probe sequence ends.
__device__ __forceinline__ bool vis_insert(uint32_t *H, uint32_t slots, uint32_t id, bool valid) {
  bool fresh = false, pending = valid;
  uint32_t s = valid ? vis_slot(id, slots) : 0u;
  while (__ballot(pending)) {
    if (pending) {
      const uint32_t old = atomicCAS(&H[s], PH_EMPTY32, id);
      if (old == PH_EMPTY32 || old == id) {
        fresh = old == PH_EMPTY32;
        pending = false;
      } else {
        s = s + 1u == slots ? 0u : s + 1u;
      }
    }
  }
  return fresh;
}

// FILT: the filter mode of the launch, tested where closest_vectors applies `include`.
//   PH_FM_NONE    no filter
//   PH_FM_BITMAP  an allow-list (a.filter): bit v of the query's bitmap
//   PH_FM_LABEL   a label column (a.label_of) and one wanted label per query (a.label_want): VectorId v passes iff
//                 want != PHNSW_LABEL_NONE && label_of[v] == want -- one 4-byte load where the bitmap mode loads a word.
//                 Written per lane as label_of[v] == want && label_of[v] != NONE: the same predicate, and the scalar
//                 test of `want` cost seven twins a wave per SIMD (profiles/labeled_walk)
//   PH_FM_LABELSET  the label column and a SET of wanted labels per query (a.set_first, a.set_values): VectorId v passes
//                 iff label_of[v] != PHNSW_LABEL_NONE && label_of[v] is one of set_values[first .. last), first and last
//                 the query's offsets, wave-uniform, read once per query.  The test is a loop over the set: every
//                 wave-uniform set value (a scalar load) against every lane's label -- per 64 tested ids one 4-byte load
//                 per lane and, per label of the set, one scalar load, one compare and one OR: LINEAR in the set's
//                 length, no LDS (the LDS budget decides occupancy and the visited table's size), no sort, no
//                 preparation.  In these (non-collecting) walks it runs over a layer's queue once per layer, not per
//                 evaluated row.  The offsets are not trusted: a query whose range is not sound (filter_route.h) does
//                 not walk -- ST_SET_RANGE, an empty row, stats 0 -- and nothing outside set_values[0 .. set_nwant) is
//                 read.  Never with a bitmap or label_want, and there is no collecting twin.
//   PH_FM_RANGE   an attribute column (a.attr_of) and two inclusive bounds per query (a.range_lo, a.range_hi, read once
//                 per query, wave-uniform): VectorId v passes iff lo <= attr_of[v] <= hi and attr_of[v] is a value, not
//                 PHNSW_ATTR_NONE -- one 4-byte load per lane as in the label mode, two compares.  Written per lane,
//                 ph_range_holds (filter_route.h): an empty range (lo > hi) passes nothing without a scalar test of the
//                 bounds, which is what cost the label twins a wave per SIMD.  Never with a bitmap, a label or a set,
//                 and there is no collecting twin (profiles/ranged).
//   PH_FM_LABEL_RANGE  a column of composites (a.pair_of: (label << 32) | key of a listed vector, UINT64_MAX elsewhere)
//                 and a label and two inclusive bounds per query (a.pair_want, a.pair_lo, a.pair_hi): VectorId v passes iff
//                 want << 32 | lo <= pair_of[v] <= want << 32 | hi and pair_of[v] is not UINT64_MAX -- ONE 8-byte load per
//                 lane.  Written per lane, ph_pair_holds_words (filter_route.h: ph_pair_holds word by word): lo > hi and a
//                 wanted NONE label pass nothing without a scalar test of want or the bounds (what cost the label twins a
//                 wave per SIMD).  The three words of the query are read where the test runs (rfl32: wave-uniform scalar
//                 loads at the layer tails), NOT once per query in front of the walk: held across the walk they cost
//                 ph_search_kernel_dense<2> 20 bytes of scratch that its range sibling does not use, as two aligned 64-bit
//                 bounds and as three words alike (profiles/label_ranged).  Never with a bitmap, a label, a set or a
//                 range, and there is no collecting twin.
//   PH_FM_LABELSET_RANGE  the column of composites (a.pair_of) and, per query, a SET of wanted labels (a.set_first,
//                 a.set_values, as in PH_FM_LABELSET: offsets read once per query, not trusted, ST_SET_RANGE for a range
//                 that is not sound) and ONE inclusive range shared by the set's labels (a.pair_lo, a.pair_hi): VectorId v
//                 passes iff the label word of pair_of[v] is one of set_values[first .. last), its key word lies inside
//                 [lo, hi] and pair_of[v] is not UINT64_MAX -- ONE 8-byte load per lane, then PH_FM_LABELSET's loop over
//                 the wave-uniform set values against the label word, and two compares of the key word
//                 (ph_pairset_holds, filter_route.h).  A NONE label in the set, lo > hi and duplicates need no scalar
//                 test.  The two bounds are read ONCE PER QUERY in front of the walk, beside the two offsets, and held
//                 across it -- NOT where the test runs, as PH_FM_LABEL_RANGE reads its three words: here that form left
//                 five instances with scratch where the set twin has none, this one leaves one
//                 (profiles/labelset_ranged, which compiles the other form with -DPH_LABELSET_RANGE_BOUNDS_AT_TEST).
//                 a.pair_want is unused.  Never with a bitmap, a single
//                 label or an attribute column, and there is no collecting twin.
// A mode of the body and not a run-time test of the pointers: the test alone cost 19 of the 88 kernels scratch
// (profiles/filter), so the filtered instances exist beside the others and are picked only when a filter is given.
//   PH_FM_COLLECT  a bit on top of PH_FM_BITMAP / PH_FM_LABEL: the collecting walk (phnsw_search_collect*, search_collect.hip,
//                  search_collect_labeled.hip).  The descent is the PLAIN search's -- the layer tails apply `exclude` only --
//                  and the walk of the last layer keeps, beside the layer's queue, the a.collect_k best evaluated rows
//                  that pass the filter (`kq`, below); those are the result row.  Only ever the last launch of a descent.
//   PH_FM_RADIUS   a mode of its own, with no filter: the radius search by graph walk (phnsw_search_batch_radius*,
//                  search_radius.hip).  The descent is the PLAIN search's; on the LAST layer the queue the running
//                  candidates were mapped into goes through threshold_nn's loop (lib.rs:944-953) against the query's own
//                  a.radius[q] -- closest_nodes again and again, every entry a seed again, the capacity doubled while the
//                  queue is full and its last entry inside the radius -- and the row is read from that QUEUE: the entries
//                  other than `exclude`, taken while d < radius, the nearest a.out_stride of them written and ALL of them
//                  counted in out_len.  Instantiated over the 1024-slot queues only, and only in search_radius.hip; a
//                  queue that would pass 1024 entries ends the query with ST_CAPACITY.  One launch, no dense tables.
enum : int { PH_FM_NONE = 0, PH_FM_BITMAP = 1, PH_FM_LABEL = 2, PH_FM_COLLECT = 4, PH_FM_LABELSET = 8, PH_FM_RANGE = 16, PH_FM_LABEL_RANGE = 32, PH_FM_LABELSET_RANGE = 64, PH_FM_RADIUS = 128 };
#define ST_SET_RANGE 8u  // the status of a query whose set range is not sound: phnsw_search_exact_labelset_device's value
// the mode a launch's arguments ask for
static inline int ph_filter_mode(const PhSearchArgs &a) {
  const int where = a.pair_of   ? (a.set_first ? PH_FM_LABELSET_RANGE : PH_FM_LABEL_RANGE)
                    : a.attr_of ? PH_FM_RANGE
                              : (a.set_first ? PH_FM_LABELSET : (a.label_of ? PH_FM_LABEL : (a.filter ? PH_FM_BITMAP : PH_FM_NONE)));
  return where | (a.collect_k ? PH_FM_COLLECT : PH_FM_NONE) | (a.radius ? PH_FM_RADIUS : PH_FM_NONE);
}

// What a query of the set modes gets whose range in set_values is not sound: the row of a failed query, ST_SET_RANGE,
// stats 0; nothing of set_values has been read
__device__ __forceinline__ void ph_search_refuse_set(const PhSearchArgs &a, uint32_t q, uint32_t lane) {
  const uint32_t ostride = a.out_stride ? a.out_stride : a.ef;
  for (uint32_t i = lane; i < ostride; i += 64) {
    a.out_ids[(uint64_t)q * ostride + i] = PH_EMPTY32;
    a.out_d[(uint64_t)q * ostride + i] = PH_FMAX;
  }
  if (lane == 0) {
    a.out_len[q] = 0u;
    a.status[q] = ST_SET_RANGE;
    if (a.out_stats) a.out_stats[2 * (uint64_t)q] = 0u, a.out_stats[2 * (uint64_t)q + 1] = 0u;
    if (a.out_key) a.out_key[q] = PH_EMPTY32;
  }
}

template <int CAPC, class Dist, bool INSTR = false, bool BIG = false, int FILT = PH_FM_NONE>
__device__ __forceinline__ void ph_search_body(const PhSearchArgs &a) {
  extern __shared__ uint32_t smem[];
  constexpr int CAP = CAPC * 64;
  constexpr int FM = FILT & (PH_FM_BITMAP | PH_FM_LABEL | PH_FM_LABELSET | PH_FM_RANGE | PH_FM_LABEL_RANGE | PH_FM_LABELSET_RANGE);  // where the filter is read from
  constexpr bool COLLECT = (FILT & PH_FM_COLLECT) != 0;
  constexpr bool RADIUS = (FILT & PH_FM_RADIUS) != 0;
  constexpr int TAILF = COLLECT ? PH_FM_NONE : FM;  // closest_vectors' `include` beyond `exclude`: none in a collecting walk
  uint32_t *Cid = smem;                    // running candidates: VectorIds (search.rs:110)
  float *Cd = (float *)(smem + CAP);       //
  uint32_t *Qid = smem + 2 * CAP;          // layer queue: NodeIds | EXPF (lib.rs:264)
  float *Qd = (float *)(smem + 3 * CAP);   //
  if constexpr (BIG) {
    Qid = a.big_q + (uint64_t)blockIdx.x * 2u * a.cap_max;
    Qd = (float *)(Qid + a.cap_max);
  }
  uint32_t *S = smem + 4 * CAP;            // prefix scratch [CAP + 64]
  float *dist_lds = (float *)(smem + 5 * CAP + 64);  // DistPQ: the query's lookup table
  if (Dist::GLOBAL_TABLE) dist_lds = (float *)((char *)a.pq_tables + (size_t)blockIdx.x * a.pq_table_bytes);
  // dense top layers (tiny.hip): this query's row of the distance table and the visited bits of the
  // table ids, both in LDS; T = 0 when the launch has none (or its layers turned out not to be nested)
  const uint32_t T = (a.tiny_layers && a.tiny_member[a.tiny_n] == 0u) ? a.tiny_layers : 0u;
  const bool tiny_lds_row = a.tiny_n <= a.tiny_lds_nodes;
  float *Dl = (float *)(smem + 5 * CAP + 64);
  uint32_t *Vl = smem + 5 * CAP + 64 + (tiny_lds_row ? a.tiny_stride : 0u);
  const uint32_t tiny_words = (a.tiny_n + 31u) / 32u;

  const uint32_t lane = threadIdx.x;
  const uint64_t lt = lanemask_lt(lane);
  constexpr bool DENSE_ONLY = dist_is_none<Dist>::value;
  // the dense-only launch and its follow-up agree through the table's device-side "usable" flag (phnsw_internal.h)
  const bool table_ok = (a.dense_only || a.after_dense) ? a.dense_flag[0] == 0u : true;
  if (DENSE_ONLY && !table_ok) return;  // layers not nested: the follow-up launch walks everything per hop
  const uint32_t layer_lo = a.after_dense ? (table_ok ? a.after_dense : 0u) : a.layer_lo;
  uint32_t *vis = a.visited + (uint64_t)blockIdx.x * a.visited_words;
  uint2 *ovf = DENSE_ONLY ? a.dense_ovf + (uint64_t)blockIdx.x * a.dense_ovf_cap : a.ovf + (uint64_t)blockIdx.x * a.ovf_cap;
  const uint32_t ovf_cap = DENSE_ONLY ? a.dense_ovf_cap : a.ovf_cap;
  uint32_t *const Qs = S;
  uint32_t *const ovf_s = INSTR ? a.ovf_s + (uint64_t)blockIdx.x * a.ovf_cap : nullptr;
  // visited set of the gathered layers in LDS (vis_slots = 0: the bitmap in HBM); empty between layers
  uint32_t *const H = smem + a.vis_off;
  const uint32_t hslots = (BIG || INSTR || !vis_lds_policy<CAPC, Dist>::value) ? 0u : a.vis_slots;
  for (uint32_t i = lane; i < hslots; i += 64) H[i] = PH_EMPTY32;

  // locality schedule: with an `order` the query list is cut into 8 consecutive segments, one
  // per XCD, so that the queries one L2 serves together are neighbours in `order`; a wave
  // whose segment is exhausted moves on to the next one (no idle tail)
  uint32_t seg_cur = 0, seg_done = 0;
  if (a.order) {
    uint32_t xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    seg_cur = (xcc & 15u) & 7u;
  }

  for (;;) {
    uint32_t q = 0, qpos = 0;  // qpos: position in the launch's processing order (row of the dense table)
    if (!a.order) {
      if (lane == 0) q = atomicAdd(a.counter, 1u);
      q = rfl32(q);
      if (q >= a.nq) break;
      qpos = q;
    } else {
      for (;;) {
        uint32_t p = 0;
        if (lane == 0) p = atomicAdd(a.counter + seg_cur * 16u, 1u);
        p = rfl32(p);
        const uint32_t base = seg_cur * a.seg;
        const uint32_t len = base >= a.nq ? 0u : min(a.seg, a.nq - base);
        if (p < len) {
          qpos = base + p;
          q = a.order[qpos];
          break;
        }
        seg_cur = (seg_cur + 1u) & 7u;
        if (++seg_done == 8u) {
          q = PH_EMPTY32;
          break;
        }
      }
      if (q == PH_EMPTY32) break;
    }

    const uint32_t last_layer = a.n_layers - 1;
    // a descent may run as two launches (upper layers; then the bottom layer with the queries
    // re-ordered by where they landed): layers [layer_lo, layer_hi) of this launch, the running
    // candidates parked in the output rows in between
    const uint32_t layer_hi = a.layer_hi ? a.layer_hi : a.n_layers;
    if (layer_lo && a.status[q] != ST_OK) continue;  // failed in the first launch: keep its status
    // knn modes: the query is a node of the bottom layer
    const uint32_t qnode = (BIG && a.knn_nodes) ? a.knn_nodes[q] : a.first_node + q;
    uint32_t qvec = a.knn_mode ? a.layers[last_layer].nodes[qnode] : (a.qids ? a.qids[q] : 0u);
    // row of this query in the dense table: its launch position (the query itself when the table was made before the
    // order, api.hip), or (the build's kept table) its NodeId in layer X
    uint64_t trow = a.table_by_query ? q : qpos;
    if (a.tiny_rows) trow = (uint64_t)((a.tiny_row_map ? a.tiny_row_map[qvec] : qvec) - a.tiny_row_first);
    Dist dist;
    if (a.queries && !a.knn_mode)
      dist.prepare_raw(a.dist, a.queries + (uint64_t)q * a.ldq, dist_lds, lane);
    else
      dist.prepare_stored(a.dist, qvec, dist_lds, lane);
    const uint32_t excl = a.exclude ? a.exclude[q] : PH_EMPTY32;
    float rad = 0.0f;  // RADIUS: the threshold of this query's loop on the last layer
    if constexpr (RADIUS) rad = a.radius[q];
    // the allow-list of this query (wave-uniform): `include` of lib.rs:250-277
    const uint32_t *const allow = FM == PH_FM_BITMAP ? a.filter + (uint64_t)q * a.filter_stride : nullptr;
    // ... or the label it wants (wave-uniform); NONE matches nothing, not even the unlisted vectors that carry it
    const uint32_t want = FM == PH_FM_LABEL ? rfl32(a.label_want[q]) : PHNSW_LABEL_NONE;
    // ... or the range of its set in set_values (wave-uniform, absolute offsets).  A range that is not sound ends the
    // query here, before anything of set_values is read: the row a failed query gets, ST_SET_RANGE, stats 0.  (A later
    // launch of a split descent never comes here: the status check above.)
    uint32_t set_b = 0, set_e = 0;
    if constexpr (FM == PH_FM_LABELSET || FM == PH_FM_LABELSET_RANGE) {
      set_b = rfl32(a.set_first[q]);
      set_e = rfl32(a.set_first[q + 1u]);
      if (!ph_set_range_sound(set_b, set_e, a.set_nwant)) {
        ph_search_refuse_set(a, q, lane);
        continue;
      }
    }
    // ... or the bounds of its range (wave-uniform, inclusive)
    const uint32_t range_lo = FM == PH_FM_RANGE ? rfl32(a.range_lo[q]) : 0u;
    const uint32_t range_hi = FM == PH_FM_RANGE ? rfl32(a.range_hi[q]) : 0u;
#ifndef PH_LABELSET_RANGE_BOUNDS_AT_TEST
    // ... or, beside the offsets of its set, the bounds of the set-range mode (wave-uniform, inclusive)
    const uint32_t pairset_lo = FM == PH_FM_LABELSET_RANGE ? rfl32(a.pair_lo[q]) : 0u;
    const uint32_t pairset_hi = FM == PH_FM_LABELSET_RANGE ? rfl32(a.pair_hi[q]) : 0u;
#endif
    // the filter test of VectorId v, written once for the layer tail, the strict pass and the collecting walk (callers
    // guard it: only lanes holding an id read a word or a label)
    auto passes = [&](uint32_t v) -> bool {
      if constexpr (FM == PH_FM_BITMAP) {
        return (allow[v >> 5] >> (v & 31)) & 1u;
      } else if constexpr (FM == PH_FM_LABEL) {
        const uint32_t lbl = a.label_of[v];
        return lbl == want && lbl != PHNSW_LABEL_NONE;
      } else if constexpr (FM == PH_FM_LABELSET) {
        return ph_set_holds(a.label_of[v], set_b, set_e, a.set_values, PHNSW_LABEL_NONE);
      } else if constexpr (FM == PH_FM_RANGE) {
        return ph_range_holds(a.attr_of[v], range_lo, range_hi, PHNSW_ATTR_NONE);
      } else if constexpr (FM == PH_FM_LABEL_RANGE) {
        return ph_pair_holds_words(a.pair_of[v], rfl32(a.pair_want[q]), rfl32(a.pair_lo[q]), rfl32(a.pair_hi[q]), 0xFFFFFFFFFFFFFFFFull);
      } else if constexpr (FM == PH_FM_LABELSET_RANGE) {
#ifndef PH_LABELSET_RANGE_BOUNDS_AT_TEST
        return ph_pairset_holds(a.pair_of[v], set_b, set_e, a.set_values, pairset_lo, pairset_hi, 0xFFFFFFFFFFFFFFFFull);
#else  // the form profiles/labelset_ranged compiles for comparison
        return ph_pairset_holds(a.pair_of[v], set_b, set_e, a.set_values, rfl32(a.pair_lo[q]), rfl32(a.pair_hi[q]), 0xFFFFFFFFFFFFFFFFull);
#endif
      } else {
        return true;
      }
    };
    // COLLECT: `kq`, the contract's `kept` (phnsw.h; named apart from the `kept` counters of the tails below): a
    // PriorityQueue of capacity a.collect_k ordered by (distance, id) like every queue here, in registers: lane i holds
    // the 64-bit key of slot i (VectorId in the low word), KEY_NONE in empty slots and in slots >= collect_k.  No LDS:
    // the LDS budget decides occupancy and the size of the visited table.
    uint64_t kq = KEY_NONE;
    uint32_t klen = 0;
    // merge of one batch into `kq`: ckey = the lane's key when its row qualifies, else KEY_NONE.  Returns whether
    // `kq` changed.  One ballot of the lanes that can enter (below the tail of a full `kq`, any while it is not
    // full); empty = nothing else to do, the common case late in a layer.  Otherwise a scalar loop over the entering
    // bits (v_readlane + 64-bit compare, the idiom of the main merge): keys are distinct and absent from `kq` (the
    // nodes are fresh), so the final slot of an entering key = (kq keys below) + (entering keys below), two s_bcnt1 of
    // compare masks, and the lane of that slot takes it; every other slot s pulls the kq entry s - (entering keys
    // placed under s) with one ds_bpermute per half.  What lands at slot >= collect_k drops out.
    auto collect = [&](uint64_t ckey) -> bool {
      const uint32_t kk = a.collect_k;
      const uint64_t tail = klen == kk ? rl64(kq, (int)kk - 1) : KEY_NONE;
      const bool ent = ckey < tail;
      const uint64_t em = __ballot(ent);
      if (!em) return false;
      uint64_t in = KEY_NONE;
      uint32_t under = 0;
      for (uint64_t rem = em; rem; rem &= rem - 1) {
        const uint64_t kj = rl64(ckey, __builtin_ctzll(rem));
        const uint32_t p = (uint32_t)__popcll(__ballot(kq < kj)) + (uint32_t)__popcll(__ballot(ent && ckey < kj));
        under += p < lane ? 1u : 0u;
        if (p == lane) in = kj;
      }
      const int src = (int)((lane - under) << 2);  // under <= lane: the slots below hold `under` entering keys
      const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)kq);
      const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(kq >> 32));
      kq = in != KEY_NONE ? in : (((uint64_t)hi << 32) | lo);
      if (lane >= kk) kq = KEY_NONE;
      klen = min(kk, klen + (uint32_t)__popcll(em));
      return true;
    };
    uint32_t n_dist = 0, n_hops = 0, err = ST_OK;
    uint32_t index_distance = 0xFFFFFFFFu;  // usize::MAX until a layer has run  search.rs:112
    uint32_t n_tab = 0;  // of n_dist: evaluations served by the dense tables (measurement: the rest are gathered rows)
    uint32_t n_dist0 = 0, n_hops0 = 0;  // counters a split descent brought in from its earlier launches
    uint32_t clen = 0;
    uint32_t ef = a.ef;  // queue capacity; grows in threshold_nn mode (resize_capacity)
    bool big_written = false;

    if (layer_lo) {
      clen = a.out_len[q];
#pragma unroll
      for (int c = 0; c < CAPC; c++) {
        uint32_t i = lane + 64u * c;
        if (i < clen) {
          Cid[i] = a.out_ids[(uint64_t)q * a.ef + i];
          Cd[i] = a.out_d[(uint64_t)q * a.ef + i];
        }
      }
      if (a.out_stats) {
        n_dist = a.out_stats[2 * (uint64_t)q];
        n_hops = a.out_stats[2 * (uint64_t)q + 1];
      }
      n_dist0 = n_dist;
      n_hops0 = n_hops;
    } else if (!a.knn_mode) {
      // entry_vector + distance_from_entry  search.rs:101-111
      uint32_t entry = a.layers[0].nodes[0];
      float d0;
      if constexpr (DENSE_ONLY) {  // the table holds it
        const PhLayerDev TLy = a.layers[a.tiny_layers - 1];
        const uint32_t tid = TLy.vec2node ? TLy.vec2node[entry] : entry;
        d0 = (a.tiny_d + trow * a.tiny_stride)[tid < a.tiny_n ? tid : 0u];
      } else {
        d0 = dist.batch(a.dist, 1ull, entry, lane);
      }
      d0 = __uint_as_float(rl32(__float_as_uint(d0), 0));
      n_dist = 1;
      if (lane == 0) {
        Cid[0] = entry;
        Cd[0] = d0;
      }
      clen = 1;
    }
    const float *Dg = a.tiny_d + trow * a.tiny_stride;  // this query's row of the table
    if (T) {
      if (tiny_lds_row)
        for (uint32_t i = lane; i < a.tiny_n; i += 64) Dl[i] = Dg[i];
      for (uint32_t i = lane; i < tiny_words; i += 64) Vl[i] = 0u;
    }
    queue_sync<BIG>();

    for (uint32_t li = a.knn_mode ? last_layer : layer_lo; li < layer_hi && err == ST_OK; li++) {
      PhLayerDev L = a.layers[li];
      // a dense top layer is walked in table ids: ids, id maps and neighbour rows of the table layer
      const bool tl = li < T;
      if (tl) {
        const PhLayerDev TLy = a.layers[T - 1];
        L.n_nodes = a.tiny_n;
        L.nodes = TLy.nodes;
        L.vec2node = TLy.vec2node;
        L.neighbors = a.tiny_nbr + a.tiny_off[li];
      }
      const bool identity = L.vec2node == nullptr;
      if constexpr (RADIUS) {
        // `while last < threshold` with last = 0.0 (lib.rs:944-946): a zero, negative or NaN radius never calls
        // closest_nodes on the last layer, and nothing of the queue lies inside it -- the empty row, the counters of the
        // layers above
        if (li == last_layer && !(rad > 0.0f)) {
          for (uint32_t i = lane; i < a.out_stride; i += 64) {
            a.out_ids[(uint64_t)q * a.out_stride + i] = PH_EMPTY32;
            a.out_d[(uint64_t)q * a.out_stride + i] = PH_FMAX;
          }
          clen = 0;
          big_written = true;
          continue;
        }
      }
      bool hv = hslots && !tl;  // this layer's visited set is the LDS table (until it would pass its load limit)
      uint32_t hn = 0;          // ids in the table
      // test-and-set of one id per valid lane in the layer's visited set: true when it was not in it.  A batch that
      // could take the table past vis_limit first moves the table into the bitmap, where the layer then goes on.
      auto visit = [&](uint32_t id, bool valid) -> bool {
        if (hv && hn + (uint32_t)__popcll(__ballot(valid)) > a.vis_limit) {
          for (uint32_t i = lane; i < hslots; i += 64) {
            const uint32_t o = H[i];
            if (o != PH_EMPTY32) {
              atomicOr(&vis[o >> 5], 1u << (o & 31));
              H[i] = PH_EMPTY32;
            }
          }
          wait_vm0();
          hv = false;
        }
        if (hv) {
          const bool f = vis_insert(H, hslots, id, valid);
          hn += (uint32_t)__popcll(__ballot(f));
          return f;
        }
        if (!valid) return false;
        const uint32_t bit = 1u << (id & 31);
        return !(atomicOr(&vis[id >> 5], bit) & bit);
      };
      // ---- closest_vectors: VectorId -> NodeId, queue = new(cap); merge_pairs  lib.rs:258-266
      uint32_t qlen;
      if (a.knn_mode) {
        // pq.merge_pairs(&[(node, 0.0)])  lib.rs:917-918
        if (lane == 0) {
          Qid[0] = qnode;
          Qd[0] = 0.0f;
        }
        visit(qnode, lane == 0);
        qlen = 1;
      } else {
        bool miss = false;
#pragma unroll
        for (int c = 0; c < CAPC; c++) {
          uint32_t i = lane + 64u * c;
          if (i < clen) {
            uint32_t vid = Cid[i];
            uint32_t nid = identity ? vid : L.vec2node[vid];
            if (nid >= L.n_nodes || (tl && !((a.tiny_member[nid] >> li) & 1u))) {  // get_node(v).unwrap() would panic  lib.rs:261
              miss = true;
              nid = 0;
            }
            Qid[i] = nid;
            Qd[i] = Cd[i];
          }
        }
        if (__ballot(miss)) {
          err = ST_MISSING;
          break;
        }
        // visited = candidates ids  lib.rs:187
#pragma unroll
        for (int c = 0; c < CAPC; c++) {
          uint32_t i = lane + 64u * c;
          if (tl) {
            if (i < clen) atomicOr(&Vl[Qid[i] >> 5], 1u << (Qid[i] & 31));
          } else if (64u * c < clen) {
            visit(i < clen ? Qid[i] : 0u, i < clen);
          }
        }
        qlen = clen;
      }
      queue_sync<BIG>();
      if constexpr (COLLECT) {
        // `kq` starts from the qualifying entries of the queue the last layer starts with (the `pairs` of
        // closest_vectors: the running candidates, still in C as VectorIds): allowed, not excluded, at most f32::MAX away
        if (li == last_layer) {
#pragma unroll
          for (int c = 0; c < CAPC; c++) {
            if (64u * c >= clen) break;
            const uint32_t i = lane + 64u * c;
            const bool has = i < clen;
            const uint32_t v = has ? Cid[i] : 0u;
            const float d = has ? Cd[i] : PH_FMAX;
            bool ok = has && v != excl && d <= PH_FMAX;
            if (ok) ok = passes(v);
            collect(ok ? mkkey(d, v) : KEY_NONE);
          }
        }
      }

      // Hnsw::threshold_nn (lib.rs:930-962, knn_mode == 2) calls closest_nodes repeatedly on a
      // growing queue; everything else runs this block once
      float thr_last = 0.0f;
      uint32_t thr_last_size = 0;
      for (;;) {
      if constexpr (RADIUS) {
        if (li == last_layer) {
          if (!(thr_last < rad && qlen > thr_last_size)) break;  // lib.rs:946, threshold = the query's radius
          const bool again = thr_last_size != 0;  // the first call's seeds were marked when the candidates were mapped
          thr_last_size = qlen;
          if (again) {
            // a fresh closest_nodes call: every queue entry is a seed again (lib.rs:182-187)
#pragma unroll
            for (int c = 0; c < CAPC; c++) {
              uint32_t i = lane + 64u * c;
              uint32_t nid = 0;
              if (i < qlen) {
                nid = Qid[i] & IDM;
                Qid[i] = nid;
              }
              if (64u * c < qlen) visit(nid, i < qlen);
            }
            queue_sync<BIG>();
          }
        }
      } else
      if (a.knn_mode == 2) {
        if (!(thr_last < a.threshold && qlen > thr_last_size)) break;  // lib.rs:945
        thr_last_size = qlen;
        if (thr_last_size > 1 || n_hops > 0) {
          // a fresh closest_nodes call: every queue entry is a seed again (lib.rs:182-187)
#pragma unroll
          for (int c = 0; c < (BIG ? (int)((qlen + 63u) >> 6) : CAPC); c++) {
            uint32_t i = lane + 64u * c;
            uint32_t nid = 0;
            if (i < qlen) {
              nid = Qid[i] & IDM;
              Qid[i] = nid;
            }
            if (64u * c < qlen) visit(nid, i < qlen);
          }
          queue_sync<BIG>();
        }
      }
      // ---- closest_nodes  lib.rs:175-248
      uint32_t ovf_n = 0;
      uint32_t pd = a.probe_depth;
      uint32_t highest = 0;  // highest_improvement  lib.rs:190
      if constexpr (INSTR) {
#pragma unroll
        for (int c = 0; c < CAPC; c++)
          if (lane + 64u * c < qlen) Qs[lane + 64u * c] = 0u;  // seeds: NodeDistance::ZERO  lib.rs:182-185
        queue_sync<BIG>();
      }
      // every queue entry below scan_from has been expanded: the pop scan starts at its 64-entry chunk,
      // and a hop's merge touches only the chunks from its first insertion point on
      uint32_t scan_from = 0;
#ifdef PH_CELL_PROBE
      const bool probing = a.probe_pos && li == last_layer && !tl;
      uint32_t probe_p0 = 0, probe_cnt[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      if (probing) probe_p0 = a.probe_pos[Qid[0] & IDM];
#endif
#ifdef PH_HOP_PROFILE
      uint64_t tprof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      uint64_t t_last = wall_clock64();
      const uint32_t hops_before = n_hops, dist_before = n_dist;
#endif
      for (;;) {
        // visit_queue.pop(): smallest (d,id) among not yet expanded nodes  lib.rs:191,243-244
        int pop = -1;
        uint32_t cur = 0;
        for (uint32_t c = scan_from >> 6; 64u * c < qlen; c++) {
          const uint32_t i = lane + 64u * c;
          const uint32_t e = i < qlen ? Qid[i] : EXPF;
          const uint64_t b = __ballot(!(e & EXPF));
          if (b) {
            const int pl = __builtin_ctzll(b);
            pop = (int)(64u * c) + pl;
            cur = rl32(e, pl);
            break;
          }
        }
        if (pop >= 0) {
          if (lane == 0) Qid[pop] = cur | EXPF;
          if constexpr (BIG) __threadfence();  // the merge below reads the slot back from another lane
        } else {
          if (ovf_n == 0) break;
          wait_vm0();  // spill stores of this wave have reached L2
          uint64_t best = KEY_NONE;
          uint32_t bi = 0;
          for (uint32_t i = lane; i < ovf_n; i += 64) {
            uint32_t id = __hip_atomic_load(&ovf[i].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!(id & EXPF)) {
              uint32_t db = __hip_atomic_load(&ovf[i].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              uint64_t k = mkkey(__uint_as_float(db), id);
              if (k < best) {
                best = k;
                bi = i;
              }
            }
          }
#pragma unroll
          for (int s = 32; s >= 1; s >>= 1) {
            uint64_t o = ((uint64_t)__shfl_xor((uint32_t)(best >> 32), s) << 32) | __shfl_xor((uint32_t)best, s);
            uint32_t oi = __shfl_xor(bi, s);
            if (o < best) {
              best = o;
              bi = oi;
            }
          }
          if (best == KEY_NONE) break;  // frontier exhausted
          cur = (uint32_t)best & IDM;
          if (lane == 0)
            __hip_atomic_store(&ovf[bi].x, cur | EXPF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          pop = -1 - (int)bi;  // INSTR reads the spilled entry's index_sum below
        }
        uint32_t cur_s = 0;
        if constexpr (INSTR) cur_s = pop >= 0 ? Qs[pop] : ovf_s[(uint32_t)(-1 - pop)];
        cur &= IDM;
        n_hops++;
        PH_TICK(0)

        // get_neighbors(next) + filter(!visited)  lib.rs:195-198
        uint32_t nb = PH_EMPTY32;
        if (lane < L.W) nb = L.neighbors[(uint64_t)cur * L.W + lane];
        if constexpr (Dist::EARLY) {
          // the candidates' rows are requested before the visited test-and-set below returns
          const bool valid = nb < L.n_nodes;
          uint32_t v = 0;
          if (valid) v = identity ? nb : L.nodes[nb];
          dist.prefetch(a.dist, valid, v, lane);
        }
        PH_TICK(1)
        bool fresh = false;
        if (tl) {
          if (nb < L.n_nodes) {
            uint32_t bit = 1u << (nb & 31);
            fresh = !(atomicOr(&Vl[nb >> 5], bit) & bit);
          }
        } else {
          fresh = visit(nb, nb < L.n_nodes);
        }
        const uint64_t fm = __ballot(fresh);
        const uint32_t m = __popcll(fm);
        n_dist += m;
        if (tl) n_tab += m;
#ifdef PH_CELL_PROBE
        if (probing) {
          uint32_t dd = 0xFFFFFFFFu;
          if (fresh) {
            const int d0 = (int)a.probe_pos[nb] - (int)probe_p0;
            dd = (uint32_t)(d0 < 0 ? -d0 : d0);
          }
#pragma unroll
          for (int k = 0; k < 10; k++) probe_cnt[k] += __popcll(__ballot(fresh && dd <= (k ? (1u << (k - 1)) : 0u)));
          probe_cnt[10] += m;
        }
#endif
        PH_TICK(2)
        // COLLECT: the filter test of the fresh lanes' vectors, one word or one label each, issued with the row requests
        uint32_t cvec = 0;
        bool cq = false;
        if constexpr (COLLECT) {
          if (li == last_layer && fresh) {
            cvec = identity ? nb : L.nodes[nb];  // (a dense layer walks table ids: its node list maps them too)
            cq = cvec != excl && passes(cvec);
          }
        }

        // distance batch: compare_vec(v, Stored(get_vector(n)))  lib.rs:200-202 -- in a dense top
        // layer the value was computed by the tile pass (same bits) and is looked up
        float myd;
        if (tl) {
          myd = 0.f;
          if (fresh) myd = tiny_lds_row ? Dl[nb] : Dg[nb];
        } else if constexpr (Dist::EARLY) {
          myd = dist.finish(a.dist, fm, lane);
        } else {
          uint32_t vid = 0;
          if (fresh) vid = identity ? nb : L.nodes[nb];
          myd = dist.batch(a.dist, fm, vid, lane);
        }

        PH_TICK(3)
        // candidates.merge_pairs(sorted batch)  lib.rs:206,226 / priority_queue.rs:109-144,
        // as one parallel rank-merge.  Batch keys are distinct and absent from the queue
        // (visited), so final slot = (#queue keys below) + (#batch keys below).
        const uint64_t key = fresh ? mkkey(myd, nb) : KEY_NONE;
        uint32_t my_s = 0;
        if constexpr (INSTR) {  // (ix, (n, d)) of the sorted batch: index_sum + ix + 1  lib.rs:211-220
          uint32_t rank_all = 0;
          uint64_t remf = fm;
          while (remf) {
            const int j = __builtin_ctzll(remf);
            remf &= remf - 1;
            rank_all += (rl64(key, j) < key) ? 1u : 0u;
          }
          my_s = cur_s + rank_all + 1u;
        }
        // An element that is worse than the tail of a FULL queue cannot enter it: it goes straight to
        // the spill list and takes no part in the merge.  Late in a layer most hops bring nothing
        // else; those skip the merge altogether.
        const bool full = qlen == ef;
        const float dtail = full ? Qd[ef - 1] : PH_FMAX;
        const uint64_t tailkey = full ? mkkey(dtail, Qid[ef - 1]) : KEY_NONE;
        // a distance above f32::MAX (an L2 sum that overflowed to +inf) never enters `candidates`: insert's and merge's
        // partition point lies past the f32::MAX fill of the empty slots (priority_queue.rs:102-107, 132-135); the
        // visit_queue still holds it (lib.rs:211-220), so it goes to the spill list like an entry past a full queue
        const bool ins = fresh && key < tailkey && myd <= PH_FMAX;
        const uint64_t im = __ballot(ins);
        uint32_t pos = 0, pos_min = 0xFFFFFFFFu, newpos = 0xFFFFFFFFu;
        // merge()'s return value (priority_queue.rs:109-144), closed form for a sorted,
        // duplicate-free batch e_0 < e_1 < ...: the first element decides.  It is inserted
        // (true) unless it ranks past a full queue; then Err(i>=cap) => break => false,
        // except when its priority ties the queue's tail (Ok branch returns cap, false) and
        // a second element follows (Err(0) on the empty slice => true without writing).
        // e_0 enters the queue exactly when some element does (im != 0); otherwise every distance is
        // >= the tail's, so e_0 ties the tail exactly when some element's distance equals it.
        bool did = im != 0;
        if (!im && m >= 2) did = __ballot(fresh && myd == dtail) != 0;
        if (im) {
          // One pass handles two 64-entry chunks of the queue, TOP chunks first.  For every entering key k_j (a
          // scalar loop over the bits of `im`) the pass counts, per queue slot, the entering keys below it (the
          // distance the slot's entry moves up: into its own chunk or the one above, both already in registers
          // or already rewritten -- a wave's LDS reads and writes execute in program order) and, per entering
          // key, the processed slots holding a greater key (s_bcnt1 of the same compare mask), which gives its
          // insertion point without a search.  The first pass also ranks the entering keys among themselves.
          // The passes stop at the first chunk whose head is below every entering key: everything under it
          // stays where it is and is neither read nor rewritten.  What falls past `ef` is spilled.
          uint32_t rank = 0, greater = 0;
          bool first_pass = true;
          const int c_top = (int)((qlen - 1u) >> 6);
          int c = c_top, c_low;
          for (;;) {
            const bool two = c > 0;  // chunk c-1 belongs to this pass (it is a full chunk)
            const uint32_t i1 = lane + 64u * (uint32_t)c, i0 = i1 - 64u;
            const bool has1 = i1 < qlen;
            const uint32_t qi1 = has1 ? Qid[i1] : PH_EMPTY32;
            const float qd1 = has1 ? Qd[i1] : PH_FMAX;
            const uint64_t qk1 = has1 ? mkkey(qd1, qi1) : KEY_NONE;
            uint32_t qi0 = PH_EMPTY32;
            float qd0 = PH_FMAX;
            if (two) {
              qi0 = Qid[i0];
              qd0 = Qd[i0];
            }
            const uint64_t qk0 = two ? mkkey(qd0, qi0) : KEY_NONE;
            uint32_t qs1 = 0, qs0 = 0;
            if constexpr (INSTR) {
              qs1 = has1 ? Qs[i1] : 0u;
              qs0 = two ? Qs[i0] : 0u;
            }
            uint32_t sh1 = 0, sh0 = 0;
            uint64_t rem = im;
            if (first_pass) {
              while (rem) {
                const int j = __builtin_ctzll(rem);
                rem &= rem - 1;
                const uint64_t kj = rl64(key, j);
                rank += (kj < key) ? 1u : 0u;
                const bool g1 = kj < qk1, g0 = two && kj < qk0;
                sh1 += g1 ? 1u : 0u;
                sh0 += g0 ? 1u : 0u;
                const uint32_t g = (uint32_t)__popcll(__ballot(g1)) + (uint32_t)__popcll(__ballot(g0));
                greater += lane == (uint32_t)j ? g : 0u;
              }
              first_pass = false;
            } else {
              while (rem) {
                const int j = __builtin_ctzll(rem);
                rem &= rem - 1;
                const uint64_t kj = rl64(key, j);
                const bool g1 = kj < qk1, g0 = two && kj < qk0;
                sh1 += g1 ? 1u : 0u;
                sh0 += g0 ? 1u : 0u;
                const uint32_t g = (uint32_t)__popcll(__ballot(g1)) + (uint32_t)__popcll(__ballot(g0));
                greater += lane == (uint32_t)j ? g : 0u;
              }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // both chunks are in registers before either is overwritten
            if constexpr (BIG) wait_vm0();
            const uint32_t np1 = i1 + sh1, np0 = i0 + sh0;
            if (has1 && np1 < ef) {
              Qid[np1] = qi1;
              Qd[np1] = qd1;
              if constexpr (INSTR) Qs[np1] = qs1;
            }
            if (two && np0 < ef) {
              Qid[np0] = qi0;
              Qd[np0] = qd0;
              if constexpr (INSTR) Qs[np0] = qs0;
            }
            if (qlen + 64u > ef) {  // only a queue within 64 entries of its capacity can push anything out
              const bool spill1 = has1 && np1 >= ef;
              const uint64_t sm1 = __ballot(spill1);
              if (sm1) {
                const uint32_t at = ovf_n + __popcll(sm1 & lt);
                if (spill1 && at < ovf_cap) ovf[at] = make_uint2(qi1, __float_as_uint(qd1));
                if constexpr (INSTR)
                  if (spill1 && at < ovf_cap) ovf_s[at] = qs1;
                ovf_n += __popcll(sm1);
              }
              const bool spill0 = two && np0 >= ef;
              const uint64_t sm0 = __ballot(spill0);
              if (sm0) {
                const uint32_t at = ovf_n + __popcll(sm0 & lt);
                if (spill0 && at < ovf_cap) ovf[at] = make_uint2(qi0, __float_as_uint(qd0));
                if constexpr (INSTR)
                  if (spill0 && at < ovf_cap) ovf_s[at] = qs0;
                ovf_n += __popcll(sm0);
              }
            }
            c_low = two ? c - 1 : c;
            // the head of the lowest chunk done (its lane 0) is below every entering key: so is all the rest
            if (c_low == 0 || rl32(two ? sh0 : sh1, 0) == 0u) break;
            c -= 2;
          }
          // slots of the chunks done (the empty ones of the top chunk count as greater) + all of the chunks below
          pos = 64u * (uint32_t)(c_top + 1) - greater;
          if (ins) newpos = pos + rank;
          pos_min = rl32(pos, __builtin_ctzll(__ballot(ins && rank == 0u)));  // the smallest entering key's
          PH_TICK(5)
          queue_sync<BIG>();
          PH_TICK(6)
        }
        {
          if (fresh && newpos < ef) {
            Qid[newpos] = nb;
            Qd[newpos] = myd;
            if constexpr (INSTR) Qs[newpos] = my_s;
          }
          bool spill = fresh && newpos >= ef;
          uint64_t sm = __ballot(spill);
          if (sm) {
            uint32_t at = ovf_n + __popcll(sm & lt);
            if (spill && at < ovf_cap) ovf[at] = make_uint2(nb, __float_as_uint(myd));
            if constexpr (INSTR)
              if (spill && at < ovf_cap) ovf_s[at] = my_s;
            ovf_n += __popcll(sm);
          }
          if constexpr (INSTR)  // current_best != candidates.first(): a new entry took slot 0  lib.rs:225-231
            if (__ballot(fresh && newpos == 0u)) highest = cur_s;
        }
        qlen = min(ef, qlen + (uint32_t)__popcll(im));  // every entering element of a queue that is not full; a full one stays full
        scan_from = min(pop >= 0 ? (uint32_t)pop + 1u : scan_from, pos_min);
        queue_sync<BIG>();
        PH_TICK(4)
        if constexpr (COLLECT) {
          // every qualifying member of the batch merge_pairs sees, those bound for the spill list included: their
          // distances are still in registers (after the main merge: its keys and ranks are dead by now).  PHNSW_COLLECT_EXTEND: a hop that changed `kq` did something.
          if (li == last_layer) {
            const bool changed = collect((cq && myd <= PH_FMAX) ? mkkey(myd, cvec) : KEY_NONE);
            if (a.collect_flags & PHNSW_COLLECT_EXTEND) did = did || changed;
          }
        }
        if (ovf_n > ovf_cap) {
          err = ST_OVERFLOW;
          break;
        }
        if (!did) {  // lib.rs:233-238
          pd -= 1;
          if (pd == 0) break;
        }
      }
      if (err != ST_OK) break;
      if constexpr (INSTR) index_distance = highest;  // last_index_distance = index_distance  search.rs:135
#ifdef PH_CELL_PROBE
      if (probing && lane == 0) {
        for (int k = 0; k < 11; k++) atomicAdd(&a.probe_out[k], (unsigned long long)probe_cnt[k]);
        atomicAdd(&a.probe_out[11], 1ull);
      }
#endif
#ifdef PH_HOP_PROFILE
      if (lane == 0 && q == 0)
        printf("hop profile q0 layer %u%s: hops %u evals %u | us: pop %.1f nbr %.1f visited %.1f dist %.1f merge %.1f (+ search/rank %.1f, shift %.1f)\n", li,
               tl ? " (dense)" : "", n_hops - hops_before, n_dist - dist_before, tprof[0] * 0.01, tprof[1] * 0.01, tprof[2] * 0.01,
               tprof[3] * 0.01, tprof[4] * 0.01, tprof[5] * 0.01, tprof[6] * 0.01);
#endif

#ifdef PH_VISITED_PROBE
      if (!tl && lane == 0) {  // every visited id is in the queue or the spill list
        const uint32_t k = li == last_layer ? 1u : 0u;
        atomicAdd(&a.vprobe_out[k * 64u + min((qlen + ovf_n) >> 6, 63u)], 1ull);
        if (!hv && hslots) atomicAdd(&a.vprobe_out[128u + k], 1ull);
      }
#endif
      // ---- clear this layer's visited set (queue + spill hold every evaluated node)
      if (tl) {
        for (uint32_t i = lane; i < tiny_words; i += 64) Vl[i] = 0u;
      } else if (hv) {
        for (uint32_t i = lane; i < hslots; i += 64) H[i] = PH_EMPTY32;
      } else {
#pragma unroll
        for (int c = 0; c < (BIG ? (int)((qlen + 63u) >> 6) : CAPC); c++) {
          uint32_t i = lane + 64u * c;
          if (i < qlen) vis[(Qid[i] & IDM) >> 5] = 0u;
        }
        if (ovf_n) {
          wait_vm0();
          for (uint32_t i = lane; i < ovf_n; i += 64) {
            uint32_t id = __hip_atomic_load(&ovf[i].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & IDM;
            vis[id >> 5] = 0u;
          }
        }
      }
      wait_vm0();
      hv = hslots && !tl;
      hn = 0;
      if constexpr (RADIUS) {
        if (li != last_layer) break;
      } else
      if (a.knn_mode != 2) break;
      thr_last = Qd[qlen - 1];  // pq.last().1  lib.rs:948
      if (thr_last < (RADIUS ? rad : a.threshold) && qlen == ef) {  // pq.resize_capacity(capacity * 2)  lib.rs:949-951
        if (ef * 2 > (BIG ? a.cap_max : (uint32_t)CAP)) {
          err = ST_CAPACITY;
          break;
        }
        ef *= 2;
      }
      }  // closest_nodes call loop
      if (err != ST_OK) break;

      if constexpr (BIG) {
        // the knn modes start from no running candidates, so closest_vectors' tail (lib.rs:268-276) followed by
        // candidates.merge_pairs (search.rs:136) is the queue itself: it goes straight to the output row, of which
        // the caller reads out_stride entries at most
        const uint32_t os = a.out_stride ? a.out_stride : a.ef;
        uint32_t kept = 0;
        for (uint32_t base = 0; base < qlen && kept < os; base += 64) {
          const uint32_t i = base + lane;
          const bool has = i < qlen;
          const uint32_t nid = has ? (Qid[i] & IDM) : 0u;
          const uint32_t v = has ? (identity ? nid : L.nodes[nid]) : PH_EMPTY32;
          const bool keep = has && v != excl;
          const uint64_t km = __ballot(keep);
          const uint32_t at = kept + __popcll(km & lt);
          if (keep && at < os) {
            a.out_ids[(uint64_t)q * os + at] = v;
            a.out_d[(uint64_t)q * os + at] = Qd[i];
          }
          kept += __popcll(km);
        }
        clen = min(kept, os);
        for (uint32_t i = clen + lane; i < os; i += 64) {
          a.out_ids[(uint64_t)q * os + i] = PH_EMPTY32;
          a.out_d[(uint64_t)q * os + i] = PH_FMAX;
        }
        big_written = true;
        continue;
      }
      if constexpr (RADIUS) {
        // the row of a radius search is read from the queue (lib.rs:954-959): the entries other than `exclude`, taken
        // while d < radius -- the queue ascends, so that is every such entry --, all of them counted, the nearest
        // out_stride written
        if (li == last_layer) {
          const uint32_t os = a.out_stride;
          uint32_t kept = 0;
          for (uint32_t base = 0; base < qlen; base += 64) {
            const uint32_t i = base + lane;
            const bool has = i < qlen;
            const uint32_t nid = has ? (Qid[i] & IDM) : 0u;
            const uint32_t v = has ? (identity ? nid : L.nodes[nid]) : PH_EMPTY32;
            const float d = has ? Qd[i] : PH_FMAX;
            const bool keep = has && v != excl && d < rad;
            const uint64_t km = __ballot(keep);
            const uint32_t at = kept + __popcll(km & lt);
            if (keep && at < os) {
              a.out_ids[(uint64_t)q * os + at] = v;
              a.out_d[(uint64_t)q * os + at] = d;
            }
            kept += __popcll(km);
          }
          for (uint32_t i = min(kept, os) + lane; i < os; i += 64) {
            a.out_ids[(uint64_t)q * os + i] = PH_EMPTY32;
            a.out_d[(uint64_t)q * os + i] = PH_FMAX;
          }
          clen = kept;  // out_len: every entry inside the radius, written or not
          big_written = true;
          continue;
        }
      }
      // ---- closest_vectors tail: NodeId -> VectorId, filter(include), take(count)  lib.rs:268-276
      const uint32_t candidate_count = (a.n_layers == 1 || li == last_layer) ? ef : a.upper;  // search.rs:122-126
      uint32_t bv[CAPC];
      float bd[CAPC];
      uint32_t bpos[CAPC];
      uint32_t kept = 0;
#pragma unroll
      for (int c = 0; c < CAPC; c++) {
        uint32_t i = lane + 64u * c;
        bool has = i < qlen;
        uint32_t nid = has ? (Qid[i] & IDM) : 0u;
        bd[c] = has ? Qd[i] : PH_FMAX;
        bv[c] = has ? (identity ? nid : L.nodes[nid]) : PH_EMPTY32;
        bool keep = has && bv[c] != excl;
        if constexpr (TAILF != PH_FM_NONE)
          if (keep) keep = passes(bv[c]);  // (only lanes holding an id read a word or a label)
        uint64_t km = __ballot(keep);
        uint32_t at = kept + __popcll(km & lt);
        bpos[c] = (keep && at < candidate_count) ? at : PH_EMPTY32;
        kept += __popcll(km);
      }
      const uint32_t blen = min(kept, candidate_count);
      queue_sync<BIG>();
#pragma unroll
      for (int c = 0; c < CAPC; c++) {
        if (bpos[c] != PH_EMPTY32) {
          Qid[bpos[c]] = bv[c];
          Qd[bpos[c]] = bd[c];
        }
      }
      queue_sync<BIG>();

      // ---- candidates.merge_pairs(&closest)  search.rs:136 : sorted set union, cap ef.
      // An element present in both lists (same id => same distance) is kept once.
      uint32_t ci[CAPC];
      float cd[CAPC];
      uint32_t cpos[CAPC];
      uint32_t dups = 0;
#pragma unroll
      for (int c = 0; c < CAPC; c++) {
        uint32_t i = lane + 64u * c;
        bool has = i < clen;
        ci[c] = has ? Cid[i] : PH_EMPTY32;
        cd[c] = has ? Cd[i] : PH_FMAX;
        bool dup = false;
        uint32_t lb = 0;
        if (has) {
          uint64_t k = mkkey(cd[c], ci[c]);
          lb = lds_lower_bound(Qid, Qd, blen, k);
          dup = lb < blen && mkkey(Qd[lb], Qid[lb]) == k;
        }
        uint64_t dm = __ballot(dup);
        uint32_t pre = dups + __popcll(dm & lt);  // duplicates among C[0..i)
        S[i] = pre;
        cpos[c] = (has && !dup) ? (i - pre) + lb : PH_EMPTY32;
        dups += __popcll(dm);
      }
      if (lane == 0) S[CAP] = dups;
      queue_sync<BIG>();
#pragma unroll
      for (int c = 0; c < CAPC; c++) {
        uint32_t j = lane + 64u * c;
        bool has = j < blen;
        bv[c] = has ? Qid[j] : PH_EMPTY32;
        bd[c] = has ? Qd[j] : PH_FMAX;
        bpos[c] = PH_EMPTY32;
        if (has) {
          uint32_t la = lds_lower_bound(Cid, Cd, clen, mkkey(bd[c], bv[c]));
          uint32_t dupb = la < clen ? S[la] : S[CAP];  // S[clen] when la == clen
          if (la == clen) dupb = dups;
          bpos[c] = j + (la - dupb);
        }
      }
      queue_sync<BIG>();
#pragma unroll
      for (int c = 0; c < CAPC; c++) {
        if (cpos[c] < ef) {
          Cid[cpos[c]] = ci[c];
          Cd[cpos[c]] = cd[c];
        }
        if (bpos[c] < ef) {
          Cid[bpos[c]] = bv[c];
          Cd[bpos[c]] = bd[c];
        }
      }
      clen = min(ef, clen - dups + blen);
      queue_sync<BIG>();
    }

    if (err != ST_OK) {
      // leave the slot clean for the next query: wipe the whole bitmap (rare path; a dense-only launch has none)
      if (!DENSE_ONLY)
        for (uint64_t w = lane; w < a.visited_words; w += 64) vis[w] = 0u;
      for (uint32_t i = lane; i < hslots; i += 64) H[i] = PH_EMPTY32;
      wait_vm0();
      clen = 0;
      kq = KEY_NONE;
      klen = 0;
    }
    // PHNSW_FILTER_STRICT: the entry vector enters `candidates` before any filter runs (search.rs:102-111) and may
    // sit in the row although it is disallowed; the last launch of a descent takes such ids out, in order
    if (TAILF && (a.filter_flags & PHNSW_FILTER_STRICT) && layer_hi == a.n_layers && !big_written) {
      uint32_t sv[CAPC];
      float sd[CAPC];
      uint32_t spos[CAPC];
      uint32_t kept = 0;
#pragma unroll
      for (int c = 0; c < CAPC; c++) {
        const uint32_t i = lane + 64u * c;
        const bool has = i < clen;
        sv[c] = has ? Cid[i] : 0u;
        sd[c] = has ? Cd[i] : PH_FMAX;
        bool keep = false;
        if (has) keep = passes(sv[c]);
        const uint64_t km = __ballot(keep);
        spos[c] = keep ? kept + __popcll(km & lt) : PH_EMPTY32;
        kept += __popcll(km);
      }
      queue_sync<BIG>();
#pragma unroll
      for (int c = 0; c < CAPC; c++) {
        if (spos[c] != PH_EMPTY32) {
          Cid[spos[c]] = sv[c];
          Cd[spos[c]] = sd[c];
        }
      }
      clen = kept;
      queue_sync<BIG>();
    }
    // (candidates.iter().collect(), ..)  search.rs:139
    if constexpr (COLLECT) {
      // the row of a collecting search is `kq`: rows of collect_k entries, the distance from the key's upper word
      // (unfkey: the walk's bits; a -0.0 comes back as +0.0, as from the exact calls)
      const uint32_t kk = a.collect_k;
      if (lane < kk) {
        a.collect_ids[(uint64_t)q * kk + lane] = lane < klen ? (uint32_t)kq : PH_EMPTY32;
        a.collect_d[(uint64_t)q * kk + lane] = lane < klen ? unfkey((uint32_t)(kq >> 32)) : PH_FMAX;
      }
    } else {
    const uint32_t ostride = a.out_stride ? a.out_stride : a.ef;
    for (uint32_t i = lane; i < ostride && !big_written; i += 64) {
      a.out_ids[(uint64_t)q * ostride + i] = i < clen ? Cid[i] : PH_EMPTY32;
      a.out_d[(uint64_t)q * ostride + i] = i < clen ? Cd[i] : PH_FMAX;
    }
    }
    if (a.out_hit) {
      // res.iter().any(|v| v == *vid)  lib.rs:1492
      // hit_eps > 0: match_within_epsilon (search.rs:173-187): only the leading results with
      // |d| < eps count
      uint32_t cut = clen;
      if (a.hit_eps > 0.f) {
#pragma unroll
        for (int c = 0; c < CAPC; c++) {
          uint32_t i = lane + 64u * c;
          bool far = i < clen && !(fabsf(Cd[i]) < a.hit_eps);
          uint64_t fmk = __ballot(far);
          if (fmk && cut == clen) cut = 64u * c + __builtin_ctzll(fmk);
        }
      }
      bool hit = false;
#pragma unroll
      for (int c = 0; c < CAPC; c++) {
        uint32_t i = lane + 64u * c;
        hit |= (i < cut && Cid[i] == qvec);
      }
      uint64_t hm = __ballot(hit);
      if (lane == 0) a.out_hit[q] = hm ? 1u : 0u;
    }
    if (a.out_key && lane == 0) {
      // where the query landed: the cell (or node) of its best candidate in the last layer done
      uint32_t key = PH_EMPTY32;
      if (clen) {
        const PhLayerDev KL = a.layers[layer_hi - 1];
        uint32_t nid = KL.vec2node ? KL.vec2node[Cid[0]] : Cid[0];
        if (nid < KL.n_nodes) key = a.key_pos ? a.key_pos[nid] : nid;
      }
      a.out_key[q] = key;
    }
    if (lane == 0 && a.totals) {
      atomicAdd(&a.totals[0], (unsigned long long)(n_dist - n_dist0));
      atomicAdd(&a.totals[1], (unsigned long long)(n_hops - n_hops0));
    }
    if (lane == 0 && a.launch_totals) {
      atomicAdd(&a.launch_totals[0], (unsigned long long)(n_dist - n_dist0));
      atomicAdd(&a.launch_totals[1], (unsigned long long)(n_hops - n_hops0));
      if (a.launch_tab && n_tab) atomicAdd(a.launch_tab, (unsigned long long)n_tab);
    }
    if constexpr (INSTR)
      if (lane == 0) a.out_index[q] = index_distance;
    if (lane == 0) {
      a.out_len[q] = COLLECT ? klen : clen;
      a.status[q] = err;
      if (a.out_stats) {
        a.out_stats[2 * (uint64_t)q] = n_dist;
        a.out_stats[2 * (uint64_t)q + 1] = n_hops;
      }
    }
    queue_sync<BIG>();
  }
}

template <int CAPC, class Dist, int FILT = PH_FM_NONE>
__global__ __launch_bounds__(64) void ph_search_kernel(PhSearchArgs a) {
  ph_search_body<CAPC, Dist, false, false, FILT>(a);
}

// The dense top layers in a launch of their own: no distance policy state, so half the registers and (queues of
// ef <= 256 in 256 slots) half the LDS of the full kernel -- twice the resident waves on a walk that is pure
// latency and instruction issue.  The running candidates are parked in the output rows for the follow-up launch.
template <int CAPC, int FILT = PH_FM_NONE>
__global__ __launch_bounds__(64) void ph_search_kernel_dense(PhSearchArgs a) {
  ph_search_body<CAPC, DistNone, false, false, FILT>(a);
}

// Small batches leave most of the chip idle and finish with their slowest query: their kernels keep up to 24
// rows in flight per wave (one load round per hop instead of up to twelve) at one wave per SIMD.  Same
// arithmetic per row, so the same results.
template <int CAPC, int NV, int FILT = PH_FM_NONE>
__global__ __launch_bounds__(64, 1) void ph_search_kernel_lat(PhSearchArgs a) {
  ph_search_body<CAPC, DistF32<NV, 0>, false, false, FILT>(a);
}

// Hnsw::search_instrumented: the same body carrying index sums (f32 stores; queues of 512 or 1024 slots)
template <int CAPC, int NV>
__global__ __launch_bounds__(64) void ph_search_kernel_instr(PhSearchArgs a) {
  ph_search_body<CAPC, DistF32<NV>, true>(a);
}

// Hnsw::threshold_nn past the LDS queues: the BIG body (queue in global memory, capacity a.cap_max)
template <class Dist>
__global__ __launch_bounds__(64) void ph_search_kernel_big(PhSearchArgs a) {
  ph_search_body<2, Dist, false, true>(a);
}

// the register-table policy keeps a whole lookup table in VGPRs: two waves per SIMD is its register budget
template <int CAPC, int M, int FILT = PH_FM_NONE>
__global__ __launch_bounds__(64, 2) void ph_search_kernel_pqr(PhSearchArgs a) {
  ph_search_body<CAPC, DistPQR<M>, false, false, FILT>(a);
}

// ------------------------------------------------------------------ naming the instances

typedef void (*ph_search_fn)(PhSearchArgs);

enum PhKernelFamily {
  PH_KF_ROWS_F32,   // throughput kernels over f32 rows
  PH_KF_ROWS_F16,   // ... f16 rows
  PH_KF_ROWS_I8,    // ... i8 rows
  PH_KF_ROWS_I8Q,   // ... i8 rows against an int8 query (integer dot products)
  PH_KF_PQ_TABLE,   // per-sub-space PQ, the query's table in LDS or global memory
  PH_KF_PQ_REG,     // ... the 8-bit table in registers (pqr_m sub-spaces)
  PH_KF_PQ_SHARED,  // shared-codebook PQ
  PH_KF_LATENCY,    // small batches over f32 rows
  PH_KF_INSTR,      // Hnsw::search_instrumented over f32 rows
  PH_KF_ROWS_BITS,  // throughput kernels over 1-bit sign rows (search_bits.hip; no filtered, collecting or radius twin)
};

// the register-table PQ policy (pick_pqr): 32 / 64 / 96 / 128 sub-spaces, queues of up to 512 entries
template <int FILT>
static ph_search_fn pick_kernel_pqr(int capc, int m) {
#define PH_KR(C, M) \
  if (capc == C && m == M) return (ph_search_fn)ph_search_kernel_pqr<C, M, FILT>;
  PH_KR(2, 32) PH_KR(2, 64) PH_KR(2, 96) PH_KR(2, 128)
  PH_KR(8, 32) PH_KR(8, 64) PH_KR(8, 96) PH_KR(8, 128)
#undef PH_KR
  return nullptr;
}

// shared-codebook PQ stores (u16 codes): the query layout is DistF32's, the candidate rows come through the codes
template <int FILT>
static ph_search_fn pick_kernel_pqs(int capc, int nv) {
#define PH_KS(C, N) \
  if (capc == C && nv == N) return (ph_search_fn)ph_search_kernel<C, DistPQS<N>, FILT>;
  PH_KS(2, 1) PH_KS(2, 3) PH_KS(2, 6) PH_KS(8, 1) PH_KS(8, 3) PH_KS(8, 6) PH_KS(16, 1) PH_KS(16, 3) PH_KS(16, 6)
#undef PH_KS
  return nullptr;
}

template <int FILT>
static ph_search_fn pick_kernel_dense(int capc) {
  switch (capc) {
    case 2: return (ph_search_fn)ph_search_kernel_dense<2, FILT>;
    case 4: return (ph_search_fn)ph_search_kernel_dense<4, FILT>;
    case 8: return (ph_search_fn)ph_search_kernel_dense<8, FILT>;
    case 16: return (ph_search_fn)ph_search_kernel_dense<16, FILT>;
  }
  return nullptr;
}

template <int FILT>
static ph_search_fn pick_kernel_lat(int capc, int nv) {
#define PH_KL(C, N) \
  if (capc == C && nv == N) return (ph_search_fn)ph_search_kernel_lat<C, N, FILT>;
  PH_KL(2, 1) PH_KL(2, 3) PH_KL(8, 1) PH_KL(8, 3)
#undef PH_KL
  return nullptr;
}

// The throughput kernels of a row store, D = DistF32 / DistF16 / DistI8 / DistI8Q: the same set shape for shape -- same
// queues, same LDS visited table, same rows in flight (DistI8Q too: 16 rows in flight would cost its headline kernel a
// wave per SIMD, 144 VGPRs against 112, profiles/i8q).  (There are no latency (U == 0), instrumented or big-queue kernels over
// converted rows: batches of any size run these, and the calls behind the others refuse a converted store.)
template <template <int, int> class D, int FILT>
static ph_search_fn pick_kernel_rows(int capc, int nv) {
#define PH_K(C, N) \
  if (capc == C && nv == N) return (ph_search_fn)ph_search_kernel<C, D<N, 4>, FILT>;
  PH_K(2, 1) PH_K(2, 3) PH_K(2, 6)
  // ef <= 256 at 768 dimensions (the headline): 8 rows in flight at 2 waves per SIMD, whose LDS share holds a visited
  // table of 3 520 slots -- 1.04 M q/s against 1.01 M for 4 rows at 3 waves per SIMD with 1 792 slots
  if (capc == 4 && nv == 3) return (ph_search_fn)ph_search_kernel<4, D<3, 8>, FILT>;
  PH_K(4, 6)
  PH_K(8, 1) PH_K(8, 3) PH_K(8, 6)
  PH_K(16, 1) PH_K(16, 3) PH_K(16, 6)
#undef PH_K
  return nullptr;
}

// the per-sub-space PQ policy with its table in LDS or in global memory (PHNSW_PQ_TABLE)
template <int FILT>
static ph_search_fn pick_kernel_pqt(int capc, bool global) {
#define PH_KQ(C) \
  if (capc == C) return global ? (ph_search_fn)ph_search_kernel<C, DistPQG, FILT> : (ph_search_fn)ph_search_kernel<C, DistPQ, FILT>;
  PH_KQ(2) PH_KQ(8) PH_KQ(16)
#undef PH_KQ
  return nullptr;
}

// the kernel of a plain search by family and shape (nullptr: none); FILT: its twin with the test of that filter mode
template <int FILT>
static ph_search_fn pick_kernel_family(int family, int capc, int nv, int pqr_m, bool pq_global) {
  switch (family) {
    case PH_KF_ROWS_F32: return pick_kernel_rows<DistF32, FILT>(capc, nv);
    case PH_KF_ROWS_F16: return pick_kernel_rows<DistF16, FILT>(capc, nv);
    case PH_KF_ROWS_I8: return pick_kernel_rows<DistI8, FILT>(capc, nv);
    case PH_KF_ROWS_I8Q: return pick_kernel_rows<DistI8Q, FILT>(capc, nv);
    case PH_KF_PQ_TABLE: return pick_kernel_pqt<FILT>(capc, pq_global);
    case PH_KF_PQ_REG: return pick_kernel_pqr<FILT>(capc, pqr_m);
    case PH_KF_PQ_SHARED: return pick_kernel_pqs<FILT>(capc, nv);
    case PH_KF_LATENCY: return pick_kernel_lat<FILT>(capc, nv);
    default: return nullptr;  // (search_instrumented, knn and threshold_nn take no filter)
  }
}

// the bitmap twins live in search_filtered.hip, the label twins in search_labeled.hip; the launchers of search.hip get
// them here
ph_search_fn ph_pick_filtered_kernel(int family, int capc, int nv, int pqr_m, bool pq_global);
ph_search_fn ph_pick_filtered_dense(int capc);
ph_search_fn ph_pick_labeled_kernel(int family, int capc, int nv, int pqr_m, bool pq_global);
ph_search_fn ph_pick_labeled_dense(int capc);
// the set twins: search_labelset.hip
ph_search_fn ph_pick_labelset_kernel(int family, int capc, int nv, int pqr_m, bool pq_global);
ph_search_fn ph_pick_labelset_dense(int capc);
// the set-range twins: search_labelset_ranged.hip
ph_search_fn ph_pick_labelset_ranged_kernel(int family, int capc, int nv, int pqr_m, bool pq_global);
ph_search_fn ph_pick_labelset_ranged_dense(int capc);
// the range twins: search_ranged.hip
ph_search_fn ph_pick_ranged_kernel(int family, int capc, int nv, int pqr_m, bool pq_global);
ph_search_fn ph_pick_ranged_dense(int capc);
// the label-range twins: search_label_ranged.hip
ph_search_fn ph_pick_label_ranged_kernel(int family, int capc, int nv, int pqr_m, bool pq_global);
ph_search_fn ph_pick_label_ranged_dense(int capc);
// the radius twins (PH_FM_RADIUS, no filter): search_radius.hip.  Row stores and the 1024-slot queues only; nullptr for
// every other family or shape
ph_search_fn ph_pick_radius_kernel(int family, int nv);
// the kernels of a bits store (search_bits.hip): queues of capc * 64 slots, capc in {2, 4, 8, 16}, nv in {1, 3, 6}; plain
// searches only -- pick_kernel_family has no case for the family, so no FILT twin of them exists
ph_search_fn ph_pick_kernel_bits(int capc, int nv);
// the collecting twins (PH_FM_COLLECT over the bitmap and over the label column): search_collect.hip and
// search_collect_labeled.hip.  No dense-only twin: a collecting kernel runs the last layer of a descent, and the
// dense-only launch of a split descent never holds it (api.hip)
ph_search_fn ph_pick_collect_kernel(int family, int capc, int nv, int pqr_m, bool pq_global);
ph_search_fn ph_pick_collect_labeled_kernel(int family, int capc, int nv, int pqr_m, bool pq_global);
