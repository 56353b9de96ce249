// The scan kernel of the exhaustive MXFP4 scan, written once for its three forms, and what scan_fp4.hip (the plain form,
// the launcher, the host staging) and scan_fp4_filtered.hip (the forms over an allow-list, the compaction of a shared
// bitmap) share.  The head of scan_fp4.hip says how the work is mapped; a form changes only WHICH rows a row group
// holds and WHICH survivors may become keys, never how a score is computed:
//   PLAIN  row group g is rows 16 g .. 16 g + 15; a survivor is a key when its row is below n;
//   LIST   row group g is entries 16 g .. 16 g + 15 of the ascending list `cand` of the m allowed rows of a SHARED bitmap
//          (fp4_scan_filter_plan.h: padded to whole groups with its last id), m read from device memory.  A lane takes
//          its operand from the row its entry names -- the same dwordx4 loads from an address it computes -- and a
//          survivor is a key when its POSITION is below m, its id the entry at that position (one aligned dwordx4 on the
//          survivor path only).  The slices cut ceil(m / 16) groups, so a slice may be empty.
//          Prefetch: a row address now depends on a load.  Rows stay ONE group ahead of the MFMAs as in the plain
//          form, and the entry that addresses them is fetched ONE GROUP BEFORE THAT (two ahead of the MFMAs), issued
//          together with the row loads: it then has a whole group's MFMAs (12 to 48 block-scaled instructions and the
//          row loads' own latency) to arrive, costs one VGPR, and is a 64-byte read of a list that streams through L2.
//          Deeper buys nothing (the rows, not the ids, are the long loads) and would hold ids of groups whose rows
//          cannot be issued yet without a third row buffer (24 to 48 VGPRs the <6,4> and <12,2> instances do not have);
//   MASK   PER-QUERY bitmaps: every row group is scanned as in the plain form and a raw survivor becomes a key only if its
//          bit is set in its own query's bitmap.  A lane's four accumulators are rows 4 (l / 16) + i of one group and one
//          query: four bits of one word, one dword load per (row group, query group) in which the lane has a
//          survivor, none otherwise.  smin tightens on allowed rows only, so while a selective filter keeps a list short
//          every pair is a survivor and is tested.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "exact_topk.h"
#include "fp4_scan_filter_plan.h"
#include "fp4_scan_plan.h"
#include "phnsw_device.h"

#define PH_TRY(x)          \
  do {                     \
    int rc__ = (x);        \
    if (rc__) return rc__; \
  } while (0)

typedef int ph_v8i __attribute__((ext_vector_type(8)));
typedef float ph_v4f __attribute__((ext_vector_type(4)));

enum { PH_FP4_SCAN_PLAIN = 0, PH_FP4_SCAN_LIST = 1, PH_FP4_SCAN_MASK = 2 };

struct PhFp4ScanArgs {
  const uint8_t *rows;      // n rows of `stride` bytes, the device layout of phnsw_device.h
  const uint8_t *qcodes;    // [nq][ph_fp4_scan_code_bytes(steps)]
  const uint8_t *qscales;   // [nq][ph_fp4_scan_scale_bytes(steps)]
  uint32_t stride, nb, steps;  // nb: blocks of a row that exist, ceil(ld / 32)
  uint32_t nq, n, k;           // k: the r of the call (the name ph_exact_write_row reads)
  int metric;
  uint32_t tiles, slices, stage;
  uint64_t groups;
  uint64_t *lists;    // [tiles * slices][T][2 k]: the running top-r of every (query, slice)
  uint64_t *scratch;  // slices > 1: [nq][slices][k] keys, each list ascending, KEY_NONE padded
  uint32_t *out_ids;  // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
  // the filtered forms only
  const uint32_t *cand;    // LIST: the ascending row list, ph_fp4_scan_list_len(m) entries
  const uint32_t *count;   // LIST: [0] = m
  const uint32_t *filter;  // MASK: the bitmap of the launch's first query
  uint32_t filter_stride;  // MASK: words from one query's bitmap to the next, >= ceil(n / 32)
};

template <int I, int N, class F>
__device__ __forceinline__ void ph_static_for(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>());
    ph_static_for<I + 1, N>(f);
  }
}

// one lane's operand of a row group: 16 code bytes a step; the scale dwords of (section, step parity)
template <int S>
struct PhFp4RowRegs {
  uint4 c[S];
  uint32_t sc[2 * ((S + 7) / 8)];
};

// the per-query state of a tile in LDS, four words
struct PhFp4ScanState {
  uint32_t staged, len, flip;
  float smin;
};

// the body of a scan workgroup (one wave64); the kernels of the two translation units are this and nothing else
template <int S, int G, int FORM>
__device__ __forceinline__ void ph_fp4_scan_body(const PhFp4ScanArgs &a) {
  extern __shared__ uint64_t scan_lds[];
  constexpr uint32_t T = 16u * G;
  constexpr int SEC = (S + 7) / 8, QW = (S + 3) / 4;
  const uint32_t lane = threadIdx.x, col = lane & 15u, kb = lane >> 4;
  uint64_t *const stage = scan_lds;                     // [T][a.stage]
  uint64_t *const sv = scan_lds + (uint64_t)T * a.stage;  // [64]
  PhFp4ScanState *const state = (PhFp4ScanState *)(sv + 64);
  const uint32_t tile = blockIdx.x % a.tiles, slice = blockIdx.x / a.tiles;
  const uint32_t q0 = tile * T, tq = min(T, a.nq - q0);
  uint64_t *const lists = a.lists + (uint64_t)blockIdx.x * T * 2u * a.k;
  const bool half = a.metric == PHNSW_METRIC_COSINE_HALF;
  for (uint32_t t = lane; t < T; t += 64u) state[t] = PhFp4ScanState{0u, 0u, 0u, t < tq ? -INFINITY : INFINITY};
  __syncthreads();

  // the tile's queries: lane's block 4 s + kb of query column `col` of every group; past the last query the last again
  uint4 qc[G][S];
  uint32_t qs[G][QW];
#pragma unroll
  for (int g = 0; g < G; g++) {
    const uint32_t q = min(q0 + 16u * g + col, a.nq - 1u);
    const uint8_t *cq = a.qcodes + (uint64_t)q * ph_fp4_scan_code_bytes(a.steps);
    const uint8_t *sq = a.qscales + (uint64_t)q * ph_fp4_scan_scale_bytes(a.steps) + kb * ph_fp4_scan_scale_run(a.steps);
#pragma unroll
    for (int s = 0; s < S; s++) qc[g][s] = (uint32_t)s < a.steps ? *(const uint4 *)(cq + (4u * s + kb) * 16u) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int w = 0; w < QW; w++) qs[g][w] = 4u * w < a.steps ? *(const uint32_t *)(sq + 4u * w) : 0x7F7F7F7Fu;
  }
  float smin[G];
#pragma unroll
  for (int g = 0; g < G; g++) smin[g] = 16u * g + col < tq ? -INFINITY : INFINITY;

  // LIST: m and with it the row groups are the device's to know
  uint32_t m = 0u;
  uint64_t groups = a.groups;
  if constexpr (FORM == PH_FP4_SCAN_LIST) {
    m = a.count[0];
    groups = ph_fp4_scan_list_groups(m);
  }
  uint64_t g0, g1;
  ph_exact_slice_range(slice, a.slices, groups, &g0, &g1);

  // the row of lane's operand of row group `grp` (LIST: an entry of the padded list, a row of the store)
  auto rowof = [&](uint64_t grp) {
    if constexpr (FORM == PH_FP4_SCAN_LIST)
      return min(a.cand[grp * 16u + col], a.n - 1u);
    else
      return min((uint32_t)(grp * 16u) + col, a.n - 1u);
  };
  // lane's operand of a row group from row `row`
  auto load = [&](PhFp4RowRegs<S> &x, uint32_t row) {
    const uint8_t *src = a.rows + (uint64_t)row * a.stride;
#pragma unroll
    for (int s = 0; s < S; s++) {
      const uint32_t blk = 4u * s + kb;
      x.c[s] = blk < a.nb ? *(const uint4 *)(src + 544u * (s >> 3) + 32u + 16u * (4u * (s & 7) + kb)) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int w = 0; w < 2 * SEC; w++)  // a section that exists has its 32 scale bytes, every one a valid E8M0
      x.sc[w] = 32u * (w >> 1) < a.nb ? *(const uint32_t *)(src + 544u * (w >> 1) + 16u * (w & 1) + 4u * kb) : 0x7F7F7F7Fu;
  };

  // the staged keys of query t into its running top-r; its threshold afterwards.  Whole wave, uniform control flow.
  auto flush = [&](uint32_t t) {
    PhFp4ScanState *const st = state + t;
    const uint32_t staged = rfl32(st->staged);
    const uint64_t key = lane < staged ? stage[t * a.stage + lane] : KEY_NONE;
    PhExactTopK top;
    top.init(lists + (uint64_t)t * 2u * a.k, a.k);
    top.sv = sv;
    if (rfl32(st->flip)) {
      uint64_t *const c = top.cur;
      top.cur = top.nxt, top.nxt = c;
    }
    top.len = rfl32(st->len);
    __syncthreads();  // the state read above is rewritten below
    top.insert(key, lane);
    __syncthreads();  // (insert returns without one when nothing survived)
    if (lane == 0) {
      st->len = top.len;
      st->flip = top.cur == lists + (uint64_t)t * 2u * a.k ? 0u : 1u;
      st->staged = 0u;
      st->smin = top.len == a.k ? ph_fp4_scan_smin(unfkey((uint32_t)(top.cur[a.k - 1u] >> 32)), half) : -INFINITY;
    }
    __syncthreads();
  };

  auto scan = [&](const PhFp4RowRegs<S> &x, uint64_t grp) {
    ph_v4f acc[G];
#pragma unroll
    for (int g = 0; g < G; g++) acc[g] = ph_v4f{0.f, 0.f, 0.f, 0.f};
    ph_static_for<0, S>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
      if ((uint32_t)s < a.steps) {  // wave-uniform
        const ph_v8i ra = {(int)x.c[s].x, (int)x.c[s].y, (int)x.c[s].z, (int)x.c[s].w, 0, 0, 0, 0};
        const int sa = (int)x.sc[2 * (s >> 3) + (s & 1)];
#pragma unroll
        for (int g = 0; g < G; g++) {
          const ph_v8i rb = {(int)qc[g][s].x, (int)qc[g][s].y, (int)qc[g][s].z, (int)qc[g][s].w, 0, 0, 0, 0};
          acc[g] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ra, rb, acc[g], 4, 4, (s & 7) >> 1, sa, s & 3, (int)qs[g][s >> 2]);
        }
      }
    });
    bool any = false;
#pragma unroll
    for (int g = 0; g < G; g++)
      any |= acc[g][0] >= smin[g] || acc[g][1] >= smin[g] || acc[g][2] >= smin[g] || acc[g][3] >= smin[g];
    if (!__ballot(any)) return;
    const uint32_t row0 = (uint32_t)(grp * 16u) + 4u * kb;  // LIST: a position of the list, else a row
    uint32_t ids[4] = {row0, row0 + 1u, row0 + 2u, row0 + 3u};
    if constexpr (FORM == PH_FP4_SCAN_LIST) {
      const uint4 e = *(const uint4 *)(a.cand + row0);  // inside the padded list: row0 + 3 < 16 groups
      ids[0] = e.x, ids[1] = e.y, ids[2] = e.z, ids[3] = e.w;
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
      uint32_t allow = 0xFu;
      if constexpr (FORM == PH_FP4_SCAN_MASK) {
        // the word exists: 16 groups <= 32 ceil(n / 32) <= 32 filter_stride
        const bool hit = acc[g][0] >= smin[g] || acc[g][1] >= smin[g] || acc[g][2] >= smin[g] || acc[g][3] >= smin[g];
        allow = hit ? a.filter[(uint64_t)min(q0 + 16u * g + col, a.nq - 1u) * a.filter_stride + (row0 >> 5)] >> (row0 & 31u) : 0u;
      }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t id = ids[i];
        const bool live = FORM == PH_FP4_SCAN_LIST ? row0 + i < m : id < a.n;
        if (live && ((allow >> i) & 1u) && acc[g][i] >= smin[g]) {  // (smin of a query past the last is +inf)
          const uint32_t t = 16u * g + col;
          const uint32_t slot = atomicAdd(&state[t].staged, 1u);  // < a.stage: at most 16 rows on top of stage - 16
          stage[t * a.stage + slot] = mkkey(finalize_metric(acc[g][i], a.metric), id);
        }
      }
    }
    __syncthreads();
    uint64_t full = __ballot(lane < T && state[lane < T ? lane : 0u].staged + 16u > a.stage);
    if (!full) return;
    for (; full; full &= full - 1ull) flush((uint32_t)__ffsll((unsigned long long)full) - 1u);
#pragma unroll
    for (int g = 0; g < G; g++) smin[g] = state[16u * g + col].smin;
  };

  if (g0 < g1) {
    PhFp4RowRegs<S> xa, xb;
    uint32_t ahead = 0u;  // LIST: the row of the group after the one whose loads were issued last
    // the loads of row group grp; LIST: with them the entry that will address group grp + 1
    auto fetch = [&](PhFp4RowRegs<S> &x, uint64_t grp) {
      if constexpr (FORM == PH_FP4_SCAN_LIST) {
        const uint32_t row = ahead;
        if (grp + 1u < g1) ahead = rowof(grp + 1u);
        load(x, row);
      } else {
        load(x, rowof(grp));
      }
    };
    if constexpr (FORM == PH_FP4_SCAN_LIST) ahead = rowof(g0);
    fetch(xa, g0);
    for (uint64_t grp = g0; grp < g1; grp += 2u) {
      if (grp + 1u < g1) fetch(xb, grp + 1u);
      scan(xa, grp);
      if (grp + 1u >= g1) break;
      if (grp + 2u < g1) fetch(xa, grp + 2u);
      scan(xb, grp + 1u);
    }
  }
  for (uint32_t t = 0; t < tq; t++) {
    PhFp4ScanState *const st = state + t;
    if (rfl32(st->staged)) flush(t);
    ph_exact_write_slice<false>(a, q0 + t, q0 + t, slice, lists + (uint64_t)t * 2u * a.k + (rfl32(st->flip) ? a.k : 0u), rfl32(st->len),
                                false, lane);
  }
}

// ------------------------------------------------------------------ host side, between the two translation units

typedef void (*PhFp4ScanFn)(PhFp4ScanArgs);
// scan_fp4_filtered.hip: the instance of a filtered form for (step class, tile), nullptr if there is none; and the
// compaction of a shared bitmap of n rows into `pre` (ph_fp4_scan_pre_bytes(n) bytes of device memory), enqueued
PhFp4ScanFn ph_fp4_scan_filtered_fn(int cls, uint32_t T, int form);
int ph_fp4_scan_list_enqueue(const uint32_t *filter_dev, uint64_t n, uint32_t *pre, hipStream_t stream);

// scan_fp4.hip: what all the calls ask of the store, of r, of `full` and k, and of the device pointers; the scan of nq
// device queries on `stream` (filter_dev nullptr: every row; else a shared bitmap, stride 0, or nq bitmaps); the host
// forms' staging around it (filter: host words, or nullptr)
int ph_fp4_scan_check(const char *call, const phnsw_store *fp4, uint64_t nq, uint64_t r);
int ph_fp4_scan_search_check(const char *call, const phnsw_store *fp4, const phnsw_store *full, uint64_t nq, uint64_t r, uint64_t k);
int ph_fp4_scan_device_check(const char *call, const float *queries_dev, uint32_t ldq, uint32_t ld_min, bool aligned,
                             const void *ids, const void *d, const void *len);
int ph_fp4_scan_enqueue(const phnsw_store *s, const float *queries_dev, uint32_t ldq, uint64_t nq, uint32_t r,
                        const uint32_t *filter_dev, uint32_t filter_stride, uint32_t *out_ids, float *out_d, uint32_t *out_len,
                        hipStream_t stream);
int ph_fp4_scan_host(const char *call, const phnsw_store *fp4, const phnsw_store *full, const float *queries, uint64_t nq,
                     uint32_t r, uint32_t k, const uint32_t *filter, uint32_t filter_stride, uint64_t *out_ids, float *out_d,
                     uint64_t *out_len);
