// The scan kernel of the exhaustive int8 scan, written once for its three forms, and what scan_i8q.hip (the plain form,
// the launcher, the scratch, the merge kernel, the host staging) and scan_i8q_filtered.hip (the forms over an allow-list)
// share.  The head of scan_i8q.hip says how the work is mapped; a form changes only WHICH rows a row tile holds and WHICH
// survivors may become keys, never a dot product (an integer sum has no order), so every form gives a (query, row) pair
// the same bits:
//   PLAIN  row tile t is rows T t .. T t + T - 1 (T = 16 tile_groups); a survivor is a key when its row is below n;
//   LIST   row tile t is POSITIONS T t .. T t + T - 1 of the ascending list `cand` of the m allowed rows of a SHARED bitmap
//          (compacted by scan_fp4_filtered.hip's ph_fp4_scan_list_enqueue, m read from device memory), the slices cut
//          over ceil(m / T) tiles, so a slice may be empty.  The 256 threads still move whole rows as coalesced dwordx4
//          runs into the same LDS tile; only the row a run comes from changes, and that row is now the result of a load.
//          The ids travel ONE REGISTER deep and otherwise through LDS: thread r < T loads the id of position T (t + 2) + r
//          together with the row loads of tile t + 1, writes it into slot (t + 2) & 3 of an ID RING in LDS beside the
//          tiles with the next `put`, and after that tile's barrier all 256 threads read the ids of their runs' rows
//          from the ring (ds_read, no global load in front of a row address).  The survivor path takes a key's id from
//          the same slot, one ds_read_b128 for a lane's four rows.  The one-barrier-a-tile double buffer keeps its
//          shape; only the first tile of a slice addresses its rows straight from the list.
//          A tile is up to 64 positions, the list is padded to 16: every position goes through ph_i8q_scan_list_pos
//          (i8q_scan_filter_plan.h) before it indexes the list, and a position at or past m is never a key;
//   MASK   PER-QUERY bitmaps: every tile is scanned as in the plain form and a survivor (dot >= smin) becomes a key only
//          if its bit is set in its own query's bitmap.  A lane's four accumulators are rows 4 (l / 16) + i of one group
//          and one query: four bits of one word, one dword load per (row group, wave) in which the lane has a survivor
//          below n, none otherwise.  smin tightens on allowed rows only.
// Per-wave ownership is as in the plain form: stages, lists and thresholds are touched by no other wave; the ring is
// written by wave 0 and read by all, between the same barriers as the tile it belongs to.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "exact_topk_wave.h"
#include "i8q_scan_filter_plan.h"
#include "i8q_scan_plan.h"
#include "phnsw_device.h"

#ifndef PH_TRY
#define PH_TRY(x)          \
  do {                     \
    int rc__ = (x);        \
    if (rc__) return rc__; \
  } while (0)
#endif

typedef int ph_v4i __attribute__((ext_vector_type(4)));

enum { PH_I8Q_SCAN_PLAIN = 0, PH_I8Q_SCAN_LIST = 1, PH_I8Q_SCAN_MASK = 2 };

struct PhI8qScanArgs {
  const uint8_t *rows;   // n rows of `stride` bytes: f32 scale, codes (RowI8)
  const uint8_t *qimg;   // [nq][ph_i8q_scan_query_bytes(steps)]
  const float *qscale;   // [nq]
  uint32_t stride, runs, steps, tile_groups;  // runs: 16-byte runs of a row that exist; stride >= 16 runs
  uint32_t nq, n, k;     // k: the r of the call (the name ph_exact_write_row reads)
  int metric;
  uint32_t qtiles, slices, stage;
  uint64_t row_tiles;
  uint64_t *lists;    // [qtiles * slices][64][2 k]: the running top-r of every (query, slice)
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

// the per-query state of a wave in LDS, four words
struct PhI8qScanState {
  uint32_t staged, len, flip;
  float smin;
};

template <int I, int N, class F>
__device__ __forceinline__ void ph_i8q_static_for(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>());
    ph_i8q_static_for<I + 1, N>(f);
  }
}

// the body of a scan workgroup (four waves); the kernels of the two translation units are this and nothing else.
// S: the step class; RG: the largest row tile of the class, in groups (ph_i8q_scan_tile_cap)
template <int S, int RG, int FORM>
__device__ __forceinline__ void ph_i8q_scan_body(const PhI8qScanArgs &a) {
  extern __shared__ uint64_t scan_lds[];
  constexpr int NL = (16 * RG * 4 * S + 255) / 256;  // ph_i8q_scan_loads
  constexpr bool LIST = FORM == PH_I8Q_SCAN_LIST;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, col = lane & 15u, kb = lane >> 4;
  const uint32_t pitch = ph_i8q_scan_pitch(a.steps), tile_bytes = 16u * a.tile_groups * pitch;
  uint8_t *const tiles = (uint8_t *)scan_lds;  // [2][16 tile_groups][pitch]
  uint64_t *const stage = scan_lds + (2u * tile_bytes + w * ph_i8q_scan_wave_bytes(a.k)) / 8u;  // [16][a.stage], this wave's
  uint64_t *const sv = stage + 16u * a.stage;                                                   // [64]
  PhI8qScanState *const state = (PhI8qScanState *)(sv + 64);                                    // [16]
  const uint32_t qtile = blockIdx.x % a.qtiles, slice = blockIdx.x / a.qtiles;
  const uint32_t q0 = qtile * PH_I8Q_SCAN_QTILE + 16u * w;  // this wave's first query
  const uint32_t tq = q0 < a.nq ? min(16u, a.nq - q0) : 0u;
  uint64_t *const lists = a.lists + ((uint64_t)blockIdx.x * PH_I8Q_SCAN_QTILE + 16u * w) * 2u * a.k;
  const bool half = a.metric == PHNSW_METRIC_COSINE_HALF;
  if (lane < 16u) state[lane] = PhI8qScanState{0u, 0u, 0u, lane < tq ? -INFINITY : INFINITY};
  ph_wave_sync();

  // the wave's queries: lane's run 4 s + kb of query column `col`; past the last query the last again
  const uint32_t q = min(q0 + col, a.nq - 1u);
  ph_v4i qc[S];
#pragma unroll
  for (int s = 0; s < S; s++)
    qc[s] = (uint32_t)s < a.steps ? *(const ph_v4i *)(a.qimg + (uint64_t)q * ph_i8q_scan_query_bytes(a.steps) + 16u * (4u * s + kb))
                                  : ph_v4i{0, 0, 0, 0};
  const float sq = a.qscale[q];
  float smin = col < tq ? -INFINITY : INFINITY;

  // LIST: m and with it the row tiles are the device's to know; the id ring [PH_I8Q_SCAN_ID_SLOTS][T] behind the waves'
  const uint32_t T = 16u * a.tile_groups;
  uint32_t m = 0u;
  uint64_t row_tiles = a.row_tiles;
  uint32_t *ring = nullptr;
  if constexpr (LIST) {
    m = a.count[0];
    row_tiles = ph_i8q_scan_list_tiles(m, a.tile_groups);
    ring = (uint32_t *)(scan_lds + ph_i8q_scan_lds(a.k, a.steps, a.tile_groups) / 8u);
  }
  // LIST: the row of position r of tile `tile`: a written entry of the list (the clamp), a row of the store
  auto listed = [&](uint64_t tile, uint32_t r) { return min(a.cand[ph_i8q_scan_list_pos(tile * T + r, m)], a.n - 1u); };

  // staging: the tile's 16 tile_groups x runs runs dealt to the threads in order, (row of the tile) << 16 | run; a
  // thread with nothing to move in a round loads row 0's first run again and drops it (bit 31)
  const uint32_t per_tile = 16u * a.tile_groups * a.runs;
  uint32_t lpos[NL];
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const uint32_t idx = tid + 256u * i;
    lpos[i] = idx < per_tile ? ((idx / a.runs) << 16) | (idx % a.runs) : 0x80000000u;
  }
  ph_v4i x[NL];
  // LIST: a run's row is the id of its position, from the tile's slot of the ring (ringed) or, for the first tile of a
  // slice, from the list itself
  auto fetch = [&](uint64_t tile, auto ringed) {
    if constexpr (LIST) {
      const uint32_t *const ids = ring + ph_i8q_scan_ids_slot(tile) * T;
#pragma unroll
      for (int i = 0; i < NL; i++) {
        const uint32_t r = (lpos[i] >> 16) & 0x7FFFu;
        uint32_t row;
        if constexpr (decltype(ringed)::value)
          row = ids[r];
        else
          row = listed(tile, r);
        x[i] = *(const ph_v4i *)(a.rows + (uint64_t)row * a.stride + 16u * (lpos[i] & 0xFFFFu));
      }
    } else {
      const uint32_t base = (uint32_t)(tile * 16u * a.tile_groups);
#pragma unroll
      for (int i = 0; i < NL; i++)
        x[i] = *(const ph_v4i *)(a.rows + (uint64_t)min(base + ((lpos[i] >> 16) & 0x7FFFu), a.n - 1u) * a.stride + 16u * (lpos[i] & 0xFFFFu));
    }
  };
  auto put = [&](uint32_t buf) {
#pragma unroll
    for (int i = 0; i < NL; i++)
      if (!(lpos[i] >> 31)) *(ph_v4i *)(tiles + buf * tile_bytes + (lpos[i] >> 16) * pitch + 16u * (lpos[i] & 0xFFFFu)) = x[i];
  };

  // the staged keys of query t into its running top-r; its threshold afterwards.  Whole wave, uniform control flow.
  auto flush = [&](uint32_t t) {
    PhI8qScanState *const st = state + t;
    const uint32_t staged = rfl32(st->staged);
    const uint64_t key = lane < staged ? stage[t * a.stage + lane] : KEY_NONE;
    PhWaveTopK top;
    top.cur = lists + (uint64_t)t * 2u * a.k, top.nxt = top.cur + a.k, top.sv = sv, top.k = a.k;
    if (rfl32(st->flip)) {
      uint64_t *const c = top.cur;
      top.cur = top.nxt, top.nxt = c;
    }
    top.len = rfl32(st->len);
    ph_wave_sync();  // the state read above is rewritten below
    top.insert(key, lane);
    ph_wave_sync();  // (insert returns without one when nothing survived)
    if (lane == 0) {
      st->len = top.len;
      st->flip = top.cur == lists + (uint64_t)t * 2u * a.k ? 0u : 1u;
      st->staged = 0u;
      st->smin = top.len == a.k ? ph_fp4_scan_smin(unfkey((uint32_t)(top.cur[a.k - 1u] >> 32)), half) : -INFINITY;
    }
    ph_wave_sync();
  };

  // one row group of a staged tile: rows (LIST: positions) row0 .. row0 + 15 at `grp` in LDS, LIST: their ids at `gids`
  auto scan = [&](const uint8_t *grp, uint32_t row0, const uint32_t *gids) {
    ph_v4i acc = {0, 0, 0, 0};
    const uint8_t *src = grp + col * pitch + 16u * kb;
    ph_i8q_static_for<0, S>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
      if ((uint32_t)s < a.steps)  // wave-uniform
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(*(const ph_v4i *)(src + 64u * s), qc[s], acc, 0, 0, 0);
    });
    float sr[4], dot[4];
    bool any = false;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      sr[i] = *(const float *)(grp + (4u * kb + i) * pitch);  // the row's scale, staged with its codes
      dot[i] = __fmul_rn(__fmul_rn(sq, sr[i]), (float)acc[i]);
      any |= dot[i] >= smin;
    }
    if (!__ballot(any)) return;
    if constexpr (FORM == PH_I8Q_SCAN_PLAIN) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t id = row0 + 4u * kb + i;
        if (id < a.n && dot[i] >= smin) {  // (smin of a query past the last is +inf)
          const uint32_t slot = atomicAdd(&state[col].staged, 1u);  // < a.stage: at most 16 rows on top of stage - 16
          stage[col * a.stage + slot] = mkkey(ph_i8q_distance(sq, sr[i], acc[i], a.metric), id);
        }
      }
    } else {
      const uint32_t base = row0 + 4u * kb;  // LIST: a position of the list, MASK: a row
      uint32_t ids[4] = {base, base + 1u, base + 2u, base + 3u}, allow = 0xFu;
      if constexpr (LIST) {
        const uint4 e = *(const uint4 *)(gids + 4u * kb);
        ids[0] = e.x, ids[1] = e.y, ids[2] = e.z, ids[3] = e.w;
      } else {
        // a tile may reach past 32 ceil(n / 32) rows, a bitmap does not: the word is read only for a row below n
        allow = any && base < a.n ? a.filter[(uint64_t)q * a.filter_stride + (base >> 5)] >> (base & 31u) : 0u;
      }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const bool live = LIST ? base + i < m : ids[i] < a.n;
        if (live && ((allow >> i) & 1u) && dot[i] >= smin) {
          const uint32_t slot = atomicAdd(&state[col].staged, 1u);
          stage[col * a.stage + slot] = mkkey(ph_i8q_distance(sq, sr[i], acc[i], a.metric), ids[i]);
        }
      }
    }
    ph_wave_sync();
    uint64_t full = __ballot(lane < 16u && state[lane & 15u].staged + 16u > a.stage);
    if (!full) return;
    for (; full; full &= full - 1ull) flush((uint32_t)__ffsll((unsigned long long)full) - 1u);
    smin = state[col].smin;
  };

  uint64_t t0, t1;
  ph_exact_slice_range(slice, a.slices, row_tiles, &t0, &t1);
  if (t0 < t1) {  // workgroup-uniform
    uint32_t ahead = 0u;  // LIST, thread r < T: the id of position r of the tile after the one whose rows were fetched last
    if constexpr (LIST)
      if (tid < T) {
        ring[ph_i8q_scan_ids_slot(t0) * T + tid] = listed(t0, tid);
        if (t0 + 1u < t1) ahead = listed(t0 + 1u, tid);
      }
    fetch(t0, std::false_type());
    uint32_t buf = 0u;
    for (uint64_t t = t0; t < t1; t++, buf ^= 1u) {
      put(buf);
      if constexpr (LIST)
        if (tid < T && t + 1u < t1) ring[ph_i8q_scan_ids_slot(t + 1u) * T + tid] = ahead;
      __syncthreads();  // the tile is whole; and every wave is done with the buffer the NEXT put rewrites
      if (t + 1u < t1) {
        fetch(t + 1u, std::true_type());
        if constexpr (LIST)
          if (tid < T && t + 2u < t1) ahead = listed(t + 2u, tid);
      }
      if (tq)  // (a wave of a partial last query tile has no query: it only stages)
        for (uint32_t g = 0; g < a.tile_groups; g++)
          scan(tiles + buf * tile_bytes + g * 16u * pitch, (uint32_t)(t * a.tile_groups + g) * 16u,
               LIST ? ring + ph_i8q_scan_ids_slot(t) * T + 16u * g : nullptr);
    }
  }
  for (uint32_t t = 0; t < tq; t++) {
    PhI8qScanState *const st = state + t;
    if (rfl32(st->staged)) flush(t);
    ph_exact_write_slice<false>(a, q0 + t, q0 + t, slice, lists + (uint64_t)t * 2u * a.k + (rfl32(st->flip) ? a.k : 0u), rfl32(st->len),
                                false, lane);
  }
}

// ------------------------------------------------------------------ host side, between the two translation units

typedef void (*PhI8qScanFn)(PhI8qScanArgs);
// scan_i8q_filtered.hip: the instance of a filtered form for a step class, nullptr if there is none
PhI8qScanFn ph_i8q_scan_filtered_fn(int cls, int form);
// scan_fp4_filtered.hip: the compaction of a shared bitmap of n rows into `pre` (ph_fp4_scan_pre_bytes(n) bytes of device
// memory), enqueued; nothing about it is fp4's but the name
int ph_fp4_scan_list_enqueue(const uint32_t *filter_dev, uint64_t n, uint32_t *pre, hipStream_t stream);

// scan_i8q.hip: what all the calls ask of the store, of r, of `full` and k, and of the device pointers; the scan of nq
// device queries on `stream` (filter_dev nullptr: every row; else a shared bitmap, stride 0, or nq bitmaps); the host
// forms' staging around it (filter: host words, or nullptr)
int ph_i8q_scan_check(const char *call, const phnsw_store *i8q, uint64_t nq, uint64_t r);
int ph_i8q_scan_search_check(const char *call, const phnsw_store *i8q, const phnsw_store *full, uint64_t nq, uint64_t r, uint64_t k);
int ph_i8q_scan_device_check(const char *call, const float *queries_dev, uint32_t ldq, uint32_t ld_min, bool aligned,
                             const void *ids, const void *d, const void *len);
int ph_i8q_scan_enqueue(const phnsw_store *s, const float *queries_dev, uint32_t ldq, uint64_t nq, uint32_t r,
                        const uint32_t *filter_dev, uint32_t filter_stride, uint32_t *out_ids, float *out_d, uint32_t *out_len,
                        hipStream_t stream);
int ph_i8q_scan_host(const char *call, const phnsw_store *i8q, const phnsw_store *full, const float *queries, uint64_t nq,
                     uint32_t r, uint32_t k, const uint32_t *filter, uint32_t filter_stride, uint64_t *out_ids, float *out_d,
                     uint64_t *out_len);
