// The exhaustive int8 scan over an i8q store (PH_ROWS_I8Q, rowstore.hip) on the matrix cores:
// phnsw_i8q_scan_topk[_device], the r rows nearest each query by the store's own distance, and
// phnsw_i8q_scan_search[_device], that scan followed by the f32 re-rank of pq.hip.  No index, no filter, no exclude:
// every row 0 .. n - 1 is a candidate.  An i8q store is never L2.
//
//   result of a query = the min(r, n) rows with the smallest (ph_i8q_distance(sq, sr, idot, metric), id), ascending.
//   idot              = the exact int32 dot product of the query's codes (ph_i8_scale / ph_i8_quant, the bits of
//                       DistI8Q::prepare_raw) and the row's: |idot| <= 1536 * 127^2 < 2^31, and an integer sum has no order.
//
// How the work is mapped (i8q_scan_plan.h has the rules):
//   * a row's codes start at byte 4 of the row, behind its scale, so no 16 codes are 16-byte aligned.  The scan
//     multiplies IMAGES instead: 16-byte RUNS of the row as it is stored, scale bytes included, against a query image
//     that has four zero bytes in their place.  Every load is an aligned dwordx4 and the scale arrives with the codes;
//     the price is four bytes, which is one more step where 4 + ld passes a multiple of 64 (13 instead of 12 at 768);
//   * ph_i8q_scan_query_kernel quantises the launch's queries into such images, and sq[nq];
//   * a workgroup of FOUR waves takes 64 queries and a slice of the row tiles.  Each wave keeps ITS OWN 16 queries in
//     registers for the whole slice (4 VGPRs a step: lane l holds run 4 s + l / 16 of query l % 16) and owns them
//     whole: its stages, its running top-r lists and its thresholds are touched by no other wave;
//   * a ROW TILE (16, 32 or 64 rows) is staged in LDS once by all 256 threads, coalesced dwordx4 loads of whole rows, and
//     read from there by every wave: a row byte crosses the L1 / L2 path once per 64 queries.  Two tiles are resident:
//     a tile's loads are issued into registers before the previous tile's MFMAs and written to the other buffer after
//     them, so ONE barrier a tile is enough (a buffer is rewritten two barriers after it was read) and these are the
//     kernel's only barriers.  Rows at or past n read row n - 1 and are never candidates;
//   * a row group is one v_mfma_i32_16x16x64_i8 a step: lane l's A operand is run 4 s + l / 16 of row l % 16 (one
//     ds_read_b128; the odd run pitch keeps 16 rows apart in the banks), its four accumulators belong to ONE query
//     (column l % 16) and rows 4 (l / 16) + i.  A step past the row's last is not issued; runs past the row's last inside
//     a step meet zero bytes of the query;
//   * selection: dot = fmul(fmul(sq, sr), (float)idot), the first two operations of ph_i8q_distance, against the query's
//     smin (ph_fp4_scan_smin, conservative for the metric's last step): one ballot per row group, and most end there.
//     Survivors become keys mkkey(ph_i8q_distance(...), id), staged per query in the wave's LDS; a stage that could not
//     take another 16 is flushed through PhWaveTopK::insert (exact_topk_wave.h), whose lists live in scratch.  insert
//     tests every key again, so no threshold changes a result;
//   * with more than one slice the lists go to [queries][slices][r] and ph_i8q_scan_merge_kernel feeds them through
//     the same running top-r (PH_EXACT_FEED).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "exact_topk_wave.h"
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

// one wave per query: the query's scale and its image -- four zero bytes, then the codes by the store's own quantiser
// (component order = byte order, as ph_i8_convert_kernel writes a row), zeros to the end of the last step
__global__ __launch_bounds__(256) void ph_i8q_scan_query_kernel(const float *__restrict__ queries, uint32_t ldq, uint32_t dim,
                                                                uint32_t nq, uint32_t steps, uint32_t *__restrict__ img,
                                                                float *__restrict__ scale) {
  const uint32_t lane = threadIdx.x & 63u, words = 16u * steps;
  for (uint64_t q = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); q < nq; q += (uint64_t)gridDim.x * 4u) {
    const float *src = queries + q * ldq;
    float m = 0.f;
    for (uint32_t c = lane; c < dim; c += 64u) m = fmaxf(m, fabsf(src[c]));
    const float sq = ph_i8_scale(wave_max(m));
    uint32_t *dst = img + q * words;
    for (uint32_t w = lane; w < words; w += 64u) {
      uint32_t word = 0u;
      if (w)
#pragma unroll
        for (uint32_t e = 0; e < 4u; e++) {
          const uint32_t c = 4u * (w - 1u) + e;
          if (c < dim) word |= ((uint32_t)ph_i8_quant(src[c], sq) & 0xFFu) << (8u * e);
        }
      dst[w] = word;
    }
    if (lane == 0) scale[q] = sq;
  }
}

// S: the step class; RG: the largest row tile of the class, in groups (ph_i8q_scan_tile_cap)
template <int S, int RG>
__global__ __launch_bounds__(256) void ph_i8q_scan_kernel(PhI8qScanArgs a) {
  extern __shared__ uint64_t scan_lds[];
  constexpr int NL = (16 * RG * 4 * S + 255) / 256;  // ph_i8q_scan_loads
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
  auto fetch = [&](uint64_t tile) {
    const uint32_t base = (uint32_t)(tile * 16u * a.tile_groups);
#pragma unroll
    for (int i = 0; i < NL; i++)
      x[i] = *(const ph_v4i *)(a.rows + (uint64_t)min(base + ((lpos[i] >> 16) & 0x7FFFu), a.n - 1u) * a.stride + 16u * (lpos[i] & 0xFFFFu));
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

  // one row group of a staged tile: rows row0 .. row0 + 15 at `grp` in LDS
  auto scan = [&](const uint8_t *grp, uint32_t row0) {
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
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t id = row0 + 4u * kb + i;
      if (id < a.n && dot[i] >= smin) {  // (smin of a query past the last is +inf)
        const uint32_t slot = atomicAdd(&state[col].staged, 1u);  // < a.stage: at most 16 rows on top of stage - 16
        stage[col * a.stage + slot] = mkkey(ph_i8q_distance(sq, sr[i], acc[i], a.metric), id);
      }
    }
    ph_wave_sync();
    uint64_t full = __ballot(lane < 16u && state[lane & 15u].staged + 16u > a.stage);
    if (!full) return;
    for (; full; full &= full - 1ull) flush((uint32_t)__ffsll((unsigned long long)full) - 1u);
    smin = state[col].smin;
  };

  uint64_t t0, t1;
  ph_exact_slice_range(slice, a.slices, a.row_tiles, &t0, &t1);
  if (t0 < t1) {  // workgroup-uniform
    fetch(t0);
    uint32_t buf = 0u;
    for (uint64_t t = t0; t < t1; t++, buf ^= 1u) {
      put(buf);
      __syncthreads();  // the tile is whole; and every wave is done with the buffer the NEXT put rewrites
      if (t + 1u < t1) fetch(t + 1u);
      if (tq)  // (a wave of a partial last query tile has no query: it only stages)
        for (uint32_t g = 0; g < a.tile_groups; g++)
          scan(tiles + buf * tile_bytes + g * 16u * pitch, (uint32_t)(t * a.tile_groups + g) * 16u);
    }
  }
  for (uint32_t t = 0; t < tq; t++) {
    PhI8qScanState *const st = state + t;
    if (rfl32(st->staged)) flush(t);
    ph_exact_write_slice<false>(a, q0 + t, q0 + t, slice, lists + (uint64_t)t * 2u * a.k + (rfl32(st->flip) ? a.k : 0u), rfl32(st->len),
                                false, lane);
  }
}

// One wave per query: the slices' ascending lists merged through the same running top-r.
__global__ __launch_bounds__(64) void ph_i8q_scan_merge_kernel(PhI8qScanArgs a) {
  extern __shared__ uint64_t scan_lds[];
  const uint32_t lane = threadIdx.x;
  for (uint32_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
    __syncthreads();
    PhExactTopK top;
    top.init(scan_lds, a.k);
    for (uint32_t s = 0; s < a.slices; s++) PH_EXACT_FEED(top, a.scratch + ((uint64_t)q * a.slices + s) * a.k, a.k, lane);
    ph_exact_write_row(a, q, top.cur, top.len, false, lane);
  }
}

// ------------------------------------------------------------------ launchers

typedef void (*PhI8qScanFn)(PhI8qScanArgs);
static PhI8qScanFn scan_fn(int cls) {  // the tile caps are ph_i8q_scan_tile_cap's
  switch (cls) {
    case 2: return ph_i8q_scan_kernel<2, 4>;
    case 7: return ph_i8q_scan_kernel<7, 4>;
    case 13: return ph_i8q_scan_kernel<13, 2>;
    case 25: return ph_i8q_scan_kernel<25, 1>;
    default: return nullptr;
  }
}

// The scratch of a scan: the prepared queries, a status word per query (ph_exact_write_row's; always ST_OK here) and
// the lists, kept PER DEVICE as scan_fp4.hip keeps its own: two blocks a device, used alternately so that scans on two
// streams may overlap; `done` closes the last launch that used a block and the next user's stream waits for it.
// g_mutex is held while a call enqueues its launches.
namespace {
struct ScanScratch {
  void *mem = nullptr;
  size_t bytes = 0;
  hipEvent_t done = nullptr;
};
struct DeviceScratch {
  ScanScratch block[2];
  unsigned next = 0;
};
std::mutex g_mutex;
std::map<int, DeviceScratch> g_scratch;    // under g_mutex
std::map<int, PhResidentMemo> g_resident;  // per device; an entry is handed to ph_resident_waves under g_resident_mutex
std::mutex g_resident_mutex;

int scratch_acquire(int device, size_t bytes, hipStream_t stream, ScanScratch **out) {
  DeviceScratch &d = g_scratch[device];
  ScanScratch &x = d.block[d.next++ & 1u];
  if (!x.done) PH_HIP(hipEventCreateWithFlags(&x.done, hipEventDisableTiming));
  if (x.bytes < bytes) {
    if (x.mem) {
      PH_HIP(hipEventSynchronize(x.done));  // the block is freed: nothing may still use it
      hipFree(x.mem);
      x.mem = nullptr, x.bytes = 0;
    }
    PH_HIP(hipMalloc(&x.mem, bytes));
    x.bytes = bytes;
  } else {
    PH_HIP(hipStreamWaitEvent(stream, x.done, 0));
  }
  *out = &x;
  return 0;
}
size_t up256(size_t b) { return (b + 255u) & ~(size_t)255u; }
}  // namespace

// the scan of nq device queries on `stream` (arguments checked by the caller): rows [nq][r] u32 ids and distances, len
static int i8q_scan_enqueue(const phnsw_store *s, const float *queries_dev, uint32_t ldq, uint64_t nq, uint32_t r,
                            uint32_t *out_ids, float *out_d, uint32_t *out_len, hipStream_t stream) {
  if (nq == 0) return 0;
  PH_HIP(hipSetDevice(s->device));
  const uint32_t steps = ph_i8q_scan_steps(s->ld), runs = ph_i8q_scan_runs(s->ld);
  const int cls = s->ld <= PH_I8Q_SCAN_LD_MAX ? ph_i8q_scan_class(steps) : 0;
  const PhI8qScanFn fn = scan_fn(cls);
  if (!fn || s->packed_stride < 16u * runs || s->packed_stride % 16u) return ph_dim_unsupported(s->dim);
  const uint32_t tg = ph_i8q_scan_tile(cls, env_ll("PHNSW_I8Q_SCAN_TILE"));  // tests and tuning: neither changes a result
  const size_t lds = ph_i8q_scan_lds(r, steps, tg), merge_lds = ph_i8q_scan_merge_lds(r);
  uint64_t resident = 0;  // workgroups of the scan the device holds at once (LDS decides, so the probe's block size does not)
  PhResidentMemo *memo;
  {
    std::lock_guard<std::mutex> g(g_resident_mutex);
    memo = &g_resident[s->device];
  }
  PH_TRY(ph_resident_waves(*memo, g_resident_mutex, s->device, (const void *)fn, lds, &resident));
  const uint64_t row_tiles = ph_i8q_scan_row_tiles(s->n, tg);
  const uint64_t first = std::min<uint64_t>(nq, PH_FP4_SCAN_CHUNK_MAX);
  const uint32_t slices = ph_i8q_scan_slices(ph_i8q_scan_qtiles(first), resident, row_tiles, env_ll("PHNSW_I8Q_SCAN_SLICES"), r);
  const uint64_t chunk = std::min<uint64_t>(nq, ph_i8q_scan_chunk(slices, r));
  const uint64_t chunk_tiles = ph_i8q_scan_qtiles(chunk);
  const size_t img_bytes = up256((size_t)chunk * ph_i8q_scan_query_bytes(steps));
  const size_t scale_bytes = up256((size_t)chunk * 4u), status_bytes = up256((size_t)chunk * 4u);
  const size_t lists_bytes = up256((size_t)chunk_tiles * PH_I8Q_SCAN_QTILE * slices * 2u * r * 8u);
  const size_t merge_bytes = slices > 1u ? up256((size_t)chunk * slices * r * 8u) : 0u;  // together: ph_i8q_scan_scratch_bytes
  const size_t bytes = img_bytes + scale_bytes + status_bytes + lists_bytes + merge_bytes;

  std::lock_guard<std::mutex> g(g_mutex);
  ScanScratch *x = nullptr;
  PH_TRY(scratch_acquire(s->device, bytes, stream, &x));
  char *at_mem = (char *)x->mem;
  PhI8qScanArgs a = {};
  a.rows = (const uint8_t *)s->packed, a.stride = s->packed_stride, a.runs = runs, a.steps = steps, a.tile_groups = tg;
  a.n = (uint32_t)s->n, a.k = r, a.metric = s->metric, a.slices = slices, a.stage = ph_fp4_scan_stage(r), a.row_tiles = row_tiles;
  a.qimg = (const uint8_t *)at_mem, at_mem += img_bytes;
  a.qscale = (const float *)at_mem, at_mem += scale_bytes;
  a.status = (uint32_t *)at_mem, at_mem += status_bytes;
  a.lists = (uint64_t *)at_mem, at_mem += lists_bytes;
  a.scratch = (uint64_t *)at_mem, at_mem += merge_bytes;
  for (uint64_t at = 0; at < nq; at += chunk) {
    const uint64_t cnt = std::min(chunk, nq - at);
    a.nq = (uint32_t)cnt, a.qtiles = (uint32_t)ph_i8q_scan_qtiles(cnt);
    a.out_ids = out_ids + at * r, a.out_d = out_d + at * r, a.out_len = out_len + at;
    hipLaunchKernelGGL(ph_i8q_scan_query_kernel, dim3((uint32_t)std::min<uint64_t>((cnt + 3u) / 4u, 1u << 16)), dim3(256), 0, stream,
                       queries_dev + at * ldq, ldq, s->dim, (uint32_t)cnt, steps, (uint32_t *)a.qimg, (float *)a.qscale);
    hipLaunchKernelGGL(fn, dim3(a.qtiles * slices), dim3(PH_I8Q_SCAN_THREADS), lds, stream, a);
    if (slices > 1u)
      hipLaunchKernelGGL(ph_i8q_scan_merge_kernel, dim3((uint32_t)std::min<uint64_t>(cnt, 1u << 20)), dim3(64), merge_lds, stream, a);
    PH_HIP(hipGetLastError());
  }
  PH_HIP(hipEventRecord(x->done, stream));
  return 0;
}

// ------------------------------------------------------------------ entry points

// what all four calls ask of the store and of r (an i8q store is never L2: phnsw_store_create_i8q refuses it)
static int i8q_scan_check(const char *call, const phnsw_store *i8q, uint64_t nq, uint64_t r) {
  if (!i8q || i8q->kind != PH_ROWS_I8Q) {
    ph_set_error("%s: needs an i8q store (phnsw_store_create_i8q), not %s", call, i8q ? ph_rows_name(i8q->kind) : "NULL");
    return PHNSW_E_UNSUPPORTED;
  }
  if (!ph_i8q_scan_r_valid(r) || nq > 0xFFFFFFFFull || i8q->n > 0x7FFFFFFFull) {
    ph_set_error("%s: needs 1 <= r <= %u, at most 2^32 - 1 queries and at most 2^31 - 1 rows", call, PH_I8Q_SCAN_RMAX);
    return PHNSW_E_INVALID;
  }
  return 0;
}
// ... and the searches of `full` and k: what rerank_check (pq.hip) demands of a converted store
static int i8q_scan_search_check(const char *call, const phnsw_store *i8q, const phnsw_store *full, uint64_t nq, uint64_t r,
                                 uint64_t k) {
  PH_TRY(i8q_scan_check(call, i8q, nq, r));
  if (!full || !ph_store_f32(full) || full->n != i8q->n || full->dim != i8q->dim || full->metric != i8q->metric ||
      full->device != i8q->device || k == 0 || k > r) {
    ph_set_error("%s: needs the f32 store of the same n / dim / metric / device and 1 <= k <= r", call);
    return PHNSW_E_INVALID;
  }
  return 0;
}
static int i8q_scan_device_check(const char *call, const float *queries_dev, uint32_t ldq, uint32_t ld_min, bool aligned,
                                 const void *ids, const void *d, const void *len) {
  if (!queries_dev || !ids || !d || !len || ldq < ld_min || (aligned && ((ldq % 4) || ((uintptr_t)queries_dev % 16)))) {
    ph_set_error("%s: invalid argument (queries and outputs not NULL; ldq >= %u%s)", call, ld_min,
                 aligned ? ", a multiple of 4, 16-byte base" : "");
    return PHNSW_E_INVALID;
  }
  return 0;
}

// the host forms: queries checked and up as rows of `ld` floats (zero padded), the device form on the null stream, the
// leading `k` of each row of r down as u64 ids (ph_take_launch)
static int i8q_scan_host(const char *call, const phnsw_store *i8q, const phnsw_store *full, const float *queries, uint64_t nq,
                         uint32_t r, uint32_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len) {
  if (!queries || !out_ids || !out_d || !out_len) {
    ph_set_error("%s: queries and outputs must not be NULL", call);
    return PHNSW_E_INVALID;
  }
  for (uint64_t i = 0; i < nq * i8q->dim; i++)
    if (!std::isfinite(queries[i])) {
      ph_set_error("%s: query %llu has a NaN or infinite component", call, (unsigned long long)(i / i8q->dim));
      return PHNSW_E_INVALID;
    }
  PH_HIP(hipSetDevice(i8q->device));
  const uint32_t ld = i8q->ld;
  float *qd = nullptr, *od = nullptr, *dk = nullptr;
  uint32_t *oid = nullptr, *olen = nullptr;
  uint64_t *ids64 = nullptr;
  int rc = 0;
  hipError_t e = hipMalloc(&qd, (size_t)nq * ld * 4);
  if (e == hipSuccess && ld != i8q->dim) e = hipMemset(qd, 0, (size_t)nq * ld * 4);
  if (e == hipSuccess)
    e = hipMemcpy2D(qd, (size_t)ld * 4, queries, (size_t)i8q->dim * 4, (size_t)i8q->dim * 4, nq, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&oid, (size_t)nq * r * 4);
  if (e == hipSuccess) e = hipMalloc(&od, (size_t)nq * r * 4);
  if (e == hipSuccess) e = hipMalloc(&olen, nq * 4);
  if (e == hipSuccess) e = hipMalloc(&ids64, (size_t)nq * k * 8);
  if (e == hipSuccess) e = hipMalloc(&dk, (size_t)nq * k * 4);
  if (e != hipSuccess) rc = ph_hip_fail(e, "i8q scan staging", __FILE__, __LINE__);
  if (!rc) rc = i8q_scan_enqueue(i8q, qd, ld, nq, r, oid, od, olen, 0);
  if (!rc && full) rc = ph_rerank_launch(full, qd, ld, nq, r, k, olen, oid, od, 0);
  if (!rc) rc = ph_take_launch(oid, od, r, k, nq, ids64, dk, 0);
  if (!rc) {
    std::vector<uint32_t> h_len(nq);
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h_len.data(), olen, nq * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_ids, ids64, (size_t)nq * k * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_d, dk, (size_t)nq * k * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = ph_hip_fail(e, "i8q scan", __FILE__, __LINE__);
    for (uint64_t i = 0; !rc && i < nq; i++) out_len[i] = std::min<uint64_t>(h_len[i], k);
  }
  for (void *p : {(void *)qd, (void *)od, (void *)dk, (void *)oid, (void *)olen, (void *)ids64})
    if (p) hipFree(p);
  return rc;
}

extern "C" int phnsw_i8q_scan_topk_device(const phnsw_store *i8q, const float *queries_dev, uint32_t ldq, uint64_t nq,
                                          uint64_t r, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                          void *stream) try {
  const char *const call = "phnsw_i8q_scan_topk_device";
  PH_TRY(i8q_scan_check(call, i8q, nq, r));
  if (nq == 0) return 0;
  PH_TRY(i8q_scan_device_check(call, queries_dev, ldq, i8q->dim, false, out_ids_dev, out_d_dev, out_len_dev));
  return i8q_scan_enqueue(i8q, queries_dev, ldq, nq, (uint32_t)r, out_ids_dev, out_d_dev, out_len_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_i8q_scan_topk(const phnsw_store *i8q, const float *queries, uint64_t nq, uint64_t r, uint64_t *out_ids,
                                   float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_i8q_scan_topk";
  PH_TRY(i8q_scan_check(call, i8q, nq, r));
  if (nq == 0) return 0;
  return i8q_scan_host(call, i8q, nullptr, queries, nq, (uint32_t)r, (uint32_t)r, out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_i8q_scan_search_device(const phnsw_store *i8q, const phnsw_store *full, const float *queries_dev,
                                            uint32_t ldq, uint64_t nq, uint64_t r, uint64_t k, uint32_t *out_ids_dev,
                                            float *out_d_dev, uint32_t *out_len_dev, void *stream) try {
  const char *const call = "phnsw_i8q_scan_search_device";
  PH_TRY(i8q_scan_search_check(call, i8q, full, nq, r, k));
  if (nq == 0) return 0;
  PH_TRY(i8q_scan_device_check(call, queries_dev, ldq, full->ld, true, out_ids_dev, out_d_dev, out_len_dev));
  PH_TRY(i8q_scan_enqueue(i8q, queries_dev, ldq, nq, (uint32_t)r, out_ids_dev, out_d_dev, out_len_dev, (hipStream_t)stream));
  return ph_rerank_launch(full, queries_dev, ldq, nq, (uint32_t)r, (uint32_t)k, out_len_dev, out_ids_dev, out_d_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_i8q_scan_search(const phnsw_store *i8q, const phnsw_store *full, const float *queries, uint64_t nq,
                                     uint64_t r, uint64_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_i8q_scan_search";
  PH_TRY(i8q_scan_search_check(call, i8q, full, nq, r, k));
  if (nq == 0) return 0;
  return i8q_scan_host(call, i8q, full, queries, nq, (uint32_t)r, (uint32_t)k, out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }
