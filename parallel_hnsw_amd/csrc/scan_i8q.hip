// The exhaustive int8 scan over an i8q store (PH_ROWS_I8Q, rowstore.hip) on the matrix cores:
// phnsw_i8q_scan_topk[_device], the r rows nearest each query by the store's own distance, and
// phnsw_i8q_scan_search[_device], that scan followed by the f32 re-rank of pq.hip.  No index, no filter, no exclude:
// every row 0 .. n - 1 is a candidate.  An i8q store is never L2.  The scan kernel's body is scan_i8q_kernel.h's,
// instantiated here in its PLAIN form; the forms over an allow-list and their entry points are scan_i8q_filtered.hip's,
// which run through this file's launcher, scratch, merge kernel and host staging.
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

#include "scan_i8q_kernel.h"

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

template <int S, int RG>
__global__ __launch_bounds__(256) void ph_i8q_scan_kernel(PhI8qScanArgs a) {
  ph_i8q_scan_body<S, RG, PH_I8Q_SCAN_PLAIN>(a);
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

// the scan of nq device queries on `stream` (arguments checked by the caller): rows [nq][r] u32 ids and distances, len.
// filter_dev: nullptr = every row (the plain form); one bitmap (filter_stride 0: compacted here, the LIST form) or nq
// bitmaps filter_stride words apart (the MASK form), scan_i8q_filtered.hip
int ph_i8q_scan_enqueue(const phnsw_store *s, const float *queries_dev, uint32_t ldq, uint64_t nq, uint32_t r,
                        const uint32_t *filter_dev, uint32_t filter_stride, uint32_t *out_ids, float *out_d, uint32_t *out_len,
                        hipStream_t stream) {
  if (nq == 0) return 0;
  PH_HIP(hipSetDevice(s->device));
  const uint32_t steps = ph_i8q_scan_steps(s->ld), runs = ph_i8q_scan_runs(s->ld);
  const int cls = s->ld <= PH_I8Q_SCAN_LD_MAX ? ph_i8q_scan_class(steps) : 0;
  const int form = !filter_dev ? PH_I8Q_SCAN_PLAIN : (filter_stride ? PH_I8Q_SCAN_MASK : PH_I8Q_SCAN_LIST);
  const PhI8qScanFn fn = form == PH_I8Q_SCAN_PLAIN ? scan_fn(cls) : ph_i8q_scan_filtered_fn(cls, form);
  if (!fn || s->packed_stride < 16u * runs || s->packed_stride % 16u) return ph_dim_unsupported(s->dim);
  const uint32_t tg = ph_i8q_scan_tile(cls, env_ll("PHNSW_I8Q_SCAN_TILE"));  // tests and tuning: neither changes a result
  const size_t lds = form == PH_I8Q_SCAN_LIST ? ph_i8q_scan_list_lds(r, steps, tg) : ph_i8q_scan_lds(r, steps, tg);
  const size_t merge_lds = ph_i8q_scan_merge_lds(r);
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
  // LIST: the compaction's words behind everything else.  The slices were cut from all the row tiles of n, the kernel
  // cuts the list's own; what is left over is empty slices
  const size_t pre_bytes = form == PH_I8Q_SCAN_LIST ? up256(ph_fp4_scan_pre_bytes(s->n)) : 0u;
  const size_t bytes = img_bytes + scale_bytes + status_bytes + lists_bytes + merge_bytes + pre_bytes;

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
  if (form == PH_I8Q_SCAN_LIST) {  // once for all chunks
    uint32_t *const pre = (uint32_t *)at_mem;
    PH_TRY(ph_fp4_scan_list_enqueue(filter_dev, s->n, pre, stream));
    a.count = pre, a.cand = pre + ph_fp4_scan_pre_list(s->n);
  }
  a.filter_stride = filter_stride;
  for (uint64_t at = 0; at < nq; at += chunk) {
    const uint64_t cnt = std::min(chunk, nq - at);
    a.nq = (uint32_t)cnt, a.qtiles = (uint32_t)ph_i8q_scan_qtiles(cnt);
    if (form == PH_I8Q_SCAN_MASK) a.filter = filter_dev + at * filter_stride;
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
int ph_i8q_scan_check(const char *call, const phnsw_store *i8q, uint64_t nq, uint64_t r) {
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
int ph_i8q_scan_search_check(const char *call, const phnsw_store *i8q, const phnsw_store *full, uint64_t nq, uint64_t r, uint64_t k) {
  PH_TRY(ph_i8q_scan_check(call, i8q, nq, r));
  if (!full || !ph_store_f32(full) || full->n != i8q->n || full->dim != i8q->dim || full->metric != i8q->metric ||
      full->device != i8q->device || k == 0 || k > r) {
    ph_set_error("%s: needs the f32 store of the same n / dim / metric / device and 1 <= k <= r", call);
    return PHNSW_E_INVALID;
  }
  return 0;
}
int ph_i8q_scan_device_check(const char *call, const float *queries_dev, uint32_t ldq, uint32_t ld_min, bool aligned,
                             const void *ids, const void *d, const void *len) {
  if (!queries_dev || !ids || !d || !len || ldq < ld_min || (aligned && ((ldq % 4) || ((uintptr_t)queries_dev % 16)))) {
    ph_set_error("%s: invalid argument (queries and outputs not NULL; ldq >= %u%s)", call, ld_min,
                 aligned ? ", a multiple of 4, 16-byte base" : "");
    return PHNSW_E_INVALID;
  }
  return 0;
}

// the host forms: queries checked and up as rows of `ld` floats (zero padded), the device form on the null stream, the
// leading `k` of each row of r down as u64 ids (ph_take_launch).  filter: nullptr, or the host words of the filtered forms
int ph_i8q_scan_host(const char *call, const phnsw_store *i8q, const phnsw_store *full, const float *queries, uint64_t nq,
                     uint32_t r, uint32_t k, const uint32_t *filter, uint32_t filter_stride, uint64_t *out_ids, float *out_d,
                     uint64_t *out_len) {
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
  uint32_t *oid = nullptr, *olen = nullptr, *fd = nullptr;
  uint64_t *ids64 = nullptr;
  int rc = 0;
  // the filter's words as the device form reads them: one bitmap, or nq whole strides
  const size_t filter_bytes = filter ? (filter_stride ? (size_t)nq * filter_stride : (size_t)ph_exact_words(i8q->n)) * 4u : 0u;
  hipError_t e = hipMalloc(&qd, (size_t)nq * ld * 4);
  if (e == hipSuccess && ld != i8q->dim) e = hipMemset(qd, 0, (size_t)nq * ld * 4);
  if (e == hipSuccess)
    e = hipMemcpy2D(qd, (size_t)ld * 4, queries, (size_t)i8q->dim * 4, (size_t)i8q->dim * 4, nq, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&oid, (size_t)nq * r * 4);
  if (e == hipSuccess) e = hipMalloc(&od, (size_t)nq * r * 4);
  if (e == hipSuccess) e = hipMalloc(&olen, nq * 4);
  if (e == hipSuccess) e = hipMalloc(&ids64, (size_t)nq * k * 8);
  if (e == hipSuccess) e = hipMalloc(&dk, (size_t)nq * k * 4);
  if (e == hipSuccess && filter_bytes) e = hipMalloc(&fd, filter_bytes);
  if (e == hipSuccess && filter_bytes) e = hipMemcpy(fd, filter, filter_bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) rc = ph_hip_fail(e, "i8q scan staging", __FILE__, __LINE__);
  if (!rc) rc = ph_i8q_scan_enqueue(i8q, qd, ld, nq, r, fd, filter_stride, oid, od, olen, 0);
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
  for (void *p : {(void *)qd, (void *)od, (void *)dk, (void *)oid, (void *)olen, (void *)ids64, (void *)fd})
    if (p) hipFree(p);
  return rc;
}

extern "C" int phnsw_i8q_scan_topk_device(const phnsw_store *i8q, const float *queries_dev, uint32_t ldq, uint64_t nq,
                                          uint64_t r, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                          void *stream) try {
  const char *const call = "phnsw_i8q_scan_topk_device";
  PH_TRY(ph_i8q_scan_check(call, i8q, nq, r));
  if (nq == 0) return 0;
  PH_TRY(ph_i8q_scan_device_check(call, queries_dev, ldq, i8q->dim, false, out_ids_dev, out_d_dev, out_len_dev));
  return ph_i8q_scan_enqueue(i8q, queries_dev, ldq, nq, (uint32_t)r, nullptr, 0u, out_ids_dev, out_d_dev, out_len_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_i8q_scan_topk(const phnsw_store *i8q, const float *queries, uint64_t nq, uint64_t r, uint64_t *out_ids,
                                   float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_i8q_scan_topk";
  PH_TRY(ph_i8q_scan_check(call, i8q, nq, r));
  if (nq == 0) return 0;
  return ph_i8q_scan_host(call, i8q, nullptr, queries, nq, (uint32_t)r, (uint32_t)r, nullptr, 0u, out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_i8q_scan_search_device(const phnsw_store *i8q, const phnsw_store *full, const float *queries_dev,
                                            uint32_t ldq, uint64_t nq, uint64_t r, uint64_t k, uint32_t *out_ids_dev,
                                            float *out_d_dev, uint32_t *out_len_dev, void *stream) try {
  const char *const call = "phnsw_i8q_scan_search_device";
  PH_TRY(ph_i8q_scan_search_check(call, i8q, full, nq, r, k));
  if (nq == 0) return 0;
  PH_TRY(ph_i8q_scan_device_check(call, queries_dev, ldq, full->ld, true, out_ids_dev, out_d_dev, out_len_dev));
  PH_TRY(ph_i8q_scan_enqueue(i8q, queries_dev, ldq, nq, (uint32_t)r, nullptr, 0u, out_ids_dev, out_d_dev, out_len_dev, (hipStream_t)stream));
  return ph_rerank_launch(full, queries_dev, ldq, nq, (uint32_t)r, (uint32_t)k, out_len_dev, out_ids_dev, out_d_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_i8q_scan_search(const phnsw_store *i8q, const phnsw_store *full, const float *queries, uint64_t nq,
                                     uint64_t r, uint64_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_i8q_scan_search";
  PH_TRY(ph_i8q_scan_search_check(call, i8q, full, nq, r, k));
  if (nq == 0) return 0;
  return ph_i8q_scan_host(call, i8q, full, queries, nq, (uint32_t)r, (uint32_t)k, nullptr, 0u, out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }
