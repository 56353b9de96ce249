// The exhaustive MXFP4 scan over an fp4 store (PH_ROWS_FP4, rowstore.hip) on the block-scaled matrix cores:
// phnsw_fp4_scan_topk[_device], the r rows nearest each query by the score s = sum q^_j x^_j of the MXFP4-quantised query
// and the stored row, and phnsw_fp4_scan_search[_device], that scan followed by the f32 re-rank of pq.hip.  No index, no
// filter, no exclude: every row 0 .. n - 1 is a candidate.  Dot-product metrics only.  The scan kernel's body is
// scan_fp4_kernel.h's, instantiated here in its PLAIN form; the forms over an allow-list and their entry points are
// scan_fp4_filtered.hip's, which run through this file's launcher, scratch, merge kernel and host staging.
//
//   result of a query = the min(r, n) rows with the smallest (finalize_metric(s), id), ascending.
//   s                 = the chain of v_mfma_scale_f32_16x16x128_f8f6f4 over ascending k, f32 accumulation from 0.
//
// How the work is mapped (fp4_scan_plan.h has the rules):
//   * ph_fp4_scan_query_kernel quantises the queries by the store's own rule (ph_fp4_e8 / ph_fp4_quant) into operand
//     order: 16 code bytes per block, the scale bytes arranged so that a lane's scales of four steps are one dword;
//   * a workgroup of one wave64 takes a TILE of G = 1, 2 or 4 query groups (16 queries each, the N side) and a SLICE
//     of the row groups (16 rows each, the M side).  The tile's codes stay in REGISTERS for the whole slice: 4 VGPRs a
//     step and group, and the scale dwords whose byte the instruction's op_sel picks;
//   * a row group is read STRAIGHT FROM THE STORE: lane l takes the 16 code bytes of block 4 s + l / 16 of row l % 16,
//     one aligned dwordx4 a step, and two scale dwords a section (even and odd steps; the byte is again an op_sel).
//     The next group's loads are issued before the current group's MFMAs.  Rows at or past n read row n - 1 and are
//     never candidates; blocks at or past the row's last are zero codes and are not read;
//   * the four accumulators of a lane belong to ONE query (column l % 16) and rows 4 (l / 16) + i.  They are compared
//     RAW against the query's threshold smin, one register per group: one ballot per row group, and most end there;
//   * survivors become keys mkkey(finalize_metric(s), id), STAGED per query in LDS (slot by an LDS atomic); a stage
//     that could not take another 16 is flushed through PhExactTopK::insert, whose lists live in scratch (64 queries
//     of r = 1024 do not fit the LDS) and whose 64 sorted survivors live in LDS.  smin is then taken again from the
//     r-th key (ph_fp4_scan_smin: conservative, insert tests every key again, so no threshold changes a result);
//   * with more than one slice the lists go to [queries][slices][r] and ph_fp4_scan_merge_kernel feeds them through
//     the same running top-r (PH_EXACT_FEED).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "scan_fp4_kernel.h"

// one lane per block of 32 components: the block's scale by ph_fp4_e8, its codes by ph_fp4_quant, component j in nibble
// j & 1 of byte j / 2 as in the store.  Components at or past dim count as 0; a block of zeros has e8 = 2 and zero codes.
__global__ __launch_bounds__(256) void ph_fp4_scan_query_kernel(const float *__restrict__ queries, uint32_t ldq, uint32_t dim,
                                                                uint32_t nq, uint32_t steps, uint8_t *__restrict__ codes,
                                                                uint8_t *__restrict__ scales) {
  const uint32_t nblk = 4u * steps;
  const uint64_t total = (uint64_t)nq * nblk;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t q = x / nblk;
    const uint32_t b = (uint32_t)(x - q * nblk);
    const float *src = queries + q * ldq;
    uint32_t xb[32], mb = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 32u; j++) {
      const uint32_t c = 32u * b + j;
      xb[j] = c < dim ? __float_as_uint(src[c]) : 0u;
      mb = max(mb, xb[j] & 0x7FFFFFFFu);
    }
    const uint32_t e8 = ph_fp4_e8(mb);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < 32u; j++) w[j >> 3] |= ph_fp4_quant(xb[j], e8) << (4u * (j & 7u));
    *(uint4 *)(codes + (q * nblk + b) * 16u) = make_uint4(w[0], w[1], w[2], w[3]);
    scales[q * ph_fp4_scan_scale_bytes(steps) + (b & 3u) * ph_fp4_scan_scale_run(steps) + (b >> 2)] = (uint8_t)e8;
  }
}

template <int S, int G>
__global__ __launch_bounds__(64) void ph_fp4_scan_kernel(PhFp4ScanArgs a) {
  ph_fp4_scan_body<S, G, PH_FP4_SCAN_PLAIN>(a);
}

// One wave per query: the slices' ascending lists merged through the same running top-r.
__global__ __launch_bounds__(64) void ph_fp4_scan_merge_kernel(PhFp4ScanArgs a) {
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

static PhFp4ScanFn scan_fn(int cls, uint32_t T) {
  switch (cls * 100 + (int)T) {
    case 216: return ph_fp4_scan_kernel<2, 1>;
    case 232: return ph_fp4_scan_kernel<2, 2>;
    case 264: return ph_fp4_scan_kernel<2, 4>;
    case 616: return ph_fp4_scan_kernel<6, 1>;
    case 632: return ph_fp4_scan_kernel<6, 2>;
    case 664: return ph_fp4_scan_kernel<6, 4>;
    case 1216: return ph_fp4_scan_kernel<12, 1>;
    case 1232: return ph_fp4_scan_kernel<12, 2>;
    default: return nullptr;
  }
}

// The scratch of a scan: the prepared queries, a status word per query (ph_exact_write_row's; always ST_OK here) and
// the lists.  An fp4 store has no index to keep it with, so the translation unit keeps it PER DEVICE, as scan_bits.hip
// does: two blocks a device, used alternately so that scans on two streams may overlap; `done` closes the last launch
// that used a block and the next user's stream waits for it.  g_mutex is held while a call enqueues its launches.
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
// bitmaps filter_stride words apart (the MASK form), scan_fp4_filtered.hip
int ph_fp4_scan_enqueue(const phnsw_store *s, const float *queries_dev, uint32_t ldq, uint64_t nq, uint32_t r,
                        const uint32_t *filter_dev, uint32_t filter_stride, uint32_t *out_ids, float *out_d, uint32_t *out_len,
                        hipStream_t stream) {
  if (nq == 0) return 0;
  PH_HIP(hipSetDevice(s->device));
  const uint32_t steps = ph_fp4_scan_steps(s->ld);
  const int cls = ph_fp4_scan_class(steps);
  if (!cls) return ph_dim_unsupported(s->dim);
  const uint32_t T = ph_fp4_scan_tile(cls, env_ll("PHNSW_FP4_SCAN_TILE"));  // tests and tuning: neither changes a result
  const int form = !filter_dev ? PH_FP4_SCAN_PLAIN : (filter_stride ? PH_FP4_SCAN_MASK : PH_FP4_SCAN_LIST);
  const PhFp4ScanFn fn = form == PH_FP4_SCAN_PLAIN ? scan_fn(cls, T) : ph_fp4_scan_filtered_fn(cls, T, form);
  if (!fn) return ph_dim_unsupported(s->dim);
  const size_t lds = ph_fp4_scan_lds(r, T), merge_lds = ph_fp4_scan_merge_lds(r);
  uint64_t resident = 0;  // workgroups of the scan the device holds at once
  PhResidentMemo *memo;
  {
    std::lock_guard<std::mutex> g(g_resident_mutex);
    memo = &g_resident[s->device];
  }
  PH_TRY(ph_resident_waves(*memo, g_resident_mutex, s->device, (const void *)fn, lds, &resident));
  const uint64_t groups = ph_fp4_scan_groups(s->n);
  const uint64_t first = std::min<uint64_t>(nq, PH_FP4_SCAN_CHUNK_MAX);
  const uint32_t slices = ph_fp4_scan_slices(ph_fp4_scan_tiles(first, T), resident, groups, env_ll("PHNSW_FP4_SCAN_SLICES"), r, T);
  const uint64_t chunk = std::min<uint64_t>(nq, ph_fp4_scan_chunk(slices, r, T));
  const uint64_t chunk_tiles = ph_fp4_scan_tiles(chunk, T);
  const size_t codes_bytes = up256((size_t)chunk * ph_fp4_scan_code_bytes(steps));
  const size_t scales_bytes = up256((size_t)chunk * ph_fp4_scan_scale_bytes(steps)), status_bytes = up256((size_t)chunk * 4u);
  const size_t lists_bytes = up256((size_t)chunk_tiles * T * slices * 2u * r * 8u);
  const size_t merge_bytes = slices > 1u ? up256((size_t)chunk * slices * r * 8u) : 0u;  // together: ph_fp4_scan_scratch_bytes
  // LIST: the compaction's words behind everything else.  The slices were cut from all ceil(n / 16) groups, the kernel
  // cuts the list's own; what is left over is empty slices
  const size_t pre_bytes = form == PH_FP4_SCAN_LIST ? up256(ph_fp4_scan_pre_bytes(s->n)) : 0u;
  const size_t bytes = codes_bytes + scales_bytes + status_bytes + lists_bytes + merge_bytes + pre_bytes;

  std::lock_guard<std::mutex> g(g_mutex);
  ScanScratch *x = nullptr;
  PH_TRY(scratch_acquire(s->device, bytes, stream, &x));
  char *at_mem = (char *)x->mem;
  PhFp4ScanArgs a = {};
  a.rows = (const uint8_t *)s->packed, a.stride = s->packed_stride, a.nb = ph_fp4_scan_blocks(s->ld), a.steps = steps;
  a.n = (uint32_t)s->n, a.k = r, a.metric = s->metric, a.slices = slices, a.stage = ph_fp4_scan_stage(r), a.groups = groups;
  a.qcodes = (const uint8_t *)at_mem, at_mem += codes_bytes;
  a.qscales = (const uint8_t *)at_mem, at_mem += scales_bytes;
  a.status = (uint32_t *)at_mem, at_mem += status_bytes;
  a.lists = (uint64_t *)at_mem, at_mem += lists_bytes;
  a.scratch = (uint64_t *)at_mem, at_mem += merge_bytes;
  if (form == PH_FP4_SCAN_LIST) {  // once for all chunks
    uint32_t *const pre = (uint32_t *)at_mem;
    PH_TRY(ph_fp4_scan_list_enqueue(filter_dev, s->n, pre, stream));
    a.count = pre, a.cand = pre + ph_fp4_scan_pre_list(s->n);
  }
  a.filter_stride = filter_stride;
  for (uint64_t at = 0; at < nq; at += chunk) {
    const uint64_t cnt = std::min(chunk, nq - at);
    a.nq = (uint32_t)cnt, a.tiles = (uint32_t)ph_fp4_scan_tiles(cnt, T);
    if (form == PH_FP4_SCAN_MASK) a.filter = filter_dev + at * filter_stride;
    a.out_ids = out_ids + at * r, a.out_d = out_d + at * r, a.out_len = out_len + at;
    hipLaunchKernelGGL(ph_fp4_scan_query_kernel, dim3((uint32_t)std::min<uint64_t>((cnt * 4u * steps + 255u) / 256u, 1u << 16)), dim3(256),
                       0, stream, queries_dev + at * ldq, ldq, s->dim, (uint32_t)cnt, steps, (uint8_t *)a.qcodes, (uint8_t *)a.qscales);
    hipLaunchKernelGGL(fn, dim3(a.tiles * slices), dim3(64), lds, stream, a);
    if (slices > 1u)
      hipLaunchKernelGGL(ph_fp4_scan_merge_kernel, dim3((uint32_t)std::min<uint64_t>(cnt, 1u << 20)), dim3(64), merge_lds, stream, a);
    PH_HIP(hipGetLastError());
  }
  PH_HIP(hipEventRecord(x->done, stream));
  return 0;
}

// ------------------------------------------------------------------ entry points

// what all four calls ask of the store and of r
int ph_fp4_scan_check(const char *call, const phnsw_store *fp4, uint64_t nq, uint64_t r) {
  if (!fp4 || fp4->kind != PH_ROWS_FP4) {
    ph_set_error("%s: needs an fp4 store (phnsw_store_create_fp4), not %s", call, fp4 ? ph_rows_name(fp4->kind) : "NULL");
    return PHNSW_E_UNSUPPORTED;
  }
  if (fp4->metric == PHNSW_METRIC_L2) {
    ph_set_error("%s: dot-product metrics only (an L2 store has no block-scaled form)", call);
    return PHNSW_E_UNSUPPORTED;
  }
  if (!ph_fp4_scan_r_valid(r) || nq > 0xFFFFFFFFull || fp4->n > 0x7FFFFFFFull) {
    ph_set_error("%s: needs 1 <= r <= %u, at most 2^32 - 1 queries and at most 2^31 - 1 rows", call, PH_FP4_SCAN_RMAX);
    return PHNSW_E_INVALID;
  }
  return 0;
}
// ... and the searches of `full` and k: what rerank_check (pq.hip) demands of a converted store
int ph_fp4_scan_search_check(const char *call, const phnsw_store *fp4, const phnsw_store *full, uint64_t nq, uint64_t r, uint64_t k) {
  PH_TRY(ph_fp4_scan_check(call, fp4, nq, r));
  if (!full || !ph_store_f32(full) || full->n != fp4->n || full->dim != fp4->dim || full->metric != fp4->metric ||
      full->device != fp4->device || k == 0 || k > r) {
    ph_set_error("%s: needs the f32 store of the same n / dim / metric / device and 1 <= k <= r", call);
    return PHNSW_E_INVALID;
  }
  return 0;
}
int ph_fp4_scan_device_check(const char *call, const float *queries_dev, uint32_t ldq, uint32_t ld_min, bool aligned,
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
int ph_fp4_scan_host(const char *call, const phnsw_store *fp4, const phnsw_store *full, const float *queries, uint64_t nq,
                     uint32_t r, uint32_t k, const uint32_t *filter, uint32_t filter_stride, uint64_t *out_ids, float *out_d,
                     uint64_t *out_len) {
  if (!queries || !out_ids || !out_d || !out_len) {
    ph_set_error("%s: queries and outputs must not be NULL", call);
    return PHNSW_E_INVALID;
  }
  for (uint64_t i = 0; i < nq * fp4->dim; i++)
    if (!std::isfinite(queries[i])) {
      ph_set_error("%s: query %llu has a NaN or infinite component", call, (unsigned long long)(i / fp4->dim));
      return PHNSW_E_INVALID;
    }
  PH_HIP(hipSetDevice(fp4->device));
  const uint32_t ld = fp4->ld;
  float *qd = nullptr, *od = nullptr, *dk = nullptr;
  uint32_t *oid = nullptr, *olen = nullptr, *fd = nullptr;
  uint64_t *ids64 = nullptr;
  int rc = 0;
  // the filter's words as the device form reads them: one bitmap, or nq whole strides
  const size_t filter_bytes = filter ? (filter_stride ? (size_t)nq * filter_stride : (size_t)ph_exact_words(fp4->n)) * 4u : 0u;
  hipError_t e = hipMalloc(&qd, (size_t)nq * ld * 4);
  if (e == hipSuccess && ld != fp4->dim) e = hipMemset(qd, 0, (size_t)nq * ld * 4);
  if (e == hipSuccess)
    e = hipMemcpy2D(qd, (size_t)ld * 4, queries, (size_t)fp4->dim * 4, (size_t)fp4->dim * 4, nq, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&oid, (size_t)nq * r * 4);
  if (e == hipSuccess) e = hipMalloc(&od, (size_t)nq * r * 4);
  if (e == hipSuccess) e = hipMalloc(&olen, nq * 4);
  if (e == hipSuccess) e = hipMalloc(&ids64, (size_t)nq * k * 8);
  if (e == hipSuccess) e = hipMalloc(&dk, (size_t)nq * k * 4);
  if (e == hipSuccess && filter_bytes) e = hipMalloc(&fd, filter_bytes);
  if (e == hipSuccess && filter_bytes) e = hipMemcpy(fd, filter, filter_bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) rc = ph_hip_fail(e, "fp4 scan staging", __FILE__, __LINE__);
  if (!rc) rc = ph_fp4_scan_enqueue(fp4, qd, ld, nq, r, fd, filter_stride, oid, od, olen, 0);
  if (!rc && full) rc = ph_rerank_launch(full, qd, ld, nq, r, k, olen, oid, od, 0);
  if (!rc) rc = ph_take_launch(oid, od, r, k, nq, ids64, dk, 0);
  if (!rc) {
    std::vector<uint32_t> h_len(nq);
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h_len.data(), olen, nq * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_ids, ids64, (size_t)nq * k * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_d, dk, (size_t)nq * k * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = ph_hip_fail(e, "fp4 scan", __FILE__, __LINE__);
    for (uint64_t i = 0; !rc && i < nq; i++) out_len[i] = std::min<uint64_t>(h_len[i], k);
  }
  for (void *p : {(void *)qd, (void *)od, (void *)dk, (void *)oid, (void *)olen, (void *)ids64, (void *)fd})
    if (p) hipFree(p);
  return rc;
}

extern "C" int phnsw_fp4_scan_topk_device(const phnsw_store *fp4, const float *queries_dev, uint32_t ldq, uint64_t nq,
                                          uint64_t r, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                          void *stream) try {
  const char *const call = "phnsw_fp4_scan_topk_device";
  PH_TRY(ph_fp4_scan_check(call, fp4, nq, r));
  if (nq == 0) return 0;
  PH_TRY(ph_fp4_scan_device_check(call, queries_dev, ldq, fp4->dim, false, out_ids_dev, out_d_dev, out_len_dev));
  return ph_fp4_scan_enqueue(fp4, queries_dev, ldq, nq, (uint32_t)r, nullptr, 0u, out_ids_dev, out_d_dev, out_len_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_fp4_scan_topk(const phnsw_store *fp4, const float *queries, uint64_t nq, uint64_t r, uint64_t *out_ids,
                                   float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_fp4_scan_topk";
  PH_TRY(ph_fp4_scan_check(call, fp4, nq, r));
  if (nq == 0) return 0;
  return ph_fp4_scan_host(call, fp4, nullptr, queries, nq, (uint32_t)r, (uint32_t)r, nullptr, 0u, out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_fp4_scan_search_device(const phnsw_store *fp4, const phnsw_store *full, const float *queries_dev,
                                            uint32_t ldq, uint64_t nq, uint64_t r, uint64_t k, uint32_t *out_ids_dev,
                                            float *out_d_dev, uint32_t *out_len_dev, void *stream) try {
  const char *const call = "phnsw_fp4_scan_search_device";
  PH_TRY(ph_fp4_scan_search_check(call, fp4, full, nq, r, k));
  if (nq == 0) return 0;
  PH_TRY(ph_fp4_scan_device_check(call, queries_dev, ldq, full->ld, true, out_ids_dev, out_d_dev, out_len_dev));
  PH_TRY(ph_fp4_scan_enqueue(fp4, queries_dev, ldq, nq, (uint32_t)r, nullptr, 0u, out_ids_dev, out_d_dev, out_len_dev, (hipStream_t)stream));
  return ph_rerank_launch(full, queries_dev, ldq, nq, (uint32_t)r, (uint32_t)k, out_len_dev, out_ids_dev, out_d_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_fp4_scan_search(const phnsw_store *fp4, const phnsw_store *full, const float *queries, uint64_t nq,
                                     uint64_t r, uint64_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_fp4_scan_search";
  PH_TRY(ph_fp4_scan_search_check(call, fp4, full, nq, r, k));
  if (nq == 0) return 0;
  return ph_fp4_scan_host(call, fp4, full, queries, nq, (uint32_t)r, (uint32_t)k, nullptr, 0u, out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }
