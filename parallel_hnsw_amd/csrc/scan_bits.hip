// The exhaustive Hamming scan over a bits store (PH_ROWS_BITS, rowstore.hip): phnsw_bits_scan_topk[_device], the r rows
// nearest each query by h = popcount(row XOR query), and phnsw_bits_scan_search[_device], that scan followed by the f32
// re-rank of pq.hip.  No index, no filter, no exclude: every row 0 .. n - 1 is a candidate.
//
//   result of a query = the min(r, n) rows with the smallest (h, id), ascending; distance = ph_bits_distance(h): the
//                       bits of phnsw_distance_batch on the store.  Every metric's map is strictly increasing in h, so
//                       (distance, id) order and (h, id) order are one order.
//
// How the work is mapped (bits_scan_plan.h has the integer rules):
//   * a workgroup of one wave64 takes a TILE of T queries and a SLICE of the rows, 64 rows (a batch) at a time, ONE ROW
//     PER LANE in registers: 2 NV dwordx4 loads a lane, the next batch's issued before the current one is used;
//   * the tile's queries are WAVE-UNIFORM: their sign words, reduced once per launch into a packed buffer
//     (ph_bits_query_kernel, the store's own reduction), come in by scalar loads, and a (query, batch) costs 8 NV XOR and
//     8 NV accumulating popcounts -- no LDS in that loop;
//   * a row is tested as an INTEGER first: against hmax, the h of the query's current r-th key (dim + 1 while the list
//     is short).  Ids ascend inside a slice, so a row enters a full list only if h < hmax, strictly; one compare and one
//     ballot, and most (query, batch) pairs end there;
//   * survivors become keys mkkey(ph_bits_distance(h), id) and are STAGED, 64 per query, appended in lane order by
//     ballot prefix; a full stage is flushed through PhExactTopK::insert (exact_topk.h) and hmax is read again.  A stale
//     hmax only lets more keys reach insert, which tests them again: the staging cannot change a result;
//   * with more than one slice the lists go to a scratch [queries][slices][r] and ph_bits_scan_merge_kernel feeds them
//     through the same running top-r (PH_EXACT_FEED).
// One work item per workgroup: every global store of the scan kernel comes after its last load.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "bits_scan_plan.h"
#include "exact_topk.h"
#include "phnsw_device.h"

#define PH_TRY(x)          \
  do {                     \
    int rc__ = (x);        \
    if (rc__) return rc__; \
  } while (0)

struct PhBitsScanArgs {
  const uint4 *rows;       // n rows of 2 NV uint4
  const uint32_t *qwords;  // [nq][8 NV]: the queries' sign words in the device row layout
  uint32_t nq, n, dim, k;  // k: the r of the call (the name ph_exact_write_row reads)
  int metric;
  uint32_t T, tiles, slices;
  uint64_t batches;
  uint64_t *scratch;  // slices > 1: [nq][slices][k] keys, each list ascending, KEY_NONE padded
  uint32_t *out_ids;  // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
};

// one wave per query: [nq][ldq] f32 -> [nq][stride_words] sign words, by the rows' rule.  A NaN (bit 0) or an infinite
// component (its sign) is not refused.
__global__ __launch_bounds__(256) void ph_bits_query_kernel(const float *__restrict__ queries, uint32_t ldq, uint32_t dim,
                                                            uint32_t nq, uint32_t *__restrict__ out, uint32_t stride_words) {
  const uint32_t lane = threadIdx.x & 63u, wpb = blockDim.x / 64u;
  bool nonfinite = false;
  for (uint64_t q = (uint64_t)blockIdx.x * wpb + threadIdx.x / 64u; q < nq; q += (uint64_t)gridDim.x * wpb) {
    const uint32_t word = ph_bits_row_words(queries + q * ldq, dim, lane, nonfinite);
    if (lane < stride_words) out[q * stride_words + lane] = word;
  }
}

// The queries' sign words as the scan kernel reads them: written by an earlier launch and by nothing in this one, so
// the kernel may take them through the constant address space, where a wave-uniform address is a scalar load whatever
// barriers stand around it (through the plain pointer the compiler issued vector loads: one per word and lane).
typedef const uint32_t __attribute__((address_space(4))) *PhBitsScanWords;

// the per-query state of a tile in LDS, four words: every lane writes the same values and reads what it wrote
struct PhBitsScanState {
  uint32_t hmax, staged, len, flip;
};

// the h of a key of the list: the smallest h whose distance is not below the key's (the map is strictly increasing)
__device__ __forceinline__ uint32_t ph_bits_scan_h_of(uint64_t key, uint32_t dim, int metric) {
  const uint32_t want = (uint32_t)(key >> 32);
  uint32_t lo = 0u, hi = dim;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (fkey(ph_bits_distance(mid, dim, metric)) < want)
      lo = mid + 1u;
    else
      hi = mid;
  }
  return lo;
}

// the staged keys of one query into its running top-r; hmax afterwards.  Whole wave, uniform control flow.
__device__ __forceinline__ void ph_bits_scan_flush(uint64_t *keys, PhBitsScanState *st, uint32_t k, uint32_t dim, int metric,
                                                   uint32_t lane) {
  const uint32_t staged = rfl32(st->staged);
  uint64_t *const stage = keys + 2u * k + 64u;
  __syncthreads();  // the staged keys are other lanes' writes
  const uint64_t key = lane < staged ? stage[lane] : KEY_NONE;
  PhExactTopK top;
  top.init(keys, k);
  if (rfl32(st->flip)) top.cur = keys + k, top.nxt = keys;
  top.len = rfl32(st->len);
  top.insert(key, lane);
  __syncthreads();  // (insert returns without one when nothing survived)
  st->len = top.len;
  st->flip = top.cur == keys ? 0u : 1u;
  st->staged = 0u;
  st->hmax = top.len == k ? ph_bits_scan_h_of(top.cur[k - 1u], dim, metric) : dim + 1u;
}

template <int NV>
__global__ __launch_bounds__(64) void ph_bits_scan_kernel(PhBitsScanArgs a) {
  extern __shared__ uint64_t scan_lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t per = ph_bits_scan_query_keys(a.k);
  PhBitsScanState *const state = (PhBitsScanState *)(scan_lds + (uint64_t)a.T * per);
  const uint32_t tile = blockIdx.x % a.tiles, slice = blockIdx.x / a.tiles;
  const uint32_t q0 = tile * a.T, tq = min(a.T, a.nq - q0);
  for (uint32_t t = 0; t < tq; t++) state[t] = PhBitsScanState{a.dim + 1u, 0u, 0u, 0u};
  uint64_t b0, b1;
  ph_exact_slice_range(slice, a.slices, a.batches, &b0, &b1);

  // lane's row of batch b; past the last row the last row again (in bounds), never a candidate
  auto load = [&](uint4 (&x)[2 * NV], uint64_t b) {
    const uint32_t row = min((uint32_t)(b * 64u) + lane, a.n - 1u);
    const uint4 *src = a.rows + (uint64_t)row * (2 * NV);
#pragma unroll
    for (int i = 0; i < 2 * NV; i++) x[i] = src[i];
  };
  auto scan = [&](const uint4 (&x)[2 * NV], uint64_t b) {
    const uint32_t id = (uint32_t)(b * 64u) + lane;
    const bool valid = id < a.n;
    for (uint32_t t = 0; t < tq; t++) {
      const PhBitsScanWords qw = (PhBitsScanWords)(uintptr_t)(a.qwords + (uint64_t)(q0 + t) * (8 * NV));  // wave-uniform
      uint32_t h = 0;
#pragma unroll
      for (int i = 0; i < 2 * NV; i++) {  // one chain: every popcount adds to h in the instruction itself
        h = __popc(x[i].x ^ qw[4 * i]) + h;
        h = __popc(x[i].y ^ qw[4 * i + 1]) + h;
        h = __popc(x[i].z ^ qw[4 * i + 2]) + h;
        h = __popc(x[i].w ^ qw[4 * i + 3]) + h;
      }
      PhBitsScanState *const st = state + t;
      const bool surv = valid && h < rfl32(st->hmax);
      const uint64_t m = __ballot(surv);
      if (!m) continue;
      uint64_t *const keys = scan_lds + (uint64_t)t * per;
      const uint32_t ns = (uint32_t)__popcll(m);
      if (rfl32(st->staged) + ns > 64u) ph_bits_scan_flush(keys, st, a.k, a.dim, a.metric, lane);
      const uint32_t at = rfl32(st->staged);
      if (surv) keys[2u * a.k + 64u + at + (uint32_t)__popcll(m & lanemask_lt(lane))] = mkkey(ph_bits_distance(h, a.dim, a.metric), id);
      st->staged = at + ns;
      if (at + ns == 64u) ph_bits_scan_flush(keys, st, a.k, a.dim, a.metric, lane);
    }
  };

  if (b0 < b1) {
    uint4 xa[2 * NV], xb[2 * NV];
    load(xa, b0);
    for (uint64_t b = b0; b < b1; b += 2u) {
      if (b + 1u < b1) load(xb, b + 1u);
      scan(xa, b);
      if (b + 1u >= b1) break;
      if (b + 2u < b1) load(xa, b + 2u);
      scan(xb, b + 1u);
    }
  }
  for (uint32_t t = 0; t < tq; t++) {
    uint64_t *const keys = scan_lds + (uint64_t)t * per;
    PhBitsScanState *const st = state + t;
    if (rfl32(st->staged)) ph_bits_scan_flush(keys, st, a.k, a.dim, a.metric, lane);
    __syncthreads();
    ph_exact_write_slice<false>(a, q0 + t, q0 + t, slice, rfl32(st->flip) ? keys + a.k : keys, rfl32(st->len), false, lane);
  }
}

// One wave per query: the slices' ascending lists merged through the same running top-r.
__global__ __launch_bounds__(64) void ph_bits_scan_merge_kernel(PhBitsScanArgs a) {
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

typedef void (*PhBitsScanFn)(PhBitsScanArgs);
static PhBitsScanFn scan_fn(int nv) {
  switch (nv) {
    case 1: return ph_bits_scan_kernel<1>;
    case 3: return ph_bits_scan_kernel<3>;
    case 6: return ph_bits_scan_kernel<6>;
    default: return nullptr;
  }
}

// The scratch of a scan: the queries' sign words, a status word per query (ph_exact_write_row's; always ST_OK here) and
// the per-slice lists.  A bits store has no index to keep it with, so the translation unit keeps it PER DEVICE (a
// block and the event that closes it belong to the device they were made on): two blocks a device, used alternately so
// that scans on two streams may overlap on the device; `done` closes the last launch that used a block and the next
// user's stream waits for it.  The blocks live as long as the process (at most 64 MiB of lists and 13 MB of words each),
// and g_mutex is held while a call enqueues its launches: host threads take turns, the launches themselves overlap.
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

// a block of `device`, the current device, of at least `bytes`, behind its previous user; under g_mutex
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
}  // namespace

// the scan of nq device queries on `stream` (arguments checked by the caller): rows [nq][r] u32 ids and distances, len
static int bits_scan_device(const phnsw_store *s, const float *queries_dev, uint32_t ldq, uint64_t nq, uint32_t r,
                            uint32_t *out_ids, float *out_d, uint32_t *out_len, hipStream_t stream) {
  if (nq == 0) return 0;
  PH_HIP(hipSetDevice(s->device));
  const int nv = ph_bits_class(s->dim);
  const PhBitsScanFn fn = scan_fn(nv);
  if (!fn) return ph_dim_unsupported(s->dim);
  const uint32_t T = ph_bits_scan_tile(r, env_ll("PHNSW_BITS_SCAN_TILE"));  // tests and tuning: neither changes a result
  const size_t lds = ph_bits_scan_lds(r, T), merge_lds = ph_bits_scan_merge_lds(r);
  uint64_t resident = 0;  // workgroups of the scan the device holds at once
  PhResidentMemo *memo;
  {
    std::lock_guard<std::mutex> g(g_resident_mutex);
    memo = &g_resident[s->device];
  }
  PH_TRY(ph_resident_waves(*memo, g_resident_mutex, s->device, (const void *)fn, lds, &resident));
  const uint64_t batches = ph_bits_scan_batches(s->n);
  const uint64_t first = std::min<uint64_t>(nq, PH_BITS_SCAN_CHUNK_MAX);
  const uint32_t slices = ph_bits_scan_slices(ph_bits_scan_tiles(first, T), resident, batches, env_ll("PHNSW_BITS_SCAN_SLICES"), r, T);
  const uint64_t chunk = std::min<uint64_t>(nq, ph_bits_scan_chunk(slices, r, T));
  const uint32_t sw = ph_bits_stride_words(nv);
  const size_t words_bytes = ((size_t)chunk * sw * 4u + 255u) & ~(size_t)255u, status_bytes = ((size_t)chunk * 4u + 255u) & ~(size_t)255u;
  const size_t bytes = words_bytes + status_bytes + (size_t)ph_bits_scan_scratch_bytes(chunk, slices, r);

  std::lock_guard<std::mutex> g(g_mutex);
  ScanScratch *x = nullptr;
  PH_TRY(scratch_acquire(s->device, bytes, stream, &x));
  PhBitsScanArgs a = {};
  a.rows = (const uint4 *)s->packed, a.n = (uint32_t)s->n, a.dim = s->dim, a.k = r, a.metric = s->metric;
  a.T = T, a.slices = slices, a.batches = batches;
  a.qwords = (const uint32_t *)x->mem;
  a.status = (uint32_t *)((char *)x->mem + words_bytes);
  a.scratch = (uint64_t *)((char *)x->mem + words_bytes + status_bytes);
  for (uint64_t at = 0; at < nq; at += chunk) {
    const uint64_t cnt = std::min(chunk, nq - at);
    a.nq = (uint32_t)cnt, a.tiles = (uint32_t)ph_bits_scan_tiles(cnt, T);
    a.out_ids = out_ids + at * r, a.out_d = out_d + at * r, a.out_len = out_len + at;
    hipLaunchKernelGGL(ph_bits_query_kernel, dim3((uint32_t)std::min<uint64_t>((cnt + 3) / 4, 1u << 16)), dim3(256), 0, stream,
                       queries_dev + at * ldq, ldq, s->dim, (uint32_t)cnt, (uint32_t *)x->mem, sw);
    hipLaunchKernelGGL(fn, dim3(a.tiles * slices), dim3(64), lds, stream, a);  // tiles x slices <= 2^23: the chunk rule
    if (slices > 1u)
      hipLaunchKernelGGL(ph_bits_scan_merge_kernel, dim3((uint32_t)std::min<uint64_t>(cnt, 1u << 20)), dim3(64), merge_lds, stream, a);
    PH_HIP(hipGetLastError());
  }
  PH_HIP(hipEventRecord(x->done, stream));
  return 0;
}

// ------------------------------------------------------------------ entry points

// what all four calls ask of the store and of r
static int scan_check(const char *call, const phnsw_store *bits, uint64_t nq, uint64_t r) {
  if (!bits || !ph_store_bits(bits)) {
    ph_set_error("%s: needs a bits store (phnsw_store_create_bits), not %s", call, bits ? ph_rows_name(bits->kind) : "NULL");
    return PHNSW_E_UNSUPPORTED;
  }
  if (!ph_bits_scan_r_valid(r) || nq > 0xFFFFFFFFull || bits->n > 0x7FFFFFFFull) {
    ph_set_error("%s: needs 1 <= r <= %u, at most 2^32 - 1 queries and at most 2^31 - 1 rows", call, PH_BITS_SCAN_RMAX);
    return PHNSW_E_INVALID;
  }
  return 0;
}
// ... and the searches of `full` and k: what rerank_check (pq.hip) demands of a converted store
static int scan_search_check(const char *call, const phnsw_store *bits, const phnsw_store *full, uint64_t nq, uint64_t r, uint64_t k) {
  PH_TRY(scan_check(call, bits, nq, r));
  if (!full || !ph_store_f32(full) || full->n != bits->n || full->dim != bits->dim || full->metric != bits->metric ||
      full->device != bits->device || k == 0 || k > r) {
    ph_set_error("%s: needs the f32 store of the same n / dim / metric / device and 1 <= k <= r", call);
    return PHNSW_E_INVALID;
  }
  return 0;
}
static int scan_device_check(const char *call, const float *queries_dev, uint32_t ldq, uint32_t ld_min, bool aligned,
                             const void *ids, const void *d, const void *len) {
  if (!queries_dev || !ids || !d || !len || ldq < ld_min || (aligned && ((ldq % 4) || ((uintptr_t)queries_dev % 16)))) {
    ph_set_error("%s: invalid argument (queries and outputs not NULL; ldq >= %u%s)", call, ld_min,
                 aligned ? ", a multiple of 4, 16-byte base" : "");
    return PHNSW_E_INVALID;
  }
  return 0;
}

// the host forms: queries up as rows of `ld` floats (zero padded), the device form on the null stream, the leading
// `k` of each row of r down as u64 ids (ph_take_launch)
static int scan_host(const char *call, const phnsw_store *bits, const phnsw_store *full, const float *queries, uint64_t nq,
                     uint32_t r, uint32_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len) {
  if (!queries || !out_ids || !out_d || !out_len) {
    ph_set_error("%s: queries and outputs must not be NULL", call);
    return PHNSW_E_INVALID;
  }
  PH_HIP(hipSetDevice(bits->device));
  const uint32_t ld = bits->ld;
  float *qd = nullptr, *od = nullptr, *dk = nullptr;
  uint32_t *oid = nullptr, *olen = nullptr;
  uint64_t *ids64 = nullptr;
  int rc = 0;
  hipError_t e = hipMalloc(&qd, (size_t)nq * ld * 4);
  if (e == hipSuccess && ld != bits->dim) e = hipMemset(qd, 0, (size_t)nq * ld * 4);
  if (e == hipSuccess)
    e = hipMemcpy2D(qd, (size_t)ld * 4, queries, (size_t)bits->dim * 4, (size_t)bits->dim * 4, nq, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&oid, (size_t)nq * r * 4);
  if (e == hipSuccess) e = hipMalloc(&od, (size_t)nq * r * 4);
  if (e == hipSuccess) e = hipMalloc(&olen, nq * 4);
  if (e == hipSuccess) e = hipMalloc(&ids64, (size_t)nq * k * 8);
  if (e == hipSuccess) e = hipMalloc(&dk, (size_t)nq * k * 4);
  if (e != hipSuccess) rc = ph_hip_fail(e, "bits scan staging", __FILE__, __LINE__);
  if (!rc) rc = bits_scan_device(bits, qd, ld, nq, r, oid, od, olen, 0);
  if (!rc && full) rc = ph_rerank_launch(full, qd, ld, nq, r, k, olen, oid, od, 0);
  if (!rc) rc = ph_take_launch(oid, od, r, k, nq, ids64, dk, 0);
  if (!rc) {
    std::vector<uint32_t> h_len(nq);
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h_len.data(), olen, nq * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_ids, ids64, (size_t)nq * k * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_d, dk, (size_t)nq * k * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = ph_hip_fail(e, "bits scan", __FILE__, __LINE__);
    for (uint64_t i = 0; !rc && i < nq; i++) out_len[i] = std::min<uint64_t>(h_len[i], k);
  }
  for (void *p : {(void *)qd, (void *)od, (void *)dk, (void *)oid, (void *)olen, (void *)ids64})
    if (p) hipFree(p);
  return rc;
}

extern "C" int phnsw_bits_scan_topk_device(const phnsw_store *bits, const float *queries_dev, uint32_t ldq, uint64_t nq,
                                           uint64_t r, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                           void *stream) try {
  const char *const call = "phnsw_bits_scan_topk_device";
  PH_TRY(scan_check(call, bits, nq, r));
  if (nq == 0) return 0;
  PH_TRY(scan_device_check(call, queries_dev, ldq, bits->dim, false, out_ids_dev, out_d_dev, out_len_dev));
  return bits_scan_device(bits, queries_dev, ldq, nq, (uint32_t)r, out_ids_dev, out_d_dev, out_len_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_bits_scan_topk(const phnsw_store *bits, const float *queries, uint64_t nq, uint64_t r, uint64_t *out_ids,
                                    float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_bits_scan_topk";
  PH_TRY(scan_check(call, bits, nq, r));
  if (nq == 0) return 0;
  return scan_host(call, bits, nullptr, queries, nq, (uint32_t)r, (uint32_t)r, out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_bits_scan_search_device(const phnsw_store *bits, const phnsw_store *full, const float *queries_dev,
                                             uint32_t ldq, uint64_t nq, uint64_t r, uint64_t k, uint32_t *out_ids_dev,
                                             float *out_d_dev, uint32_t *out_len_dev, void *stream) try {
  const char *const call = "phnsw_bits_scan_search_device";
  PH_TRY(scan_search_check(call, bits, full, nq, r, k));
  if (nq == 0) return 0;
  PH_TRY(scan_device_check(call, queries_dev, ldq, full->ld, true, out_ids_dev, out_d_dev, out_len_dev));
  PH_TRY(bits_scan_device(bits, queries_dev, ldq, nq, (uint32_t)r, out_ids_dev, out_d_dev, out_len_dev, (hipStream_t)stream));
  return ph_rerank_launch(full, queries_dev, ldq, nq, (uint32_t)r, (uint32_t)k, out_len_dev, out_ids_dev, out_d_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_bits_scan_search(const phnsw_store *bits, const phnsw_store *full, const float *queries, uint64_t nq,
                                      uint64_t r, uint64_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_bits_scan_search";
  PH_TRY(scan_search_check(call, bits, full, nq, r, k));
  if (nq == 0) return 0;
  return scan_host(call, bits, full, queries, nq, (uint32_t)r, (uint32_t)k, out_ids, out_d, out_len);
} catch (...) { return ph_caught(); }
