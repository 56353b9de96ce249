// The host-pointer search entry points: what `Hnsw::search` binds to through the Rust shim
// (/root/reference/src/lib.rs:654-673; rust/parallel-hnsw-gpu).  Queries arrive in host memory, results leave to
// host memory as u64 ids -- the boundary BASELINE's drop-in story is about, so it gets the same care as the kernels:
//
//  * staging is PERSISTENT per index (device buffers and pinned mirrors sized to the high-water mark, two slots
//    with a stream each): no hipMalloc, no hipFree, no device-wide synchronisation per call;
//  * a long query list is cut into chunks that alternate between the two slots: the upload of chunk k+1 and the
//    download of chunk k-1 run beside the search of chunk k (the two search workspaces of the index alternate the
//    same way), and the first chunk is small so that the GPU starts after a fraction of the upload;
//  * the results are narrowed to the caller's top-k and widened to u64 ON THE DEVICE (ph_take_kernel): the
//    reference returns the whole queue and lets the caller truncate (lib.rs:1118), here the truncation saves the
//    transfer -- phnsw_search_batch_topk; k = number_of_candidates is phnsw_search_batch;
//  * queries whose frontier outgrew the spill workspace are re-run alone with 8x the room, as before.
#include <hip/hip_runtime.h>

#include <chrono>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "phnsw_internal.h"

#define PH_TRY(x)          \
  do {                     \
    int rc__ = (x);        \
    if (rc__) return rc__; \
  } while (0)

namespace {

struct Slot {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;  // after the slot's last download was enqueued
  float *q = nullptr;
  size_t q_bytes = 0;
  uint32_t *small = nullptr;  // device: qid | excl | len | status | index | stats(2)   [7][n_cap]
                              // (a collecting search by label has no index row: it stages `want` there)
  size_t n_cap = 0;
  uint32_t *ids = nullptr;  // device [cnt][ef]
  float *d = nullptr;
  size_t out_cap = 0;
  uint64_t *ids64 = nullptr;  // device [cnt][k]
  float *dk = nullptr;
  size_t take_cap = 0;
  uint32_t *h_small = nullptr;  // pinned mirror of `small`
  size_t h_cap = 0;
  uint32_t *filt = nullptr;  // device: the chunk's per-query allow bitmaps [cnt][stride] (filtered searches)
  size_t filt_bytes = 0;
  uint64_t c0 = 0, cnt = 0;  // the chunk in flight
  bool busy = false;
};

}  // namespace

struct PhHostStage {
  Slot slot[2];
  uint32_t *filt = nullptr;  // device: a call's shared allow bitmap, staged once per call
  size_t filt_bytes = 0;
  bool in_use = false;
  bool streams_checked = false;  // the two slots' streams were seen to run side by side (pair_streams)
};

namespace {

void slot_free(Slot &s) {
  if (s.q) hipFree(s.q);
  if (s.small) hipFree(s.small);
  if (s.ids) hipFree(s.ids);
  if (s.d) hipFree(s.d);
  if (s.ids64) hipFree(s.ids64);
  if (s.dk) hipFree(s.dk);
  if (s.filt) hipFree(s.filt);
  if (s.h_small) hipHostFree(s.h_small);
  if (s.done) hipEventDestroy(s.done);
  if (s.stream) hipStreamDestroy(s.stream);
  s = Slot();
}

template <class T>
int grow(T **p, size_t *have, size_t need, const char *what) {
  if (*have >= need) return 0;
  if (*p) hipFree(*p);
  *p = nullptr;
  *have = 0;
  need += need / 4;  // headroom: lists that grow a little do not reallocate every call
  hipError_t e = hipMalloc((void **)p, need);
  if (e != hipSuccess) return ph_hip_fail(e, what, __FILE__, __LINE__);
  *have = need;
  return 0;
}

// the pipeline needs its two streams on different hardware queues (ph_stream_beside, misc.hip): tried once per staging set
int pair_streams(PhHostStage &st) {
  if (st.streams_checked) return 0;
  Slot &a = st.slot[0], &b = st.slot[1];
  if (!a.stream) return 0;
  PH_TRY(ph_stream_beside(a.stream, &b.stream));
  st.streams_checked = true;
  return 0;
}

int slot_ensure(Slot &s, uint64_t cnt, uint32_t ld, bool has_q, uint32_t ef, uint32_t k) {
  if (!s.stream) {
    PH_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    PH_HIP(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
  }
  if (has_q) PH_TRY(grow(&s.q, &s.q_bytes, (size_t)cnt * ld * 4, "host path: query staging"));
  if (s.n_cap < cnt) {
    if (s.small) hipFree(s.small);
    s.small = nullptr;
    s.n_cap = 0;
    const size_t n = cnt + cnt / 4 + 64;
    hipError_t e = hipMalloc(&s.small, n * 7 * 4);
    if (e != hipSuccess) return ph_hip_fail(e, "host path: per-query staging", __FILE__, __LINE__);
    s.n_cap = n;
  }
  if (s.h_cap < s.n_cap) {
    if (s.h_small) hipHostFree(s.h_small);
    s.h_small = nullptr;
    s.h_cap = 0;
    hipError_t e = hipHostMalloc((void **)&s.h_small, s.n_cap * 7 * 4, hipHostMallocDefault);
    if (e != hipSuccess) return ph_hip_fail(e, "host path: pinned staging", __FILE__, __LINE__);
    s.h_cap = s.n_cap;
  }
  const size_t out = (size_t)cnt * ef;
  if (s.out_cap < out) {
    if (s.ids) hipFree(s.ids);
    if (s.d) hipFree(s.d);
    s.ids = nullptr;
    s.d = nullptr;
    s.out_cap = 0;
    const size_t n = out + out / 4;
    hipError_t e = hipMalloc(&s.ids, n * 4);
    if (e == hipSuccess) e = hipMalloc(&s.d, n * 4);
    if (e != hipSuccess) return ph_hip_fail(e, "host path: result staging", __FILE__, __LINE__);
    s.out_cap = n;
  }
  const size_t take = (size_t)cnt * k;
  if (s.take_cap < take) {
    if (s.ids64) hipFree(s.ids64);
    if (s.dk) hipFree(s.dk);
    s.ids64 = nullptr;
    s.dk = nullptr;
    s.take_cap = 0;
    const size_t n = take + take / 4;
    hipError_t e = hipMalloc(&s.ids64, n * 8);
    if (e == hipSuccess) e = hipMalloc(&s.dk, n * 4);
    if (e != hipSuccess) return ph_hip_fail(e, "host path: top-k staging", __FILE__, __LINE__);
    s.take_cap = n;
  }
  return 0;
}

// rows of `ef` results -> the leading k of each as u64 ids (0xFFFFFFFF -> PHNSW_EMPTY) + distances
__global__ void ph_take_kernel(const uint32_t *ids, const float *d, uint32_t ef, uint32_t k, uint64_t n, uint64_t *ids64,
                               float *dk) {
  const uint64_t total = n * k;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = x / k, c = x - r * k;
    const uint32_t id = ids[r * ef + c];
    ids64[x] = id == PH_EMPTY32 ? PHNSW_EMPTY : (uint64_t)id;
    dk[x] = d[r * ef + c];
  }
}

PhHostStage *stage_acquire(phnsw_index *ix) {
  std::lock_guard<std::mutex> g(ix->stage_mutex);
  for (PhHostStage *st : ix->stages)
    if (!st->in_use) {
      st->in_use = true;
      return st;
    }
  PhHostStage *st = new PhHostStage();
  st->in_use = true;
  ix->stages.push_back(st);
  return st;
}
void stage_release(phnsw_index *ix, PhHostStage *st) {
  std::lock_guard<std::mutex> g(ix->stage_mutex);
  st->in_use = false;
}
struct StageGuard {
  phnsw_index *ix;
  PhHostStage *st;
  ~StageGuard() { stage_release(ix, st); }
};

// chunk plan: short lists whole; long ones start with a small chunk (the GPU starts early), then even pieces
void plan_chunks(uint64_t nq, std::vector<uint64_t> &bounds) {
  uint64_t pipe_min = 6144, first = 1024, piece = 4096;
  if (const char *e = getenv("PHNSW_HOST_CHUNKS")) {  // "pipe_min,first,piece" -- tuning knob
    unsigned long long a = 0, b = 0, c = 0;
    if (sscanf(e, "%llu,%llu,%llu", &a, &b, &c) == 3 && b > 0 && c > 0) pipe_min = a, first = b, piece = c;
  }
  bounds.clear();
  bounds.push_back(0);
  if (nq < pipe_min) {
    bounds.push_back(nq);
    return;
  }
  uint64_t at = std::min(first, nq);
  bounds.push_back(at);
  const uint64_t rest = nq - at;
  uint64_t pieces = std::max<uint64_t>(1, (rest + piece - 1) / piece);
  // very long lists: pieces of at least PH_TWO_LAUNCH_MIN queries, so that each still descends in launches of
  // its own per large layer, its queries ordered by where they landed (api.hip; the upload of 100 MB per piece
  // hides behind the previous piece's search all the same)
  if (nq >= 2 * (uint64_t)PH_TWO_LAUNCH_MIN && !getenv("PHNSW_HOST_CHUNKS")) pieces = std::max<uint64_t>(1, rest / PH_TWO_LAUNCH_MIN);
  for (uint64_t p = 1; p <= pieces; p++) bounds.push_back(at + rest * p / pieces);
}

}  // namespace

int ph_take_launch(const uint32_t *ids, const float *d, uint32_t ef, uint32_t k, uint64_t n, uint64_t *ids64, float *dk,
                   hipStream_t s) {
  hipLaunchKernelGGL(ph_take_kernel, dim3((uint32_t)std::min<uint64_t>((n * k + 255) / 256, 4096)), dim3(256), 0, s, ids, d, ef,
                     k, n, ids64, dk);
  PH_HIP(hipGetLastError());
  return 0;
}

void ph_host_stages_free(phnsw_index *ix) {
  for (PhHostStage *st : ix->stages) {
    slot_free(st->slot[0]);
    slot_free(st->slot[1]);
    if (st->filt) hipFree(st->filt);
    delete st;
  }
  ix->stages.clear();
}

int ph_search_host(const phnsw_index *ix, const PhHostSearch &h) {
  if (!h.exact) PH_TRY(ph_check_sp(ix, h.sp));  // (the exact scan has no search parameters: ph_exact_check ran)
  const float *const queries = h.queries;
  const uint64_t *const qids = h.qids, *const exclude = h.exclude;
  const uint64_t nq = h.nq, out_k = h.out_k;
  uint64_t *const out_ids = h.out_ids, *const out_len = h.out_len, *const out_stats = h.out_stats, *const out_index = h.out_index;
  float *const out_d = h.out_d;
  // entries of a staged result row (a collecting search writes rows of k, whatever number_of_candidates is)
  const uint32_t ef = (h.exact || h.collect) ? (uint32_t)h.out_k : (uint32_t)h.sp->number_of_candidates;
  if ((!queries && !qids && !h.knn_mode) || !out_ids || !out_d || !out_len || nq > 0xFFFFFFFFull || out_k > ef) {
    ph_set_error("search: invalid argument (queries or ids, outputs, k <= number_of_candidates)");
    return PHNSW_E_INVALID;
  }
  if (nq == 0) return 0;
  const uint32_t k = out_k ? (uint32_t)out_k : ef;
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  if (qids)
    for (uint64_t i = 0; i < nq; i++)
      if (qids[i] >= s->n) {
        ph_set_error("search: stored query id %llu out of range", (unsigned long long)qids[i]);
        return PHNSW_E_INVALID;
      }
  phnsw_index *mix = const_cast<phnsw_index *>(ix);
  PhHostStage *st = stage_acquire(mix);
  StageGuard guard{mix, st};
  std::vector<uint64_t> bounds;
  plan_chunks(nq, bounds);
  const size_t n_chunks = bounds.size() - 1;
  std::vector<uint32_t> redo;
  int rc = 0;

  // download of the chunk a slot holds: per-query words through the pinned mirror, result rows straight into the
  // caller's arrays; returns after everything of that chunk has landed
  auto finish = [&](Slot &sl) -> int {
    if (!sl.busy) return 0;
    sl.busy = false;
    const uint64_t c0 = sl.c0, cnt = sl.cnt, N = sl.cnt;  // the per-query words are laid out [7][cnt]
    PH_TRY(ph_take_launch(sl.ids, sl.d, ef, k, cnt, sl.ids64, sl.dk, sl.stream));
    // len | status | index | stats sit contiguously at rows 2..6 of `small`
    PH_HIP(hipMemcpyAsync(sl.h_small + 2 * N, sl.small + 2 * N, 5 * N * 4, hipMemcpyDeviceToHost, sl.stream));
    PH_HIP(hipMemcpyAsync(out_ids + c0 * k, sl.ids64, (size_t)cnt * k * 8, hipMemcpyDeviceToHost, sl.stream));
    PH_HIP(hipMemcpyAsync(out_d + c0 * k, sl.dk, (size_t)cnt * k * 4, hipMemcpyDeviceToHost, sl.stream));
    PH_HIP(hipStreamSynchronize(sl.stream));
    const uint32_t *h_len = sl.h_small + 2 * N, *h_status = sl.h_small + 3 * N, *h_index = sl.h_small + 4 * N,
                   *h_stats = sl.h_small + 5 * N;
    for (uint64_t i = 0; i < cnt; i++) {
      if (h_status[i] == 4) {
        ph_set_error("search: a candidate vector is missing from a lower layer (layers not nested, lib.rs:261)");
        return PHNSW_E_MISSING_NODE;
      }
      if (h_status[i] == 5) redo.push_back((uint32_t)(c0 + i));
      out_len[c0 + i] = std::min<uint32_t>(h_len[i], k);
    }
    if (out_stats)
      for (uint64_t i = 0; i < 2 * cnt; i++) out_stats[2 * c0 + i] = h_stats[i];
    if (out_index)
      for (uint64_t i = 0; i < cnt; i++) out_index[c0 + i] = h_index[i] == 0xFFFFFFFFu ? UINT64_MAX : h_index[i];
    return 0;
  };

  // the allow-list: a shared bitmap goes to the device once per call, per-query bitmaps travel with their chunk
  const PhFilter &filter = h.filter;
  const bool filtered = filter.words != nullptr;
  const bool per_query = filtered && filter.stride != 0;
  const bool labeled = filter.label_of != nullptr;  // the collecting search by label: the column is on the device, want [nq] here
  const uint64_t filter_words = (s->n + 31u) / 32u;
  PhFilter fdev = {nullptr, 0u, filtered ? filter.flags : 0u};
  if (filtered && h.filter_on_device) fdev.words = filter.words;
  if (filtered && !h.filter_on_device && !per_query) {
    Slot &s0 = st->slot[0];
    if (!s0.stream) {
      PH_HIP(hipStreamCreateWithFlags(&s0.stream, hipStreamNonBlocking));
      PH_HIP(hipEventCreateWithFlags(&s0.done, hipEventDisableTiming));
    }
    PH_TRY(grow(&st->filt, &st->filt_bytes, (size_t)filter_words * 4, "host path: filter staging"));
    PH_HIP(hipMemcpyAsync(st->filt, filter.words, (size_t)filter_words * 4, hipMemcpyHostToDevice, s0.stream));
    PH_HIP(hipStreamSynchronize(s0.stream));  // both slots' streams read it
    fdev.words = st->filt;
  }
  if (n_chunks >= 2 && !st->streams_checked) {  // the first pipelined call of this staging set: see pair_streams
    for (Slot &sl : st->slot)
      if (!sl.stream) {
        PH_HIP(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
        PH_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
      }
    rc = pair_streams(*st);
  }
  // queries [first, first + cnt) into a slot and onto its stream: the query rows (padded to the store's row length), the
  // id and exclude words, the per-query bitmaps, then the search.  A failed upload leaves the chunk loop at once, the
  // step's other failures drain the slots first, and the re-run loop returns at once on both: as before the step was
  // written once (which paths should drain is a question of its own)
  bool upload_failed = false;
#define PH_STAGE_HIP(x)                               \
  do {                                                \
    hipError_t e__ = (x);                             \
    if (e__ != hipSuccess) {                          \
      upload_failed = true;                           \
      return ph_hip_fail(e__, #x, __FILE__, __LINE__); \
    }                                                 \
  } while (0)
  auto stage_and_launch = [&](Slot &sl, uint64_t first, uint64_t cnt, uint32_t ovf_cap) -> int {
    PH_TRY(slot_ensure(sl, cnt, s->ld, queries != nullptr, ef, k));
    const uint64_t N = cnt;  // the per-query words are laid out [7][cnt]: qid | excl | len | status | index | stats(2)
    if (queries) {
      if (s->ld != s->dim) {
        PH_STAGE_HIP(hipMemsetAsync(sl.q, 0, (size_t)cnt * s->ld * 4, sl.stream));
        PH_STAGE_HIP(hipMemcpy2DAsync(sl.q, (size_t)s->ld * 4, queries + first * s->dim, (size_t)s->dim * 4, (size_t)s->dim * 4, cnt,
                                hipMemcpyHostToDevice, sl.stream));
      } else {
        PH_STAGE_HIP(hipMemcpyAsync(sl.q, queries + first * s->dim, (size_t)cnt * s->dim * 4, hipMemcpyHostToDevice, sl.stream));
      }
    }
    if (qids || exclude) {
      if (qids)
        for (uint64_t i = 0; i < cnt; i++) sl.h_small[i] = (uint32_t)qids[first + i];
      if (exclude)
        for (uint64_t i = 0; i < cnt; i++) sl.h_small[N + i] = exclude[first + i] >= s->n ? PH_EMPTY32 : (uint32_t)exclude[first + i];
      PH_STAGE_HIP(hipMemcpyAsync(sl.small, sl.h_small, 2 * N * 4, hipMemcpyHostToDevice, sl.stream));
    }
    if (per_query) {
      const size_t bytes = (size_t)cnt * filter.stride * 4;
      PH_TRY(grow(&sl.filt, &sl.filt_bytes, bytes, "host path: per-query filter staging"));
      PH_STAGE_HIP(hipMemcpyAsync(sl.filt, filter.words + first * filter.stride, bytes, hipMemcpyHostToDevice, sl.stream));
      fdev.words = sl.filt;
      fdev.stride = filter.stride;
    }
    if (labeled) {  // the wanted labels travel with their chunk, in the (unused) index row of the per-query words
      for (uint64_t i = 0; i < cnt; i++) sl.h_small[4 * N + i] = filter.want[first + i];
      PH_STAGE_HIP(hipMemcpyAsync(sl.small + 4 * N, sl.h_small + 4 * N, N * 4, hipMemcpyHostToDevice, sl.stream));
    }
    if (h.exact) {  // the scan over the allow-list (filter_exact.hip) on the same staging: rows of k entries
      PhExactCall x = {};
      if (queries) x.queries = sl.q;
      if (qids) x.qids = sl.small;
      if (exclude) x.exclude = sl.small + N;
      if (filtered) x.filter = fdev;
      x.ldq = s->ld, x.nq = cnt, x.k = k;
      x.out_ids = sl.ids, x.out_d = sl.d, x.out_len = sl.small + 2 * N, x.status = sl.small + 3 * N;
      x.stream = sl.stream;
      PH_TRY(ph_exact_device(ix, x));
      sl.c0 = first;
      sl.cnt = cnt;
      sl.busy = true;
      return 0;
    }
    PhSearchCall c = {};
    if (queries) c.queries = sl.q;
    if (qids) c.qids = sl.small;
    if (exclude) c.exclude = sl.small + N;
    if (filtered) c.filter = fdev;
    if (labeled) c.filter.label_of = filter.label_of, c.filter.want = sl.small + 4 * N;
    if (h.collect) c.collect_k = k, c.collect_flags = h.collect_flags;
    c.ldq = s->ld, c.nq = cnt, c.sp = h.sp, c.upto = h.upto;
    c.out_ids = sl.ids, c.out_d = sl.d, c.out_len = sl.small + 2 * N, c.status = sl.small + 3 * N;
    if (out_index) c.out_index = sl.small + 4 * N;
    c.out_stats = sl.small + 5 * N;
    c.ovf_cap = ovf_cap, c.stream = sl.stream;
    c.knn_mode = h.knn_mode, c.first_node = (uint32_t)first;  // first_node: read in the knn modes only
    PH_TRY(ph_search_device(ix, c));
    sl.c0 = first;
    sl.cnt = cnt;
    sl.busy = true;
    return 0;
  };
#undef PH_STAGE_HIP
  for (size_t c = 0; c < n_chunks && !rc; c++) {
    Slot &sl = st->slot[c & 1];
    rc = finish(sl);  // the slot's previous chunk (two chunks back) comes home first
    if (!rc) rc = stage_and_launch(sl, bounds[c], bounds[c + 1] - bounds[c], 0);
    if (upload_failed) return rc;
  }
  // the (up to two) chunks still in flight, oldest first
  if (n_chunks >= 2) {
    int r2 = finish(st->slot[n_chunks & 1]);
    if (!rc) rc = r2;
  }
  {
    int r2 = finish(st->slot[(n_chunks - 1) & 1]);
    if (!rc) rc = r2;
  }
  if (rc) {
    for (Slot &sl : st->slot) {
      if (sl.stream) hipStreamSynchronize(sl.stream);
      sl.busy = false;
    }
    return rc;
  }

  // queries whose frontier spill outgrew the workspace: rerun them alone with 8x the room (rare)
  uint32_t ovf_cap = ph_default_ovf_cap(h.collect ? (uint32_t)h.sp->number_of_candidates : ef);
  for (int attempt = 0; !redo.empty(); attempt++) {
    if (h.knn_mode) {
      ph_set_error("knn: frontier spill exceeded %u entries", ovf_cap);
      return PHNSW_E_OVERFLOW;
    }
    if (attempt == 3) {
      ph_set_error("search: frontier spill exceeded %u entries for %zu queries", ovf_cap, redo.size());
      return PHNSW_E_OVERFLOW;
    }
    ovf_cap *= 8;
    std::vector<uint32_t> todo;
    todo.swap(redo);
    Slot &sl = st->slot[0];
    for (uint32_t qi : todo) {
      PH_TRY(stage_and_launch(sl, qi, 1, ovf_cap));
      PH_TRY(finish(sl));
    }
  }
  return 0;
}

// ------------------------------------------------------------------ C ABI

// what every host entry point below asks for: queries or ids, the parameters, the three result arrays
static PhHostSearch host_call(const float *queries, const uint64_t *qids, uint64_t nq, const phnsw_search_params *sp,
                              uint64_t *out_ids, float *out_d, uint64_t *out_len) {
  PhHostSearch h = {};
  h.queries = queries, h.qids = qids, h.nq = nq, h.sp = sp;
  h.out_ids = out_ids, h.out_d = out_d, h.out_len = out_len;
  return h;
}

// Hnsw::search for a batch of AbstractVector::Unstored queries  lib.rs:663-665
extern "C" int phnsw_search_batch(const phnsw_index *ix, const float *queries, uint64_t nq,
                                  const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude,
                                  uint64_t *out_ids, float *out_d, uint64_t *out_len, uint64_t *out_stats) try {
  if (!queries && nq) {
    ph_set_error("phnsw_search_batch: queries is NULL");
    return PHNSW_E_INVALID;
  }
  PhHostSearch h = host_call(queries, nullptr, nq, sp, out_ids, out_d, out_len);
  h.upto = upto_layers, h.exclude = exclude, h.out_stats = out_stats;
  return ph_search_host(ix, h);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_batch_stored(const phnsw_index *ix, const uint64_t *qids, uint64_t nq,
                                         const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude,
                                         uint64_t *out_ids, float *out_d, uint64_t *out_len, uint64_t *out_stats) try {
  if (!qids && nq) {
    ph_set_error("phnsw_search_batch_stored: qids is NULL");
    return PHNSW_E_INVALID;
  }
  PhHostSearch h = host_call(nullptr, qids, nq, sp, out_ids, out_d, out_len);
  h.upto = upto_layers, h.exclude = exclude, h.out_stats = out_stats;
  return ph_search_host(ix, h);
} catch (...) { return ph_caught(); }

// the same keeping only the best k results of every query: the truncation callers of Hnsw::search do themselves
// (lib.rs:1118 takes neighborhood_size of them, a k-NN service takes k) happens before the transfer
extern "C" int phnsw_search_batch_topk(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                                       const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude,
                                       uint64_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len) try {
  if (((!queries) == (!qids)) && nq) {
    ph_set_error("phnsw_search_batch_topk: pass queries or qids (exactly one)");
    return PHNSW_E_INVALID;
  }
  if (k == 0) {
    ph_set_error("phnsw_search_batch_topk: k must be 1..number_of_candidates");
    return PHNSW_E_INVALID;
  }
  PhHostSearch h = host_call(queries, qids, nq, sp, out_ids, out_d, out_len);
  h.upto = upto_layers, h.exclude = exclude, h.out_k = k;
  return ph_search_host(ix, h);
} catch (...) { return ph_caught(); }

// Hnsw::search_instrumented  lib.rs:667-673: results + the index_distance of search_layers_instrumented
// (search.rs:93-140; usize::MAX = UINT64_MAX when no layer ran)
extern "C" int phnsw_search_instrumented(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                                         const phnsw_search_params *sp, uint64_t *out_ids, float *out_d,
                                         uint64_t *out_len, uint64_t *out_index_distance) try {
  if (ix)
    if (int rc = ph_search_only_unsupported(ix->store, "phnsw_search_instrumented")) return rc;
  if ((((!queries) == (!qids)) && nq) || !out_index_distance) {
    ph_set_error("phnsw_search_instrumented: pass queries or qids (exactly one) and out_index_distance");
    return PHNSW_E_INVALID;
  }
  PhHostSearch h = host_call(queries, qids, nq, sp, out_ids, out_d, out_len);
  h.out_index = out_index_distance;
  return ph_search_host(ix, h);
} catch (...) { return ph_caught(); }

// Hnsw::search with closest_vectors' `include` (lib.rs:250-277) as an allow bitmap over VectorIds
extern "C" int phnsw_search_batch_filtered(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                                           const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude,
                                           const uint32_t *filter, uint32_t filter_stride_words, uint32_t flags, uint64_t k,
                                           uint64_t *out_ids, float *out_d, uint64_t *out_len, uint64_t *out_stats) try {
  if (((!queries) == (!qids)) && nq) {
    ph_set_error("phnsw_search_batch_filtered: pass queries or qids (exactly one)");
    return PHNSW_E_INVALID;
  }
  if (!ix || ix->layers.empty()) {
    ph_set_error("search: null index/params or index without layers");
    return PHNSW_E_INVALID;
  }
  PhHostSearch h = host_call(queries, qids, nq, sp, out_ids, out_d, out_len);
  h.upto = upto_layers, h.exclude = exclude, h.out_k = k, h.out_stats = out_stats;
  PH_TRY(ph_filter_check(ix, filter, filter_stride_words, flags, "phnsw_search_batch_filtered", &h.filter));
  h.filter_on_device = !h.filter.words && ix->default_filter;  // phnsw_index_set_filter_device: device words
  if (h.filter_on_device) h.filter.words = ix->default_filter;
  return ph_search_host(ix, h);
} catch (...) { return ph_caught(); }

// the exact top-k of the allowed vectors, by a scan instead of the graph search: the call for selective filters
extern "C" int phnsw_search_exact_filtered(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                                           const uint64_t *exclude, const uint32_t *filter, uint32_t filter_stride_words,
                                           uint64_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len) try {
  PH_TRY(ph_exact_check(ix, k, "phnsw_search_exact_filtered"));
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("phnsw_search_exact_filtered: pass queries or qids (exactly one)");
    return PHNSW_E_INVALID;
  }
  PhHostSearch h = host_call(queries, qids, nq, nullptr, out_ids, out_d, out_len);
  h.exclude = exclude, h.out_k = k, h.exact = true;
  PH_TRY(ph_filter_check(ix, filter, filter_stride_words, 0u, "phnsw_search_exact_filtered", &h.filter));
  h.filter_on_device = !h.filter.words && ix->default_filter;  // phnsw_index_set_filter_device: device words
  if (h.filter_on_device) h.filter.words = ix->default_filter;
  return ph_search_host(ix, h);
} catch (...) { return ph_caught(); }

// ---- the collecting search: the plain search whose last layer keeps the best ALLOWED rows it evaluates (phnsw.h)

// what the four collecting entry points check first, in this order: index and parameters, the flags, k, the stride
int ph_collect_check(const phnsw_index *ix, const phnsw_search_params *sp, uint32_t stride, uint32_t flags, uint64_t k,
                     const char *call) {
  if (ix) PH_TRY(ph_bits_unsupported(ix->store, call));  // a bits store has the plain walk alone
  PH_TRY(ph_check_sp(ix, sp));
  if (flags & ~(uint32_t)PHNSW_COLLECT_EXTEND) {
    ph_set_error("%s: unknown flag bits 0x%x", call, flags);
    return PHNSW_E_INVALID;
  }
  if (k == 0 || k > PH_COLLECT_KMAX) {
    ph_set_error("%s: k must be 1..%u (got %llu)", call, PH_COLLECT_KMAX, (unsigned long long)k);
    return PHNSW_E_INVALID;
  }
  const uint64_t words = (ix->store->n + 31u) / 32u;
  if (stride && stride < words) {
    ph_set_error("%s: filter_stride_words %u is below the %llu words of one bitmap (0 = one shared bitmap)", call, stride,
                 (unsigned long long)words);
    return PHNSW_E_INVALID;
  }
  return 0;
}

extern "C" int phnsw_search_collect(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                                    const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude,
                                    const uint32_t *filter, uint32_t filter_stride_words, uint32_t flags, uint64_t k,
                                    uint64_t *out_ids, float *out_d, uint64_t *out_len, uint64_t *out_stats) try {
  const char *const call = "phnsw_search_collect";
  PH_TRY(ph_collect_check(ix, sp, filter_stride_words, flags, k, call));
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  PhHostSearch h = host_call(queries, qids, nq, sp, out_ids, out_d, out_len);
  h.upto = upto_layers, h.exclude = exclude, h.out_k = k, h.out_stats = out_stats;
  h.collect = true, h.collect_flags = flags;
  h.filter.words = filter, h.filter.stride = filter ? filter_stride_words : 0u;
  PH_TRY(ph_collect_filter(ix, &h.filter, &h.filter_on_device));
  return ph_search_host(ix, h);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_collect_labeled(const phnsw_index *ix, const phnsw_labels *lb, const float *queries,
                                            const uint64_t *qids, uint64_t nq, const phnsw_search_params *sp,
                                            uint32_t upto_layers, const uint64_t *exclude, const uint32_t *want, uint32_t flags,
                                            uint64_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len,
                                            uint64_t *out_stats) try {
  const char *const call = "phnsw_search_collect_labeled";
  PH_TRY(ph_collect_check(ix, sp, 0u, flags, k, call));
  PH_TRY(ph_labels_fresh(ix, lb, call));
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!want) {
    ph_set_error("%s: invalid argument (want is NULL)", call);
    return PHNSW_E_INVALID;
  }
  PhHostSearch h = host_call(queries, qids, nq, sp, out_ids, out_d, out_len);
  h.upto = upto_layers, h.exclude = exclude, h.out_k = k, h.out_stats = out_stats;
  h.collect = true, h.collect_flags = flags;
  h.filter.label_of = ph_labels_column(lb), h.filter.want = want;
  return ph_search_host(ix, h);
} catch (...) { return ph_caught(); }
