// The exhaustive int8 scan over an ALLOW-LIST of rows: phnsw_i8q_scan_topk_filtered[_device] and
// phnsw_i8q_scan_search_filtered[_device].  The scan of scan_i8q.hip restricted to the rows whose bit is set: the same
// quantised query, the same v_mfma_i32_16x16x64_i8 over the same images, the same ph_i8q_distance -- and because an
// integer sum has no order, for every (query, row) the bits the unfiltered scan computes.
//
//   result of a query = the min(r, allowed rows) allowed rows with the smallest (distance, id), ascending.
//
// Two forms of the one kernel body (scan_i8q_kernel.h says what each changes):
//   * a SHARED bitmap (filter_stride_words 0) is compacted ON THE DEVICE by scan_fp4_filtered.hip's
//     ph_fp4_scan_list_enqueue, nothing read back; the LIST form gathers the listed rows through the LDS tile, its
//     slices cut over ceil(m / tile rows) tiles, so its cost follows the allowed rows;
//   * PER-QUERY bitmaps go to the MASK form: the full scan, a survivor's bit tested before it is staged.
// Launcher, scratch, merge kernel, host staging and argument checks are scan_i8q.hip's (ph_i8q_scan_enqueue / _host).
// No router between the forms or towards phnsw_search_exact_filtered: the stride chooses.
#include <hip/hip_runtime.h>

#include "scan_i8q_kernel.h"

template <int S, int RG, int FORM>
__global__ __launch_bounds__(256) void ph_i8q_scan_filtered_kernel(PhI8qScanArgs a) {
  ph_i8q_scan_body<S, RG, FORM>(a);
}

template <int FORM>
static PhI8qScanFn filtered_fn(int cls) {  // the tile caps are ph_i8q_scan_tile_cap's
  switch (cls) {
    case 2: return ph_i8q_scan_filtered_kernel<2, 4, FORM>;
    case 7: return ph_i8q_scan_filtered_kernel<7, 4, FORM>;
    case 13: return ph_i8q_scan_filtered_kernel<13, 2, FORM>;
    case 25: return ph_i8q_scan_filtered_kernel<25, 1, FORM>;
    default: return nullptr;
  }
}
PhI8qScanFn ph_i8q_scan_filtered_fn(int cls, int form) {
  return form == PH_I8Q_SCAN_LIST ? filtered_fn<PH_I8Q_SCAN_LIST>(cls) : filtered_fn<PH_I8Q_SCAN_MASK>(cls);
}

// ------------------------------------------------------------------ entry points

// what the four calls ask of the filter, after ph_i8q_scan_check has seen the store
static int filter_check(const char *call, const phnsw_store *i8q, const uint32_t *filter, uint32_t stride) {
  if (!filter) {
    ph_set_error("%s: filter must not be NULL (the unfiltered phnsw_i8q_scan_* calls scan every row)", call);
    return PHNSW_E_INVALID;
  }
  if (stride && stride < ph_exact_words(i8q->n)) {
    ph_set_error("%s: filter_stride_words %u is neither 0 nor at least ceil(n / 32) = %llu", call, stride,
                 (unsigned long long)ph_exact_words(i8q->n));
    return PHNSW_E_INVALID;
  }
  return 0;
}

extern "C" int phnsw_i8q_scan_topk_filtered_device(const phnsw_store *i8q, const float *queries_dev, uint32_t ldq, uint64_t nq,
                                                   uint64_t r, const uint32_t *filter_dev, uint32_t filter_stride_words,
                                                   uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                   void *stream) try {
  const char *const call = "phnsw_i8q_scan_topk_filtered_device";
  PH_TRY(ph_i8q_scan_check(call, i8q, nq, r));
  PH_TRY(filter_check(call, i8q, filter_dev, filter_stride_words));
  if (nq == 0) return 0;
  PH_TRY(ph_i8q_scan_device_check(call, queries_dev, ldq, i8q->dim, false, out_ids_dev, out_d_dev, out_len_dev));
  return ph_i8q_scan_enqueue(i8q, queries_dev, ldq, nq, (uint32_t)r, filter_dev, filter_stride_words, out_ids_dev, out_d_dev,
                             out_len_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_i8q_scan_topk_filtered(const phnsw_store *i8q, const float *queries, uint64_t nq, uint64_t r,
                                            const uint32_t *filter, uint32_t filter_stride_words, uint64_t *out_ids,
                                            float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_i8q_scan_topk_filtered";
  PH_TRY(ph_i8q_scan_check(call, i8q, nq, r));
  PH_TRY(filter_check(call, i8q, filter, filter_stride_words));
  if (nq == 0) return 0;
  return ph_i8q_scan_host(call, i8q, nullptr, queries, nq, (uint32_t)r, (uint32_t)r, filter, filter_stride_words, out_ids, out_d,
                          out_len);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_i8q_scan_search_filtered_device(const phnsw_store *i8q, const phnsw_store *full, const float *queries_dev,
                                                     uint32_t ldq, uint64_t nq, uint64_t r, uint64_t k,
                                                     const uint32_t *filter_dev, uint32_t filter_stride_words,
                                                     uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                     void *stream) try {
  const char *const call = "phnsw_i8q_scan_search_filtered_device";
  PH_TRY(ph_i8q_scan_search_check(call, i8q, full, nq, r, k));
  PH_TRY(filter_check(call, i8q, filter_dev, filter_stride_words));
  if (nq == 0) return 0;
  PH_TRY(ph_i8q_scan_device_check(call, queries_dev, ldq, full->ld, true, out_ids_dev, out_d_dev, out_len_dev));
  PH_TRY(ph_i8q_scan_enqueue(i8q, queries_dev, ldq, nq, (uint32_t)r, filter_dev, filter_stride_words, out_ids_dev, out_d_dev,
                             out_len_dev, (hipStream_t)stream));
  return ph_rerank_launch(full, queries_dev, ldq, nq, (uint32_t)r, (uint32_t)k, out_len_dev, out_ids_dev, out_d_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_i8q_scan_search_filtered(const phnsw_store *i8q, const phnsw_store *full, const float *queries, uint64_t nq,
                                              uint64_t r, uint64_t k, const uint32_t *filter, uint32_t filter_stride_words,
                                              uint64_t *out_ids, float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_i8q_scan_search_filtered";
  PH_TRY(ph_i8q_scan_search_check(call, i8q, full, nq, r, k));
  PH_TRY(filter_check(call, i8q, filter, filter_stride_words));
  if (nq == 0) return 0;
  return ph_i8q_scan_host(call, i8q, full, queries, nq, (uint32_t)r, (uint32_t)k, filter, filter_stride_words, out_ids, out_d,
                          out_len);
} catch (...) { return ph_caught(); }
