// The exhaustive MXFP4 scan over an ALLOW-LIST of rows: phnsw_fp4_scan_topk_filtered[_device] and
// phnsw_fp4_scan_search_filtered[_device].  The scan of scan_fp4.hip restricted to the rows whose bit is set: the same
// quantised query, the same chain of v_mfma_scale_f32_16x16x128_f8f6f4, and -- because a score never depends on the rows
// beside it in the instruction -- for every (query, row) the bits the unfiltered scan computes.
//
//   result of a query = the min(r, allowed rows) allowed rows with the smallest (finalize_metric(s), id), ascending.
//
// Two forms of the one kernel body (scan_fp4_kernel.h says what each changes):
//   * a SHARED bitmap (filter_stride_words 0) is compacted ON THE DEVICE, nothing read back: a popcount per word
//     (ph_fp4_list_popc_kernel), their exclusive prefix by one workgroup (ph_fp4_list_prefix_kernel, more than one turn
//     past 1024 words) and every word's ids written at its offset (ph_fp4_list_expand_kernel), which also pads the list
//     to whole row groups with its last id.  m stays in device memory; the LIST form reads it and cuts its slices over
//     ceil(m / 16) row groups, so its cost follows the allowed rows;
//   * PER-QUERY bitmaps go to the MASK form: the full scan, a survivor's bit tested before it is staged.
// Launcher, scratch, merge kernel, host staging and argument checks are scan_fp4.hip's (ph_fp4_scan_enqueue / _host).
// No router between the forms or towards phnsw_search_exact_filtered: the stride chooses.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "scan_fp4_kernel.h"

template <int S, int G, int FORM>
__global__ __launch_bounds__(64) void ph_fp4_scan_filtered_kernel(PhFp4ScanArgs a) {
  ph_fp4_scan_body<S, G, FORM>(a);
}

template <int FORM>
static PhFp4ScanFn filtered_fn(int cls, uint32_t T) {
  switch (cls * 100 + (int)T) {
    case 216: return ph_fp4_scan_filtered_kernel<2, 1, FORM>;
    case 232: return ph_fp4_scan_filtered_kernel<2, 2, FORM>;
    case 264: return ph_fp4_scan_filtered_kernel<2, 4, FORM>;
    case 616: return ph_fp4_scan_filtered_kernel<6, 1, FORM>;
    case 632: return ph_fp4_scan_filtered_kernel<6, 2, FORM>;
    case 664: return ph_fp4_scan_filtered_kernel<6, 4, FORM>;
    case 1216: return ph_fp4_scan_filtered_kernel<12, 1, FORM>;
    case 1232: return ph_fp4_scan_filtered_kernel<12, 2, FORM>;
    default: return nullptr;
  }
}
PhFp4ScanFn ph_fp4_scan_filtered_fn(int cls, uint32_t T, int form) {
  return form == PH_FP4_SCAN_LIST ? filtered_fn<PH_FP4_SCAN_LIST>(cls, T) : filtered_fn<PH_FP4_SCAN_MASK>(cls, T);
}

// ------------------------------------------------------------------ the row list of a shared bitmap

struct PhFp4ListArgs {
  const uint32_t *filter;  // [nwords]
  uint32_t n, nwords;
  uint32_t *head;  // [PH_FP4_SCAN_HEAD_WORDS]: [0] = m
  uint32_t *off;   // [nwords + 1]
  uint32_t *list;  // [ph_fp4_scan_list_len(n)]
};

__global__ __launch_bounds__(256) void ph_fp4_list_popc_kernel(PhFp4ListArgs a) {
  for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < a.nwords; w += (uint64_t)gridDim.x * 256u)
    a.off[w] = (uint32_t)__popc(a.filter[w] & ph_fp4_scan_word_mask(w, a.n));
}

// One workgroup walks the counts 1024 at a time and leaves their exclusive prefix in place; the total, m <= n <= 2^31 - 1,
// goes behind the last word and into the head
__global__ __launch_bounds__(1024) void ph_fp4_list_prefix_kernel(PhFp4ListArgs a) {
  uint32_t base = 0;
  for (uint64_t at = 0; at < a.nwords; at += 1024u) {
    const uint64_t w = at + threadIdx.x;
    const uint32_t before = ph_block_exclusive_scan(w < a.nwords ? a.off[w] : 0u, base);
    if (w < a.nwords) a.off[w] = before;
    __syncthreads();  // the totals are rewritten by the next 1024
  }
  if (threadIdx.x == 0) a.off[a.nwords] = base, a.head[0] = base;
}

// Every word writes its rows at its offset, ascending within the word and across words; the word that holds the last
// allowed row repeats it up to the next multiple of 16 entries.  Every index written is below ph_fp4_scan_list_len(m) <=
// ph_fp4_scan_list_len(n).
__global__ __launch_bounds__(256) void ph_fp4_list_expand_kernel(PhFp4ListArgs a) {
  const uint32_t m = a.off[a.nwords];
  for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < a.nwords; w += (uint64_t)gridDim.x * 256u) {
    const uint32_t bits = a.filter[w] & ph_fp4_scan_word_mask(w, a.n);
    if (!bits) continue;
    uint32_t o = a.off[w];
    for (uint32_t t = bits; t; t &= t - 1u) a.list[o++] = (uint32_t)w * 32u + (uint32_t)__ffs((int)t) - 1u;
    if (o == m) {
      const uint32_t last = (uint32_t)w * 32u + 31u - (uint32_t)__clz((int)bits);
      for (uint64_t p = m; p < ph_fp4_scan_list_len(m); p++) a.list[p] = last;
    }
  }
}

int ph_fp4_scan_list_enqueue(const uint32_t *filter_dev, uint64_t n, uint32_t *pre, hipStream_t stream) {
  PhFp4ListArgs l = {};
  l.filter = filter_dev, l.n = (uint32_t)n, l.nwords = (uint32_t)ph_exact_words(n);
  l.head = pre, l.off = pre + PH_FP4_SCAN_HEAD_WORDS, l.list = pre + ph_fp4_scan_pre_list(n);
  const uint32_t wgrid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((l.nwords + 255u) / 256u, 1u), 1u << 16);
  hipLaunchKernelGGL(ph_fp4_list_popc_kernel, dim3(wgrid), dim3(256), 0, stream, l);
  hipLaunchKernelGGL(ph_fp4_list_prefix_kernel, dim3(1), dim3(1024), 0, stream, l);
  hipLaunchKernelGGL(ph_fp4_list_expand_kernel, dim3(wgrid), dim3(256), 0, stream, l);
  PH_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ entry points

// what the four calls ask of the filter, after ph_fp4_scan_check has seen the store
static int filter_check(const char *call, const phnsw_store *fp4, const uint32_t *filter, uint32_t stride) {
  if (!filter) {
    ph_set_error("%s: filter must not be NULL (the unfiltered phnsw_fp4_scan_* calls scan every row)", call);
    return PHNSW_E_INVALID;
  }
  if (stride && stride < ph_exact_words(fp4->n)) {
    ph_set_error("%s: filter_stride_words %u is neither 0 nor at least ceil(n / 32) = %llu", call, stride,
                 (unsigned long long)ph_exact_words(fp4->n));
    return PHNSW_E_INVALID;
  }
  return 0;
}

extern "C" int phnsw_fp4_scan_topk_filtered_device(const phnsw_store *fp4, const float *queries_dev, uint32_t ldq, uint64_t nq,
                                                   uint64_t r, const uint32_t *filter_dev, uint32_t filter_stride_words,
                                                   uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                   void *stream) try {
  const char *const call = "phnsw_fp4_scan_topk_filtered_device";
  PH_TRY(ph_fp4_scan_check(call, fp4, nq, r));
  PH_TRY(filter_check(call, fp4, filter_dev, filter_stride_words));
  if (nq == 0) return 0;
  PH_TRY(ph_fp4_scan_device_check(call, queries_dev, ldq, fp4->dim, false, out_ids_dev, out_d_dev, out_len_dev));
  return ph_fp4_scan_enqueue(fp4, queries_dev, ldq, nq, (uint32_t)r, filter_dev, filter_stride_words, out_ids_dev, out_d_dev,
                             out_len_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_fp4_scan_topk_filtered(const phnsw_store *fp4, const float *queries, uint64_t nq, uint64_t r,
                                            const uint32_t *filter, uint32_t filter_stride_words, uint64_t *out_ids,
                                            float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_fp4_scan_topk_filtered";
  PH_TRY(ph_fp4_scan_check(call, fp4, nq, r));
  PH_TRY(filter_check(call, fp4, filter, filter_stride_words));
  if (nq == 0) return 0;
  return ph_fp4_scan_host(call, fp4, nullptr, queries, nq, (uint32_t)r, (uint32_t)r, filter, filter_stride_words, out_ids, out_d,
                          out_len);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_fp4_scan_search_filtered_device(const phnsw_store *fp4, const phnsw_store *full, const float *queries_dev,
                                                     uint32_t ldq, uint64_t nq, uint64_t r, uint64_t k,
                                                     const uint32_t *filter_dev, uint32_t filter_stride_words,
                                                     uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                     void *stream) try {
  const char *const call = "phnsw_fp4_scan_search_filtered_device";
  PH_TRY(ph_fp4_scan_search_check(call, fp4, full, nq, r, k));
  PH_TRY(filter_check(call, fp4, filter_dev, filter_stride_words));
  if (nq == 0) return 0;
  PH_TRY(ph_fp4_scan_device_check(call, queries_dev, ldq, full->ld, true, out_ids_dev, out_d_dev, out_len_dev));
  PH_TRY(ph_fp4_scan_enqueue(fp4, queries_dev, ldq, nq, (uint32_t)r, filter_dev, filter_stride_words, out_ids_dev, out_d_dev,
                             out_len_dev, (hipStream_t)stream));
  return ph_rerank_launch(full, queries_dev, ldq, nq, (uint32_t)r, (uint32_t)k, out_len_dev, out_ids_dev, out_d_dev, (hipStream_t)stream);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_fp4_scan_search_filtered(const phnsw_store *fp4, const phnsw_store *full, const float *queries, uint64_t nq,
                                              uint64_t r, uint64_t k, const uint32_t *filter, uint32_t filter_stride_words,
                                              uint64_t *out_ids, float *out_d, uint64_t *out_len) try {
  const char *const call = "phnsw_fp4_scan_search_filtered";
  PH_TRY(ph_fp4_scan_search_check(call, fp4, full, nq, r, k));
  PH_TRY(filter_check(call, fp4, filter, filter_stride_words));
  if (nq == 0) return 0;
  return ph_fp4_scan_host(call, fp4, full, queries, nq, (uint32_t)r, (uint32_t)k, filter, filter_stride_words, out_ids, out_d,
                          out_len);
} catch (...) { return ph_caught(); }
