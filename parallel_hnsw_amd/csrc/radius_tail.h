// The tail of the exact radius calls, written once for filter_radius.hip (candidates of one shared bitmap, distances
// from tables) and filter_list_radius.hip (candidates of a list per query, distances from dist.batch): what follows once
// a record pool in radius_plan.h's layout has been filled --
//
//   ph_radius_init_kernel    before the fill: count[q] = 0, the cursor = 0, status[q] = 0 or the refusal's status
//   ph_radius_tail           the exclusive sum of count [nq + 1] into out_first; the cursor is the total, read back when
//                            there is a pool (or the host form wants it): the one synchronisation of the tail; total <=
//                            cap: two stable radix passes, by key and then by query
//   ph_radius_unpack         sorted record i is entry i of the CSR arrays
//
// (The kernels are kernels of the header: each unit launches its own copy.)
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "call_set.h"
#include "phnsw_device.h"
#include "radius_plan.h"

[[maybe_unused]] static __global__ __launch_bounds__(256) void ph_radius_init_kernel(uint32_t *count, unsigned long long *cursor,
                                                                                     const uint32_t *refuse, uint32_t *status,
                                                                                     uint64_t nq) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q <= nq; q += (uint64_t)gridDim.x * 256u) {
    count[q] = 0u;
    if (q < nq) status[q] = refuse ? refuse[q] : ST_OK;
    if (q == 0) cursor[0] = 0ull;
  }
}

// sorted record i is entry i of the CSR arrays: the records are in (query, key) order and out_first is the exclusive
// sum of the queries' counts
template <class Id>
__global__ __launch_bounds__(256) void ph_radius_unpack_kernel(const uint64_t *keys, uint64_t total, Id *out_ids, float *out_d) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t key = keys[i];
    out_ids[i] = (Id)((uint32_t)key & IDM);
    out_d[i] = unfkey((uint32_t)(key >> 32));
  }
}

struct PhRadiusWidenCount {
  __host__ __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; }
};
typedef hipcub::TransformInputIterator<uint64_t, PhRadiusWidenCount, const uint32_t *> PhRadiusCountIter;

// a filled pool and what the tail makes of it; device pointers unless said
struct PhRadiusTail {
  uint64_t nq, cap, records;  // nq <= 2^31 - 2 (checked by the entry points); records: the pool's capacity, 0 = count only
  const unsigned long long *cursor;
  const uint32_t *count;   // [nq + 1], count[nq] == 0
  uint64_t *keys_a, *keys_b;  // [records] each
  uint32_t *qs_a, *qs_b;
  uint64_t *out_first;  // [nq + 1]
  uint64_t *out_total;  // nullable
  bool total_to_host;   // read the total back even when there is no pool
  uint64_t *h_total;    // pinned host word
  // the set of the call and its block for hipCUB's temporaries
  PhCallSet *set;
  void **tmp;
  size_t *tmp_bytes;
  // the caller has ensured `tmp` at ph_radius_tail_sizes().most() or more, BEFORE it enqueued anything that uses the
  // block: the tail then never resizes it.  A caller that uses `tmp` for work of its own ahead of the tail must do so --
  // a block that grows goes back to the pool, and nothing may be queued on it then (call_set.h)
  bool tmp_ready;
  hipStream_t stream;
};

// hipCUB's temporaries for the tail's scan and its two sorts, asked before anything is enqueued
struct PhRadiusTailSizes {
  size_t scan, sort1, sort2;
  size_t most() const { return std::max<size_t>(std::max(scan, std::max(sort1, sort2)), 16u); }
};
static inline int ph_radius_tail_sizes(const PhRadiusTail &t, PhRadiusTailSizes *z) {
  z->scan = z->sort1 = z->sort2 = 0;
  const PhRadiusCountIter counts(t.count, PhRadiusWidenCount());
  PH_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, z->scan, counts, t.out_first, (int)(t.nq + 1u), t.stream));
  if (t.records) {
    PH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, z->sort1, t.keys_a, t.keys_b, t.qs_a, t.qs_b, (int)t.records, 0, 64, t.stream));
    PH_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, z->sort2, t.qs_b, t.qs_a, t.keys_b, t.keys_a, (int)t.records, 0,
                                              ph_radius_query_bits(t.nq), t.stream));
  }
  return 0;
}

// *total is exact (and 0 when it was not read back: the device form's count-only call); *sorted is the (query, key)
// ordered records when ph_radius_emits(*total, cap), else nullptr
static inline int ph_radius_tail(const PhRadiusTail &t, uint64_t *total, const uint64_t **sorted) {
  *total = 0, *sorted = nullptr;
  const int n1 = (int)(t.nq + 1u);
  const PhRadiusCountIter counts(t.count, PhRadiusWidenCount());
  const int qbits = ph_radius_query_bits(t.nq);
  PhRadiusTailSizes z;
  PH_TRY(ph_radius_tail_sizes(t, &z));
  const size_t scan_bytes = z.scan, sort1_bytes = z.sort1, sort2_bytes = z.sort2;
  if (!t.tmp_ready) {
    PH_TRY(t.set->block_ensure(t.tmp, t.tmp_bytes, z.most(), t.stream));
  } else if (!*t.tmp || *t.tmp_bytes < z.most()) {
    ph_set_error("exact radius search: the temporary block (%zu bytes) is smaller than the tail's %zu", *t.tmp_bytes, z.most());
    return PHNSW_E_INVALID;
  }
  size_t bytes = scan_bytes;
  PH_HIP(hipcub::DeviceScan::ExclusiveSum(*t.tmp, bytes, counts, t.out_first, n1, t.stream));
  if (t.out_total) PH_HIP(hipMemcpyAsync(t.out_total, t.cursor, 8, hipMemcpyDeviceToDevice, t.stream));
  if (t.records || t.total_to_host) {
    PH_HIP(hipMemcpyAsync(t.h_total, t.cursor, 8, hipMemcpyDeviceToHost, t.stream));
    PH_HIP(hipStreamSynchronize(t.stream));  // whether and how much to sort
    *total = *t.h_total;
  }
  if (t.records && ph_radius_emits(*total, t.cap)) {  // total <= records: nothing was dropped
    bytes = sort1_bytes;
    PH_HIP(hipcub::DeviceRadixSort::SortPairs(*t.tmp, bytes, t.keys_a, t.keys_b, t.qs_a, t.qs_b, (int)*total, 0, 64, t.stream));
    bytes = sort2_bytes;
    PH_HIP(hipcub::DeviceRadixSort::SortPairs(*t.tmp, bytes, t.qs_b, t.qs_a, t.keys_b, t.keys_a, (int)*total, 0, qbits, t.stream));
    *sorted = t.keys_a;
  }
  return 0;
}

template <class Id>
static inline int ph_radius_unpack(const uint64_t *sorted, uint64_t total, Id *out_ids, float *out_d, hipStream_t stream) {
  hipLaunchKernelGGL(ph_radius_unpack_kernel<Id>, dim3(grid1(total)), dim3(256), 0, stream, sorted, total, out_ids, out_d);
  PH_HIP(hipGetLastError());
  return 0;
}
